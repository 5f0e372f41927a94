// colour.hip.h -- YUV 4:2:0 <-> planar RGB on device for the RGB (6->3) network, gfx950 only.
//
//   yuv420_to_rgb_kernel : packed I420 frames (Y plane H x W, then U, then V, each ceil(H/2) x ceil(W/2); the
//                          frames `in_stride` bytes apart: a Y4M frame payload) -> planar RGB uint8 [B,3,H,W],
//                          the layout fiunet_forward_u8 takes for frame_channels == 3
//   rgb_to_yuv420_kernel : the inverse, writing packed I420 frames `out_stride` bytes apart
//   the 10-bit kernels (yuv420p10_to_rgb / rgb_to_yuv420p10) are the same two templates on uint16 samples
//                          (<uint16_t, VEC>): 10-bit codes in uint16 words, a C420p10 Y4M frame payload, strides counted
//                          in samples, and planar RGB uint16, the layout fiunet_forward_p10 takes.  The template
//                          parameter is the sample type (ColourSample); the uint8_t instantiations compile to the
//                          instructions the 8-bit kernels had before it (only the symbol name changed).
//
// The reference has no colour path, so the conversion is defined here, in integer arithmetic, so that the device
// and a numpy restatement (tests/colour_ref.py) agree bit for bit.  S = 2^14.
//
//   matrix   BT.601 (Kr 0.299, Kb 0.114) or BT.709 (Kr 0.2126, Kb 0.0722); 10-bit only: BT.2020 non-constant
//            luminance (Kr 0.2627, Kb 0.0593); Kg = 1 - Kr - Kb
//   range    limited: Y = 16 + 219 E'Y, C = 128 + 224 E'P;  full: Y = 255 E'Y, C = 128 + 255 E'P
//            ys = 219/255 or 1, cs = 224/255 or 1 (scale per RGB code); yoff = 16 or 0
//            10-bit: Y = 64 + 876 E'Y, C = 512 + 896 E'P;  full: Y = 1023 E'Y, C = 512 + 1023 E'P
//            ys = 876/1023 or 1, cs = 896/1023 or 1; yoff = 64 or 0; chroma centre 512 (128 at 8 bits) and
//            every result clamped to [0, 1023]; input samples above 1023 are read as 1023
//   rnd(x)   floor(x * S + 0.5), in double
//   encode   yr = rnd(Kr ys), yb = rnd(Kb ys), yg = rnd(ys) - yr - yb                 (row sums to rnd(ys))
//            cbr = rnd(-Kr / (2 (1 - Kb)) cs), cbb = rnd(0.5 cs), cbg = -cbr - cbb      (row sums to 0)
//            crr = rnd(0.5 cs), crb = rnd(-Kb / (2 (1 - Kr)) cs), crg = -crr - crb      (row sums to 0)
//            so R = G = B gives Cb = Cr = 128 exactly
//   decode   dy = rnd(1 / ys), dcr = rnd(2 (1 - Kr) / cs), dcb = rnd(2 (1 - Kb) / cs),
//            dgb = rnd(-2 Kb (1 - Kb) / Kg / cs), dgr = rnd(-2 Kr (1 - Kr) / Kg / cs)
//   siting   jpeg (also plain 420 / no tag): a chroma sample sits at the centre of its 2x2 luma block;
//            mpeg2: co-sited with the even luma column, centred vertically.  Outside the image rows and columns
//            are replicated (the last chroma row / column of an odd size covers a 2x1, 1x2 or 1x1 block).
//   Y        clamp((yr R + yg G + yb B + yoff S + S/2) >> 14)
//   Cb, Cr   from sums over n samples: jpeg n = 4, the 2x2 block; mpeg2 n = 8, the horizontal [1,2,1] at
//            x = 2j-1, 2j, 2j+1 times the vertical [1,1] at y = 2i, 2i+1
//            C = clamp((c_r SR + c_g SG + c_b SB + centre n S + n S/2) >> (14 + log2 n))
//   up-sample chroma x16, not rounded: vertical 3 x nearest + 1 x next-nearest row (both sitings); horizontal
//            jpeg 3 x nearest + 1 x next-nearest column (together 9a + 3b + 3c + d), mpeg2 4 x its own sample at an
//            even x, 2 x the sum of the two neighbours at an odd x
//   RGB      with Y' = Y - yoff, U = Cb16 - 16 centre, V = Cr16 - 16 centre (U = Cb16 - 2048 at 8 bits, - 8192 at 10):
//            R = clamp((16 dy Y' + dcr V + 2^17) >> 18), G = clamp((16 dy Y' + dgb U + dgr V + 2^17) >> 18),
//            B = clamp((16 dy Y' + dcb U + 2^17) >> 18); `>>` is an arithmetic shift (round half up)
//            int32 bound: |intermediate| <= ~1.6e8 at 8 bits, <= 6.0e8 at 10 bits over every matrix and range (0.28 of
//            2^31; tests/test_p10_host.py recomputes it from the coefficients).  The encode stays below 2.1e8.  12 bits
//            would overflow: not supported.
//
// 4:2:2 and 4:4:4 (the kernels are in yuv4xx.hip.h) extend this definition along its one remaining axis,
// the sub-sampling pattern; coefficients, range, clamps, the Y row and the RGB stage above are unchanged, and chroma
// reaches the RGB stage at the same x16 unrounded scale.
//   4:4:4    encode, per pixel (n = 1): C = clamp((c_r R + c_g G + c_b B + centre S + S/2) >> 14)
//            decode: Cb16 = 16 Cb, Cr16 = 16 Cr.  Siting has no meaning: accepted and ignored.
//   4:2:2    the horizontal half of the 4:2:0 rule; chroma row y belongs to luma row y
//            encode jpeg (centred): the sum over columns 2j, 2j+1, n = 2, shift 15; mpeg2 (co-sited with the even
//            column): [1,2,1] over 2j-1, 2j, 2j+1, n = 4, shift 16; columns clamped into the image; bias
//            centre n S + n S/2
//            decode: the 4:2:0 horizontal taps times 4: jpeg 4 (3a + b); mpeg2 16a at an even x, 8 (a + b) at an odd x
//            default siting where the caller gives none: mpeg2
//            On chroma that does not change down a column this decode is the 4:2:0 decode, on RGB rows that come in
//            equal pairs chroma row 2i of this encode is chroma row i of the 4:2:0 encode, bit for bit; every
//            intermediate is bounded by its 4:2:0 counterpart, so the int32 bound above carries over
//            (tests/test_yuv4xx_host.py recomputes it).
//
// All four kernels are HBM-bound elementwise work.  A thread covers 4 luma columns of a row (decode) or of a row pair
// (encode), so a wave reads and writes 256 contiguous samples of every luma / RGB row; with W % 4 == 0 and aligned
// bases (VEC) those are single 4-sample accesses (4 bytes at 8 bits, 8 bytes at 10), otherwise samples with the edge
// clamped.  Chroma is read / written per sample (half the columns, one quarter of the samples).
//
// Semi-planar surfaces (NV12 at 8 bits, P010 at 10: what a hardware decoder returns) go through the same
// two bodies with the layout as a template parameter (NV): the arithmetic above is untouched, only where a sample lives
// changes.  A frame is H luma rows `luma_pitch` samples apart, then, `chroma_offset` samples after the frame's base,
// ceil(H/2) chroma rows `chroma_pitch` apart, each ceil(W/2) pairs U0 V0 U1 V1 ...; frames `frame_stride` apart
// (ColourSurface, every field in samples).  A P010 word is code << 6: read as word >> 6 (the low six bits are ignored),
// written with the low six bits zero.  The chroma pairs 2t and 2t+1 a thread owns are adjacent, so with VEC (W, every
// pitch, offset and stride a multiple of 4 samples, bases aligned) they are one 4-sample access - a load in the decode,
// a store in the encode, where I420 takes four scalar accesses - and the decode's two neighbour pairs one 2-sample
// load each; otherwise every access is per sample.  Samples outside the W / 2 ceil(W/2) used columns and between the
// planes are never read and never written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/fiunet.h"

namespace fiunet {

struct ColourCoef {
    int yr, yg, yb, yoff;     // encode, luma row
    int cbr, cbg, cbb;        // encode, Cb row
    int crr, crg, crb;        // encode, Cr row
    int dy, dcr, dgb, dgr, dcb;  // decode
    int mpeg2;                // siting
};

constexpr unsigned kColourFlags = FIUNET_YUV_MPEG2 | FIUNET_YUV_BT709 | FIUNET_YUV_FULL_RANGE;
constexpr unsigned kColourFlagsP10 = kColourFlags | FIUNET_YUV_BT2020;   // BT.2020 is defined for 10 and 12 bits only

inline int colour_rnd(double x) { return (int)std::floor(x * 16384.0 + 0.5); }

// bits: 8 (ABI v6) or 10 (ABI v7); the flags are checked by the caller (FIUNET_YUV_BT2020 only with 10)
inline ColourCoef colour_coef(unsigned flags, int bits = 8)
{
    const bool full = flags & FIUNET_YUV_FULL_RANGE, bt709 = flags & FIUNET_YUV_BT709,
               bt2020 = flags & FIUNET_YUV_BT2020, p10 = bits == 10;
    const double kr = bt2020 ? 0.2627 : bt709 ? 0.2126 : 0.299, kb = bt2020 ? 0.0593 : bt709 ? 0.0722 : 0.114,
                 kg = 1.0 - kr - kb;
    const double ys = full ? 1.0 : p10 ? 876.0 / 1023.0 : 219.0 / 255.0,
                 cs = full ? 1.0 : p10 ? 896.0 / 1023.0 : 224.0 / 255.0;
    ColourCoef k;
    k.yr = colour_rnd(kr * ys);
    k.yb = colour_rnd(kb * ys);
    k.yg = colour_rnd(ys) - k.yr - k.yb;
    k.yoff = full ? 0 : p10 ? 64 : 16;
    k.cbr = colour_rnd(-kr / (2.0 * (1.0 - kb)) * cs);
    k.cbb = colour_rnd(0.5 * cs);
    k.cbg = -k.cbr - k.cbb;
    k.crr = colour_rnd(0.5 * cs);
    k.crb = colour_rnd(-kb / (2.0 * (1.0 - kr)) * cs);
    k.crg = -k.crr - k.crb;
    k.dy = colour_rnd(1.0 / ys);
    k.dcr = colour_rnd(2.0 * (1.0 - kr) / cs);
    k.dcb = colour_rnd(2.0 * (1.0 - kb) / cs);
    k.dgb = colour_rnd(-2.0 * kb * (1.0 - kb) / kg / cs);
    k.dgr = colour_rnd(-2.0 * kr * (1.0 - kr) / kg / cs);
    k.mpeg2 = (flags & FIUNET_YUV_MPEG2) ? 1 : 0;
    return k;
}

// The sample types: 8-bit I420 (ABI v6) and 10-bit codes in uint16 words (ABI v7).  read() is how a kernel takes an
// input sample (10 bits: anything above 1023 reads as 1023), clamp() how it stores a result.
template <typename T>
struct ColourSample;
template <>
struct ColourSample<uint8_t> {
    static constexpr int kMax = 255, kCentre = 128;
    using Vec4 = uchar4;
    using Vec2 = uchar2;
    __device__ static __forceinline__ int read(uint8_t v) { return v; }
    __device__ static __forceinline__ uint8_t clamp(int v) { return (uint8_t)min(max(v, 0), 255); }
    __device__ static __forceinline__ Vec4 make(uint8_t a, uint8_t b, uint8_t c, uint8_t d) { return make_uchar4(a, b, c, d); }
};
template <>
struct ColourSample<uint16_t> {
    static constexpr int kMax = 1023, kCentre = 512;
    using Vec4 = ushort4;
    using Vec2 = ushort2;
    __device__ static __forceinline__ int read(uint16_t v) { return min((int)v, 1023); }
    __device__ static __forceinline__ uint16_t clamp(int v) { return (uint16_t)min(max(v, 0), 1023); }
    __device__ static __forceinline__ Vec4 make(uint16_t a, uint16_t b, uint16_t c, uint16_t d)
    {
        return make_ushort4(a, b, c, d);
    }
};

// A semi-planar surface, every field in samples and resolved by the caller (no zeros): see the head of this file.
struct ColourSurface {
    size_t luma_pitch, chroma_offset, chroma_pitch, frame_stride;
};

// How a stored YUV word holds its code.  Planar frames (NV = false): the code itself (ColourSample).  Semi-planar
// surfaces: the same at 8 bits (NV12); at 10 bits (P010) the code sits in the upper ten bits of the word.
template <typename T, bool NV>
struct ColourWord {
    static constexpr int kShift = (NV && sizeof(T) == 2) ? 6 : 0;
    __device__ static __forceinline__ int read(T v) { return kShift ? (int)(v >> kShift) : ColourSample<T>::read(v); }
    __device__ static __forceinline__ T store(int v) { return (T)(ColourSample<T>::clamp(v) << kShift); }
};

constexpr int kColourBlock = 128;   // threads per workgroup; each covers 4 luma columns

// The decode of one thread.  NV = false: packed I420 frames sf.frame_stride apart (the other fields unused); NV = true:
// the semi-planar surface sf.  Strides and offsets in samples.
template <typename T, bool VEC, bool NV>
__device__ __forceinline__ void colour_decode(const T* __restrict__ in, const ColourSurface& sf, T* __restrict__ out,
                                              int H, int W, const ColourCoef& k)
{
    using S = ColourSample<T>;
    using Y = ColourWord<T, NV>;
    using Vec4 = typename S::Vec4;
    using Vec2 = typename S::Vec2;
    const int t = blockIdx.x * kColourBlock + threadIdx.x, x0 = 4 * t, y = blockIdx.y;
    if (x0 >= W) return;
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const size_t plane = (size_t)H * W;
    const T* fy = in + (size_t)blockIdx.z * sf.frame_stride;
    // chroma rows: the nearest (weight 3) and the next-nearest (weight 1), both sitings
    const int i0 = y >> 1, i1 = min(max((y & 1) ? i0 + 1 : i0 - 1, 0), Hc - 1);
    // chroma columns 2t-1 .. 2t+2 (clamped) cover every neighbour of luma columns 4t .. 4t+3
    int u4[4], v4[4];
    if (NV) {
        const T* c0 = fy + sf.chroma_offset + (size_t)i0 * sf.chroma_pitch;
        const T* c1 = fy + sf.chroma_offset + (size_t)i1 * sf.chroma_pitch;
        if (VEC) {
            // W % 4 == 0: pairs 2t and 2t+1 exist and lie at samples 4t .. 4t+3 of the row; the neighbours are one pair each
            const int jl = max(2 * t - 1, 0), jr = min(2 * t + 2, Wc - 1);
            const Vec4 m0 = *reinterpret_cast<const Vec4*>(c0 + 4 * t), m1 = *reinterpret_cast<const Vec4*>(c1 + 4 * t);
            const Vec2 l0 = *reinterpret_cast<const Vec2*>(c0 + 2 * jl), l1 = *reinterpret_cast<const Vec2*>(c1 + 2 * jl);
            const Vec2 r0 = *reinterpret_cast<const Vec2*>(c0 + 2 * jr), r1 = *reinterpret_cast<const Vec2*>(c1 + 2 * jr);
            u4[0] = 3 * Y::read(l0.x) + Y::read(l1.x); v4[0] = 3 * Y::read(l0.y) + Y::read(l1.y);
            u4[1] = 3 * Y::read(m0.x) + Y::read(m1.x); v4[1] = 3 * Y::read(m0.y) + Y::read(m1.y);
            u4[2] = 3 * Y::read(m0.z) + Y::read(m1.z); v4[2] = 3 * Y::read(m0.w) + Y::read(m1.w);
            u4[3] = 3 * Y::read(r0.x) + Y::read(r1.x); v4[3] = 3 * Y::read(r0.y) + Y::read(r1.y);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = min(max(2 * t - 1 + q, 0), Wc - 1);
                u4[q] = 3 * Y::read(c0[2 * j]) + Y::read(c1[2 * j]);
                v4[q] = 3 * Y::read(c0[2 * j + 1]) + Y::read(c1[2 * j + 1]);
            }
        }
    } else {
        const T* fu = fy + plane;
        const T* fv = fu + (size_t)Hc * Wc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = min(max(2 * t - 1 + q, 0), Wc - 1);
            u4[q] = 3 * S::read(fu[(size_t)i0 * Wc + j]) + S::read(fu[(size_t)i1 * Wc + j]);
            v4[q] = 3 * S::read(fv[(size_t)i0 * Wc + j]) + S::read(fv[(size_t)i1 * Wc + j]);
        }
    }
    int yv[4];
    const T* row = fy + (size_t)y * (NV ? sf.luma_pitch : (size_t)W) + x0;
    if (VEC) {
        const Vec4 p = *reinterpret_cast<const Vec4*>(row);
        yv[0] = Y::read(p.x); yv[1] = Y::read(p.y); yv[2] = Y::read(p.z); yv[3] = Y::read(p.w);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) yv[c] = Y::read(row[min(c, W - 1 - x0)]);
    }
    T r[4], g[4], b[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // pixel x0 + c: nearest chroma column index 1 + (c >> 1) in u4 / v4; jpeg's next-nearest is to the left at an
        // even x and to the right at an odd x; mpeg2 takes its own sample at an even x and the two neighbours at an odd x
        const int n = 1 + (c >> 1), f = (c & 1) ? n + 1 : n - 1;
        int U, V;
        if (k.mpeg2) {
            U = (c & 1) ? 2 * (u4[n] + u4[n + 1]) : 4 * u4[n];
            V = (c & 1) ? 2 * (v4[n] + v4[n + 1]) : 4 * v4[n];
        } else {
            U = 3 * u4[n] + u4[f];
            V = 3 * v4[n] + v4[f];
        }
        U -= 16 * S::kCentre;
        V -= 16 * S::kCentre;
        const int yy = 16 * k.dy * (yv[c] - k.yoff) + (1 << 17);
        r[c] = S::clamp((yy + k.dcr * V) >> 18);
        g[c] = S::clamp((yy + k.dgb * U + k.dgr * V) >> 18);
        b[c] = S::clamp((yy + k.dcb * U) >> 18);
    }
    T* o = out + (size_t)blockIdx.z * 3 * plane + (size_t)y * W + x0;
    if (VEC) {
        *reinterpret_cast<Vec4*>(o) = S::make(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<Vec4*>(o + plane) = S::make(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<Vec4*>(o + 2 * plane) = S::make(b[0], b[1], b[2], b[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (x0 + c < W) {
                o[c] = r[c];
                o[plane + c] = g[c];
                o[2 * plane + c] = b[c];
            }
    }
}

// grid = (ceil(ceil(W/4) / 128), H, B); strides and offsets in samples
template <typename T, bool VEC>
__global__ __launch_bounds__(kColourBlock) void yuv420_to_rgb_kernel(const T* __restrict__ in, size_t in_stride,
                                                                     T* __restrict__ out, int H, int W, ColourCoef k)
{
    colour_decode<T, VEC, false>(in, ColourSurface{0, 0, 0, in_stride}, out, H, W, k);
}

// the same grid; NV12 (uint8_t) / P010 (uint16_t) surfaces `sf` -> planar RGB codes
template <typename T, bool VEC>
__global__ __launch_bounds__(kColourBlock) void nv12_to_rgb_kernel(const T* __restrict__ in, ColourSurface sf,
                                                                   T* __restrict__ out, int H, int W, ColourCoef k)
{
    colour_decode<T, VEC, true>(in, sf, out, H, W, k);
}

// The encode of one thread: luma rows 2i, 2i+1 and columns 4t .. 4t+3, i.e. chroma samples (i, 2t) and (i, 2t+1).
// NV as for colour_decode.
template <typename T, bool VEC, bool NV>
__device__ __forceinline__ void colour_encode(const T* __restrict__ in, T* __restrict__ out, const ColourSurface& sf,
                                              int H, int W, const ColourCoef& k)
{
    using S = ColourSample<T>;
    using Y = ColourWord<T, NV>;
    using Vec4 = typename S::Vec4;
    const int t = blockIdx.x * kColourBlock + threadIdx.x, x0 = 4 * t, i = blockIdx.y;
    if (x0 >= W) return;
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const size_t plane = (size_t)H * W;
    const int ya = 2 * i, yb = min(2 * i + 1, H - 1);
    const T* src = in + (size_t)blockIdx.z * 3 * plane;
    // px[ch][row][1 + c] = channel ch at (row ya / yb, column x0 + c), c = -1 .. 3, columns clamped into the image
    int px[3][2][5];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const T* row = src + ch * plane + (size_t)(rr ? yb : ya) * W;
            px[ch][rr][0] = S::read(row[max(x0 - 1, 0)]);
            if (VEC) {
                const Vec4 p = *reinterpret_cast<const Vec4*>(row + x0);
                px[ch][rr][1] = S::read(p.x); px[ch][rr][2] = S::read(p.y);
                px[ch][rr][3] = S::read(p.z); px[ch][rr][4] = S::read(p.w);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) px[ch][rr][1 + c] = S::read(row[min(x0 + c, W - 1)]);
            }
        }
    T* fy = out + (size_t)blockIdx.z * sf.frame_stride;
    T* fu = fy + plane;                  // I420: the U and V planes
    T* fv = fu + (size_t)Hc * Wc;
    T* fc = fy + sf.chroma_offset + (size_t)i * sf.chroma_pitch;   // NV: this thread's row of U,V pairs
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        if (2 * i + rr >= H) break;
        T yv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            yv[c] = Y::store((k.yr * px[0][rr][1 + c] + k.yg * px[1][rr][1 + c] + k.yb * px[2][rr][1 + c] +
                              k.yoff * 16384 + 8192) >> 14);
        T* o = fy + (size_t)(2 * i + rr) * (NV ? sf.luma_pitch : (size_t)W) + x0;
        if (VEC) {
            *reinterpret_cast<Vec4*>(o) = S::make(yv[0], yv[1], yv[2], yv[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (x0 + c < W) o[c] = yv[c];
        }
    }
    T cu[2], cv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int j = 2 * t + m;
        if (!(NV && VEC) && j >= Wc) break;   // (NV && VEC: W % 4 == 0, both pairs exist)
        int s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            // local column of luma x = 2j is 1 + 2m in px; jpeg: 2j, 2j+1; mpeg2: [1,2,1] over 2j-1, 2j, 2j+1
            const int a = 1 + 2 * m;
            s[ch] = 0;
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
                s[ch] += k.mpeg2 ? px[ch][rr][a - 1] + 2 * px[ch][rr][a] + px[ch][rr][a + 1]
                                 : px[ch][rr][a] + px[ch][rr][a + 1];
        }
        const int sh = k.mpeg2 ? 17 : 16, bias = (S::kCentre << sh) + (1 << (sh - 1));
        cu[m] = Y::store((k.cbr * s[0] + k.cbg * s[1] + k.cbb * s[2] + bias) >> sh);
        cv[m] = Y::store((k.crr * s[0] + k.crg * s[1] + k.crb * s[2] + bias) >> sh);
        if (!NV) {
            fu[(size_t)i * Wc + j] = cu[m];
            fv[(size_t)i * Wc + j] = cv[m];
        } else if (!VEC) {
            fc[2 * j] = cu[m];
            fc[2 * j + 1] = cv[m];
        }
    }
    if (NV && VEC) *reinterpret_cast<Vec4*>(fc + 4 * t) = S::make(cu[0], cv[0], cu[1], cv[1]);   // U V U V, one store
}

// grid = (ceil(ceil(W/4) / 128), ceil(H/2), B)
template <typename T, bool VEC>
__global__ __launch_bounds__(kColourBlock) void rgb_to_yuv420_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                     size_t out_stride, int H, int W, ColourCoef k)
{
    colour_encode<T, VEC, false>(in, out, ColourSurface{0, 0, 0, out_stride}, H, W, k);
}

// the same grid; planar RGB codes -> NV12 (uint8_t) / P010 (uint16_t) surfaces `sf`
template <typename T, bool VEC>
__global__ __launch_bounds__(kColourBlock) void rgb_to_nv12_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                   ColourSurface sf, int H, int W, ColourCoef k)
{
    colour_encode<T, VEC, true>(in, out, sf, H, W, k);
}

}  // namespace fiunet
