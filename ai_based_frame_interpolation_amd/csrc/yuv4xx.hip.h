// yuv4xx.hip.h -- YUV 4:2:2 and 4:4:4 <-> planar RGB on device for the RGB (6->3) network, gfx950 only.
//
// The arithmetic is the one defined at the head of colour.hip.h (coefficients, ranges, clamps, the Y row and the
// `>> 18` RGB stage are shared: ColourCoef, ColourSample); this file adds the two sub-sampling patterns that file's
// bodies do not have, and the two packed 4:2:2 layouts.  One decode body and one encode body, with the pattern and the
// packing as the compile-time parameter FMT (fiunet_yuv_format):
//
//   FIUNET_YUV_422P     planar: Y plane H x W, then U, then V, each H x ceil(W/2) (yuv422p / yuv422p10le)
//   FIUNET_YUV_444P     planar: Y, U, V each H x W                                 (yuv444p / yuv444p10le)
//   FIUNET_YUV_UYVY422  one plane, U0 Y0 V0 Y1 per two pixels, 8 bits, even W      (uyvy422)
//   FIUNET_YUV_YUYV422  one plane, Y0 U0 Y1 V0 per two pixels, 8 bits, even W      (yuyv422)
//
// 4:4:4   encode, per pixel (n = 1): C = clamp((c_r R + c_g G + c_b B + centre S + S/2) >> 14)
//         decode: Cb16 = 16 Cb, Cr16 = 16 Cr.  Siting has no meaning and is ignored.
// 4:2:2   the horizontal half of the 4:2:0 rule; chroma row y belongs to luma row y.
//         encode jpeg (centred): columns 2j, 2j+1, n = 2, shift 15; mpeg2 (co-sited with the even column): [1,2,1] over
//         2j-1, 2j, 2j+1, n = 4, shift 16; columns clamped into the image; bias centre n S + n S/2
//         decode: the 4:2:0 horizontal taps times 4: jpeg 4 (3a + b); mpeg2 16a at an even x, 8 (a + b) at an odd x
// so on chroma that does not change down a column the 4:2:2 decode is the 4:2:0 decode (3a + a = 4a), on RGB rows that
// come in equal pairs the 4:2:2 chroma row 2i is the 4:2:0 chroma row i (both sums and the shift halve), and every
// intermediate is bounded by its 4:2:0 counterpart: the int32 argument of colour.hip.h carries over.
//
// Thread shape as in colour.hip.h, but both directions run one thread-row per luma row: a thread covers 4 luma columns
// of one row, grid = (ceil(ceil(W/4) / 128), H, B).  With VEC (W % 4 == 0; bases, strides and pitches multiples of 4
// samples: the host decides) the luma / RGB quads and the 4:4:4 chroma quads are single 4-sample accesses, the
// thread's two 4:2:2 chroma samples per plane one 2-sample access, and its 4 packed pixels one 8-byte access declared
// dword-aligned; the decode's left and right chroma neighbours are scalar (planar) or one dword each (packed).  Without
// VEC every access is per sample with the edge clamped.  No byte outside the used columns of a pitched row is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "colour.hip.h"

namespace fiunet {

// Where the frames lie, resolved by the caller (no zeros where a value is used).  Planar formats: frames
// `frame_stride` samples apart, tight inside (row_pitch unused).  Packed formats: rows `row_pitch` bytes apart.
struct YuvLayout {
    size_t row_pitch, frame_stride;
};

constexpr bool yuv_is_packed(int fmt) { return fmt == FIUNET_YUV_UYVY422 || fmt == FIUNET_YUV_YUYV422; }
constexpr bool yuv_is_444(int fmt) { return fmt == FIUNET_YUV_444P; }

// 8 packed bytes = 4 pixels of a packed 4:2:2 row, as one access that asks for dword alignment only
typedef uint32_t YuvQuad __attribute__((ext_vector_type(2), aligned(4)));

// byte offsets inside a 4-byte group U0 Y0 V0 Y1 (UYVY) / Y0 U0 Y1 V0 (YUYV): luma of the even / odd pixel, U, V
template <int FMT>
struct YuvPackedOrder {
    static constexpr int kY0 = FMT == FIUNET_YUV_UYVY422 ? 1 : 0, kY1 = kY0 + 2;
    static constexpr int kU = FMT == FIUNET_YUV_UYVY422 ? 0 : 1, kV = kU + 2;
};

__device__ __forceinline__ int yuv_byte(uint32_t w, int i) { return (int)((w >> (8 * i)) & 0xFFu); }

// The decode of one thread: luma row y, columns 4t .. 4t+3.
template <typename T, int FMT, bool VEC>
__device__ __forceinline__ void yuv_decode(const T* __restrict__ in, const YuvLayout& lay, T* __restrict__ out, int H,
                                           int W, const ColourCoef& k)
{
    using S = ColourSample<T>;
    using Vec4 = typename S::Vec4;
    using Vec2 = typename S::Vec2;
    using O = YuvPackedOrder<FMT>;
    const int t = blockIdx.x * kColourBlock + threadIdx.x, x0 = 4 * t, y = blockIdx.y;
    if (x0 >= W) return;
    const size_t plane = (size_t)H * W;
    const T* f = in + (size_t)blockIdx.z * lay.frame_stride;
    int yv[4], U[4], V[4];   // luma codes and chroma x16 of the 4 pixels
    if (yuv_is_444(FMT)) {
        const T* py = f + (size_t)y * W + x0;
        if (VEC) {
            const Vec4 a = *reinterpret_cast<const Vec4*>(py), u = *reinterpret_cast<const Vec4*>(py + plane),
                       v = *reinterpret_cast<const Vec4*>(py + 2 * plane);
            yv[0] = S::read(a.x); yv[1] = S::read(a.y); yv[2] = S::read(a.z); yv[3] = S::read(a.w);
            U[0] = S::read(u.x); U[1] = S::read(u.y); U[2] = S::read(u.z); U[3] = S::read(u.w);
            V[0] = S::read(v.x); V[1] = S::read(v.y); V[2] = S::read(v.z); V[3] = S::read(v.w);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int cc = min(c, W - 1 - x0);
                yv[c] = S::read(py[cc]);
                U[c] = S::read(py[plane + cc]);
                V[c] = S::read(py[2 * plane + cc]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            U[c] *= 16;
            V[c] *= 16;
        }
    } else {
        const int Wc = (W + 1) >> 1;
        // chroma columns 2t-1 .. 2t+2 (clamped) cover every neighbour of luma columns 4t .. 4t+3; x4, the weight the
        // two vertical taps of 4:2:0 add up to
        int u4[4], v4[4];
        const int jl = max(2 * t - 1, 0), jr = min(2 * t + 2, Wc - 1);
        if (yuv_is_packed(FMT)) {
            const uint8_t* row = reinterpret_cast<const uint8_t*>(f) + (size_t)y * lay.row_pitch;
            if (VEC) {
                // W % 4 == 0: groups 2t and 2t+1 exist and are the 8 bytes at 8t; the neighbours are one dword each
                const YuvQuad m = *reinterpret_cast<const YuvQuad*>(row + 8 * (size_t)t);
                const uint32_t l = *reinterpret_cast<const uint32_t*>(row + 4 * (size_t)jl),
                               r = *reinterpret_cast<const uint32_t*>(row + 4 * (size_t)jr);
                u4[0] = yuv_byte(l, O::kU); v4[0] = yuv_byte(l, O::kV);
                u4[1] = yuv_byte(m.x, O::kU); v4[1] = yuv_byte(m.x, O::kV);
                u4[2] = yuv_byte(m.y, O::kU); v4[2] = yuv_byte(m.y, O::kV);
                u4[3] = yuv_byte(r, O::kU); v4[3] = yuv_byte(r, O::kV);
                yv[0] = yuv_byte(m.x, O::kY0); yv[1] = yuv_byte(m.x, O::kY1);
                yv[2] = yuv_byte(m.y, O::kY0); yv[3] = yuv_byte(m.y, O::kY1);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = min(max(2 * t - 1 + q, 0), Wc - 1);
                    u4[q] = row[4 * (size_t)j + O::kU];
                    v4[q] = row[4 * (size_t)j + O::kV];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int x = min(x0 + c, W - 1);   // (W is even: pixel x is in group x >> 1)
                    yv[c] = row[4 * (size_t)(x >> 1) + ((x & 1) ? O::kY1 : O::kY0)];
                }
            }
        } else {
            const T* fu = f + plane + (size_t)y * Wc;
            const T* fv = fu + (size_t)H * Wc;
            if (VEC) {
                const Vec2 mu = *reinterpret_cast<const Vec2*>(fu + 2 * t), mv = *reinterpret_cast<const Vec2*>(fv + 2 * t);
                u4[0] = S::read(fu[jl]); v4[0] = S::read(fv[jl]);
                u4[1] = S::read(mu.x); v4[1] = S::read(mv.x);
                u4[2] = S::read(mu.y); v4[2] = S::read(mv.y);
                u4[3] = S::read(fu[jr]); v4[3] = S::read(fv[jr]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = min(max(2 * t - 1 + q, 0), Wc - 1);
                    u4[q] = S::read(fu[j]);
                    v4[q] = S::read(fv[j]);
                }
            }
            const T* py = f + (size_t)y * W + x0;
            if (VEC) {
                const Vec4 a = *reinterpret_cast<const Vec4*>(py);
                yv[0] = S::read(a.x); yv[1] = S::read(a.y); yv[2] = S::read(a.z); yv[3] = S::read(a.w);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) yv[c] = S::read(py[min(c, W - 1 - x0)]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u4[q] *= 4;
            v4[q] *= 4;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // the horizontal taps of colour_decode: nearest column index 1 + (c >> 1) in u4 / v4
            const int n = 1 + (c >> 1), nn = (c & 1) ? n + 1 : n - 1;
            if (k.mpeg2) {
                U[c] = (c & 1) ? 2 * (u4[n] + u4[n + 1]) : 4 * u4[n];
                V[c] = (c & 1) ? 2 * (v4[n] + v4[n + 1]) : 4 * v4[n];
            } else {
                U[c] = 3 * u4[n] + u4[nn];
                V[c] = 3 * v4[n] + v4[nn];
            }
        }
    }
    T r[4], g[4], b[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int u = U[c] - 16 * S::kCentre, v = V[c] - 16 * S::kCentre;
        const int yy = 16 * k.dy * (yv[c] - k.yoff) + (1 << 17);
        r[c] = S::clamp((yy + k.dcr * v) >> 18);
        g[c] = S::clamp((yy + k.dgb * u + k.dgr * v) >> 18);
        b[c] = S::clamp((yy + k.dcb * u) >> 18);
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

// grid = (ceil(ceil(W/4) / 128), H, B)
template <typename T, int FMT, bool VEC>
__global__ __launch_bounds__(kColourBlock) void yuv_to_rgb_kernel(const T* __restrict__ in, YuvLayout lay,
                                                                  T* __restrict__ out, int H, int W, ColourCoef k)
{
    yuv_decode<T, FMT, VEC>(in, lay, out, H, W, k);
}

// The encode of one thread: luma row y, columns 4t .. 4t+3; 4:2:2: chroma samples (y, 2t) and (y, 2t+1).
template <typename T, int FMT, bool VEC>
__device__ __forceinline__ void yuv_encode(const T* __restrict__ in, T* __restrict__ out, const YuvLayout& lay, int H,
                                           int W, const ColourCoef& k)
{
    using S = ColourSample<T>;
    using Vec4 = typename S::Vec4;
    using Vec2 = typename S::Vec2;
    using O = YuvPackedOrder<FMT>;
    const int t = blockIdx.x * kColourBlock + threadIdx.x, x0 = 4 * t, y = blockIdx.y;
    if (x0 >= W) return;
    const size_t plane = (size_t)H * W;
    const T* src = in + (size_t)blockIdx.z * 3 * plane + (size_t)y * W;
    // px[ch][1 + c] = channel ch at column x0 + c, c = -1 .. 3, columns clamped into the image
    int px[3][5];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const T* row = src + ch * plane;
        px[ch][0] = S::read(row[max(x0 - 1, 0)]);
        if (VEC) {
            const Vec4 p = *reinterpret_cast<const Vec4*>(row + x0);
            px[ch][1] = S::read(p.x); px[ch][2] = S::read(p.y); px[ch][3] = S::read(p.z); px[ch][4] = S::read(p.w);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) px[ch][1 + c] = S::read(row[min(x0 + c, W - 1)]);
        }
    }
    T yv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        yv[c] = S::clamp((k.yr * px[0][1 + c] + k.yg * px[1][1 + c] + k.yb * px[2][1 + c] + k.yoff * 16384 + 8192) >> 14);
    T* f = out + (size_t)blockIdx.z * lay.frame_stride;
    if (yuv_is_444(FMT)) {
        T cu[4], cv[4];
        const int bias = (S::kCentre << 14) + (1 << 13);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            cu[c] = S::clamp((k.cbr * px[0][1 + c] + k.cbg * px[1][1 + c] + k.cbb * px[2][1 + c] + bias) >> 14);
            cv[c] = S::clamp((k.crr * px[0][1 + c] + k.crg * px[1][1 + c] + k.crb * px[2][1 + c] + bias) >> 14);
        }
        T* o = f + (size_t)y * W + x0;
        if (VEC) {
            *reinterpret_cast<Vec4*>(o) = S::make(yv[0], yv[1], yv[2], yv[3]);
            *reinterpret_cast<Vec4*>(o + plane) = S::make(cu[0], cu[1], cu[2], cu[3]);
            *reinterpret_cast<Vec4*>(o + 2 * plane) = S::make(cv[0], cv[1], cv[2], cv[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (x0 + c < W) {
                    o[c] = yv[c];
                    o[plane + c] = cu[c];
                    o[2 * plane + c] = cv[c];
                }
        }
        return;
    }
    const int Wc = (W + 1) >> 1;
    T cu[2], cv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        // local column of luma x = 2j (j = 2t + m) is 1 + 2m in px; jpeg: 2j, 2j+1; mpeg2: [1,2,1] over 2j-1, 2j, 2j+1
        const int a = 1 + 2 * m;
        int s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            s[ch] = k.mpeg2 ? px[ch][a - 1] + 2 * px[ch][a] + px[ch][a + 1] : px[ch][a] + px[ch][a + 1];
        const int sh = k.mpeg2 ? 16 : 15, bias = (S::kCentre << sh) + (1 << (sh - 1));
        cu[m] = S::clamp((k.cbr * s[0] + k.cbg * s[1] + k.cbb * s[2] + bias) >> sh);
        cv[m] = S::clamp((k.crr * s[0] + k.crg * s[1] + k.crb * s[2] + bias) >> sh);
    }
    if (yuv_is_packed(FMT)) {
        uint8_t* row = reinterpret_cast<uint8_t*>(f) + (size_t)y * lay.row_pitch;
        if (VEC) {
            YuvQuad q;
            q.x = (uint32_t)yv[0] << (8 * O::kY0) | (uint32_t)yv[1] << (8 * O::kY1) | (uint32_t)cu[0] << (8 * O::kU) |
                  (uint32_t)cv[0] << (8 * O::kV);
            q.y = (uint32_t)yv[2] << (8 * O::kY0) | (uint32_t)yv[3] << (8 * O::kY1) | (uint32_t)cu[1] << (8 * O::kU) |
                  (uint32_t)cv[1] << (8 * O::kV);
            *reinterpret_cast<YuvQuad*>(row + 8 * (size_t)t) = q;
        } else {
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int j = 2 * t + m;
                if (j >= Wc) break;   // (W is even: a group is whole or absent)
                uint8_t* p = row + 4 * (size_t)j;
                p[O::kY0] = (uint8_t)yv[2 * m];
                p[O::kY1] = (uint8_t)yv[2 * m + 1];
                p[O::kU] = (uint8_t)cu[m];
                p[O::kV] = (uint8_t)cv[m];
            }
        }
        return;
    }
    T* o = f + (size_t)y * W + x0;
    T* fu = f + plane + (size_t)y * Wc;
    T* fv = fu + (size_t)H * Wc;
    if (VEC) {
        *reinterpret_cast<Vec4*>(o) = S::make(yv[0], yv[1], yv[2], yv[3]);
        Vec2 u2, v2;
        u2.x = cu[0]; u2.y = cu[1];
        v2.x = cv[0]; v2.y = cv[1];
        *reinterpret_cast<Vec2*>(fu + 2 * t) = u2;
        *reinterpret_cast<Vec2*>(fv + 2 * t) = v2;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (x0 + c < W) o[c] = yv[c];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int j = 2 * t + m;
            if (j >= Wc) break;
            fu[j] = cu[m];
            fv[j] = cv[m];
        }
    }
}

// the same grid
template <typename T, int FMT, bool VEC>
__global__ __launch_bounds__(kColourBlock) void rgb_to_yuv_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                                  YuvLayout lay, int H, int W, ColourCoef k)
{
    yuv_encode<T, FMT, VEC>(in, out, lay, H, W, k);
}

}  // namespace fiunet
