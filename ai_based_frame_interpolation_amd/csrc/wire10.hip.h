// wire10.hip.h -- 10-bit 4:2:2 wire packings <-> the planar yuv422p10le working format, gfx950 only.
//
// v210, y210le and p210le carry the samples of yuv422p10le; only where the bits lie differs.  The working format is
// yuv422p10le as yuv4xx.hip.h reads it: tight frames of uint16 words holding the code, Y H x W, then U, then V, each
// H x ceil(W/2), frames `frame_stride` samples apart.  Every wire word is little-endian.  The packing is the compile-
// time parameter P (fiunet_packing10):
//
//   FIUNET_PACK10_V210  one plane, W even.  Group g holds pixels 6g .. 6g+5 in four 32-bit words, each with a low, a
//                       middle and a high 10-bit field (bits 0-9, 10-19, 20-29):
//                           w0 = U0 Y0 V0    w1 = Y1 U1 Y2    w2 = V1 Y3 U2    w3 = Y4 V2 Y5
//                       (Uk, Vk: chroma sample 3g + k).  A tight row is 128 * ceil(W / 48) bytes.
//   FIUNET_PACK10_Y210  one plane, W even.  16-bit words Y0 U0 Y1 V0 per two pixels, each word code << 6.  A tight row
//                       is 4 W bytes.
//   FIUNET_PACK10_P210  two planes, any W.  A Y plane of H x W words, then H rows of interleaved U V pairs
//                       (2 ceil(W/2) words), each word code << 6: P010 with chroma of full height.
//
// Reading: bits 30-31 of a v210 word and the low six bits of a y210 / p210 word are ignored whatever they hold; v210
// fields past column W and row padding are never interpreted.  Writing: the ignored bits are zero, the v210 fields past
// W in the last group are zero, and so are the bytes from the end of the last group to the tight row size: a tight frame
// is fully determined.  Bytes between the tight row and a larger pitch, and between frames, are neither read nor
// written.  A working word above 1023 packs as 1023 (ColourSample<uint16_t>::read); no code is clamped to 4..1019.
//
// One unpack body and one pack body, each with two shapes, chosen on the host (csrc/formats.hip):
//
//   VEC      W % 8 == 0, every base 16-byte aligned, every pitch, offset and stride a multiple of 16 bytes.  Every
//            global access is a whole vector and consecutive lanes touch consecutive vectors:
//              v210   a workgroup owns 512 groups of one row (3072 pixels, 8 KB of wire).  A thread moves whole groups
//                     between global memory (one 16-byte access a group) and LDS, where the Y, U and V of the
//                     workgroup's pixels lie as three arrays; the arrays go to and from the planes in 16-byte (Y) and
//                     8-byte (U, V) accesses.  The pack's groups run to the end of the tight row: what lies behind
//                     column W is masked to zero.  grid = (ceil(8 ceil(W / 48) / 512), H, B)
//              y210   a thread owns 4 pixels: 16 wire bytes, 8 bytes of Y, 4 of U, 4 of V.  grid = (ceil(W / 4 / 128), H, B)
//              p210   a thread owns 8 pixels: 16 bytes of wire luma and of Y, 16 bytes of wire chroma, 8 of U, 8 of V.
//                     grid = (ceil(W / 8 / 128), H, B)
//   per sample  otherwise.  A thread owns 24 pixels of one row - four whole v210 groups - and moves them in 16-bit
//            accesses.  grid = (ceil(units / 128), H, B), units = ceil(W / 24) (v210: 2 ceil(W / 48), the tight row).
// Both shapes give the same bytes.  All offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "colour.hip.h"

namespace fiunet {

// Where the wire frames lie, resolved by the caller.  v210 / y210: rows `pitch` BYTES apart, frames `frame_stride`
// BYTES apart (chroma_offset, chroma_pitch unused).  p210: the ColourSurface quantities, in SAMPLES (pitch = the luma
// pitch).
struct Wire10Layout {
    size_t pitch, chroma_offset, chroma_pitch, frame_stride;
};

constexpr int kWire10Unit = 24;                        // pixels per thread on the per-sample path
constexpr int kWire10Groups = 4 * kColourBlock;        // v210 groups per workgroup on the vector path
constexpr int kWire10Pixels = 6 * kWire10Groups;       // and their pixels

// v210 groups of one tight row
__host__ __device__ inline int wire10_row_groups(int W) { return 8 * ((W + 47) / 48); }

// workgroups along a row (see the head of this file)
inline int wire10_blocks(int packing, bool vec, int W)
{
    int items;
    if (vec)
        items = packing == FIUNET_PACK10_V210 ? (wire10_row_groups(W) + 3) / 4 : packing == FIUNET_PACK10_Y210 ? W / 4 : W / 8;
    else
        items = packing == FIUNET_PACK10_V210 ? wire10_row_groups(W) / 4 : (W + kWire10Unit - 1) / kWire10Unit;
    return (items + kColourBlock - 1) / kColourBlock;
}

// a 32-bit little-endian word at a 2-byte aligned address
__device__ __forceinline__ uint32_t wire10_load32(const uint16_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 16; }

__device__ __forceinline__ void wire10_store32(uint16_t* p, uint32_t w)
{
    p[0] = (uint16_t)(w & 0xFFFFu);
    p[1] = (uint16_t)(w >> 16);
}

// two 16-bit words in one register: both `>> 6` (P010-style words -> codes), both `<< 6` of codes, both clamped to 1023
__device__ __forceinline__ uint32_t wire10_down2(uint32_t w) { return (w >> 6) & 0x03FF03FFu; }
__device__ __forceinline__ uint32_t wire10_up2(uint32_t w) { return w << 6; }
__device__ __forceinline__ uint32_t wire10_clamp2(uint32_t w) { return min(w & 0xFFFFu, 1023u) | min(w >> 16, 1023u) << 16; }
__device__ __forceinline__ uint32_t wire10_lo2(uint32_t a, uint32_t b) { return (a & 0xFFFFu) | b << 16; }   // low halves
__device__ __forceinline__ uint32_t wire10_hi2(uint32_t a, uint32_t b) { return a >> 16 | (b & 0xFFFF0000u); }   // high halves

// the twelve fields of one v210 group <-> its four words
__device__ __forceinline__ void wire10_v210_split(const uint32_t* w, int* Y, int* U, int* V)
{
    U[0] = w[0] & 1023; Y[0] = (w[0] >> 10) & 1023; V[0] = (w[0] >> 20) & 1023;
    Y[1] = w[1] & 1023; U[1] = (w[1] >> 10) & 1023; Y[2] = (w[1] >> 20) & 1023;
    V[1] = w[2] & 1023; Y[3] = (w[2] >> 10) & 1023; U[2] = (w[2] >> 20) & 1023;
    Y[4] = w[3] & 1023; V[2] = (w[3] >> 10) & 1023; Y[5] = (w[3] >> 20) & 1023;
}

__device__ __forceinline__ void wire10_v210_join(const int* Y, const int* U, const int* V, uint32_t* w)
{
    w[0] = (uint32_t)U[0] | (uint32_t)Y[0] << 10 | (uint32_t)V[0] << 20;
    w[1] = (uint32_t)Y[1] | (uint32_t)U[1] << 10 | (uint32_t)Y[2] << 20;
    w[2] = (uint32_t)V[1] | (uint32_t)Y[3] << 10 | (uint32_t)U[2] << 20;
    w[3] = (uint32_t)Y[4] | (uint32_t)V[2] << 10 | (uint32_t)Y[5] << 20;
}

// The Y, U and V of one workgroup's pixels on the v210 vector path (12 KB of LDS)
struct Wire10Stage {
    uint32_t y[kWire10Pixels / 2];   // pairs of 16-bit codes
    uint16_t u[kWire10Pixels / 2], v[kWire10Pixels / 2];
};

// The unpack of one thread on the vector path (W % 8 == 0, everything 16-byte aligned).
template <int P>
__device__ __forceinline__ void wire10_unpack_vec(const uint16_t* __restrict__ in, const Wire10Layout& lay,
                                                  uint16_t* __restrict__ out, size_t out_frame_stride, int H, int W)
{
    const int y = blockIdx.y, Wc = W >> 1, tid = threadIdx.x;
    uint16_t* o = out + blockIdx.z * out_frame_stride;
    uint16_t* oy = o + (size_t)y * W;
    uint16_t* ou = o + (size_t)H * W + (size_t)y * Wc;
    uint16_t* ov = ou + (size_t)H * Wc;
    if constexpr (P == FIUNET_PACK10_V210) {
        __shared__ __attribute__((aligned(16))) Wire10Stage s;
        const int xb = blockIdx.x * kWire10Pixels;
        const int npx = max(min(kWire10Pixels, W - xb), 0), ng = (npx + 5) / 6;   // (the last group may hold 2 or 4 pixels)
        const uint4* row = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(in) + blockIdx.z * lay.frame_stride +
                                                          (size_t)y * lay.pitch) + (size_t)blockIdx.x * kWire10Groups;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int g = tid + kColourBlock * k;
            if (g < ng) {
                const uint4 q = row[g];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
                int Y[6], U[3], V[3];
                wire10_v210_split(w, Y, U, V);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    s.y[3 * g + i] = (uint32_t)Y[2 * i] | (uint32_t)Y[2 * i + 1] << 16;
                    s.u[3 * g + i] = (uint16_t)U[i];
                    s.v[3 * g + i] = (uint16_t)V[i];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // npx is a multiple of 8: whole vectors
            const int j = tid + kColourBlock * k;
            if (8 * j < npx) {
                *reinterpret_cast<uint4*>(oy + xb + 8 * j) = *reinterpret_cast<const uint4*>(&s.y[4 * j]);
                *reinterpret_cast<uint2*>(ou + xb / 2 + 4 * j) = *reinterpret_cast<const uint2*>(&s.u[4 * j]);
                *reinterpret_cast<uint2*>(ov + xb / 2 + 4 * j) = *reinterpret_cast<const uint2*>(&s.v[4 * j]);
            }
        }
    } else if constexpr (P == FIUNET_PACK10_Y210) {
        const int j = blockIdx.x * kColourBlock + tid;   // pixels 4j .. 4j+3: words Y U Y V Y U Y V
        if (4 * j >= W) return;
        const uint4 q = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(in) + blockIdx.z * lay.frame_stride +
                                                       (size_t)y * lay.pitch)[j];
        uint2 yy;
        yy.x = wire10_down2(wire10_lo2(q.x, q.y));
        yy.y = wire10_down2(wire10_lo2(q.z, q.w));
        *reinterpret_cast<uint2*>(oy + 4 * (size_t)j) = yy;
        *reinterpret_cast<uint32_t*>(ou + 2 * (size_t)j) = wire10_down2(wire10_hi2(q.x, q.z));
        *reinterpret_cast<uint32_t*>(ov + 2 * (size_t)j) = wire10_down2(wire10_hi2(q.y, q.w));
    } else {
        const int j = blockIdx.x * kColourBlock + tid;   // pixels 8j .. 8j+7
        if (8 * j >= W) return;
        const uint16_t* f = in + blockIdx.z * lay.frame_stride;
        const uint4 a = *reinterpret_cast<const uint4*>(f + (size_t)y * lay.pitch + 8 * (size_t)j);
        const uint4 c = *reinterpret_cast<const uint4*>(f + lay.chroma_offset + (size_t)y * lay.chroma_pitch + 8 * (size_t)j);
        uint4 yy;
        yy.x = wire10_down2(a.x); yy.y = wire10_down2(a.y); yy.z = wire10_down2(a.z); yy.w = wire10_down2(a.w);
        *reinterpret_cast<uint4*>(oy + 8 * (size_t)j) = yy;
        uint2 u, v;   // (a chroma word pair is U | V << 16)
        u.x = wire10_down2(wire10_lo2(c.x, c.y)); u.y = wire10_down2(wire10_lo2(c.z, c.w));
        v.x = wire10_down2(wire10_hi2(c.x, c.y)); v.y = wire10_down2(wire10_hi2(c.z, c.w));
        *reinterpret_cast<uint2*>(ou + 4 * (size_t)j) = u;
        *reinterpret_cast<uint2*>(ov + 4 * (size_t)j) = v;
    }
}

// The unpack of one thread on the per-sample path: row y, pixels 24t .. 24t+23 of frame blockIdx.z.
template <int P>
__device__ __forceinline__ void wire10_unpack_scalar(const uint16_t* __restrict__ in, const Wire10Layout& lay,
                                                     uint16_t* __restrict__ out, size_t out_frame_stride, int H, int W)
{
    const int t = blockIdx.x * kColourBlock + threadIdx.x, y = blockIdx.y;
    const size_t x0 = (size_t)kWire10Unit * t;
    if (x0 >= (size_t)W) return;
    const int Wc = (W + 1) >> 1;
    const int ny = min(kWire10Unit, W - (int)x0), nc = min(kWire10Unit / 2, Wc - (int)(x0 / 2));
    int Y[24], U[12], V[12];   // the codes of this unit (entries past ny / nc are never stored)
    if (P == FIUNET_PACK10_V210) {
        // (lay in bytes; `in` counts 16-bit words)
        const uint16_t* row = in + (blockIdx.z * lay.frame_stride + (size_t)y * lay.pitch) / 2 + 32 * (size_t)t;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint32_t w[4] = {0, 0, 0, 0};
            if (6 * g < ny) {   // (a group that holds a pixel lies whole inside the tight row)
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = wire10_load32(row + 8 * g + 2 * i);
            }
            wire10_v210_split(w, Y + 6 * g, U + 3 * g, V + 3 * g);
        }
    } else if (P == FIUNET_PACK10_Y210) {
        const uint16_t* row = in + (blockIdx.z * lay.frame_stride + (size_t)y * lay.pitch) / 2 + 2 * x0;
#pragma unroll
        for (int k = 0; k < 12; ++k) {   // (W is even: a pair is whole or absent)
            const bool have = k < nc;
            Y[2 * k] = have ? row[4 * k] >> 6 : 0;
            U[k] = have ? row[4 * k + 1] >> 6 : 0;
            Y[2 * k + 1] = have ? row[4 * k + 2] >> 6 : 0;
            V[k] = have ? row[4 * k + 3] >> 6 : 0;
        }
    } else {
        const uint16_t* f = in + blockIdx.z * lay.frame_stride;
        const uint16_t* py = f + (size_t)y * lay.pitch + x0;
        const uint16_t* pc = f + lay.chroma_offset + (size_t)y * lay.chroma_pitch + x0;   // (pair x0 / 2 at word x0)
#pragma unroll
        for (int i = 0; i < 24; ++i) Y[i] = i < ny ? py[i] >> 6 : 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            U[k] = k < nc ? pc[2 * k] >> 6 : 0;
            V[k] = k < nc ? pc[2 * k + 1] >> 6 : 0;
        }
    }
    uint16_t* o = out + blockIdx.z * out_frame_stride;
    uint16_t* oy = o + (size_t)y * W + x0;
    uint16_t* ou = o + (size_t)H * W + (size_t)y * Wc + x0 / 2;
    uint16_t* ov = ou + (size_t)H * Wc;
#pragma unroll
    for (int i = 0; i < 24; ++i)
        if (i < ny) oy[i] = (uint16_t)Y[i];
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if (k < nc) {
            ou[k] = (uint16_t)U[k];
            ov[k] = (uint16_t)V[k];
        }
}

// grid = (wire10_blocks(P, VEC, W), H, B)
template <int P, bool VEC>
__global__ __launch_bounds__(kColourBlock) void unpack_422p10_kernel(const uint16_t* __restrict__ in, Wire10Layout lay,
                                                                     uint16_t* __restrict__ out, size_t out_frame_stride,
                                                                     int H, int W)
{
    if constexpr (VEC) wire10_unpack_vec<P>(in, lay, out, out_frame_stride, H, W);
    else wire10_unpack_scalar<P>(in, lay, out, out_frame_stride, H, W);
}

// The pack of one thread on the vector path.
template <int P>
__device__ __forceinline__ void wire10_pack_vec(const uint16_t* __restrict__ in, size_t in_frame_stride,
                                                uint16_t* __restrict__ out, const Wire10Layout& lay, int H, int W)
{
    const int y = blockIdx.y, Wc = W >> 1, tid = threadIdx.x;
    const uint16_t* f = in + blockIdx.z * in_frame_stride;
    const uint16_t* py = f + (size_t)y * W;
    const uint16_t* pu = f + (size_t)H * W + (size_t)y * Wc;
    const uint16_t* pv = pu + (size_t)H * Wc;
    if constexpr (P == FIUNET_PACK10_V210) {
        __shared__ __attribute__((aligned(16))) Wire10Stage s;
        const int xb = blockIdx.x * kWire10Pixels;
        const int npx = max(min(kWire10Pixels, W - xb), 0);                                       // pixels to read
        const int ng = min(kWire10Groups, wire10_row_groups(W) - (int)blockIdx.x * kWire10Groups);   // groups to write
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // npx is a multiple of 8: whole vectors
            const int j = tid + kColourBlock * k;
            if (8 * j < npx) {
                *reinterpret_cast<uint4*>(&s.y[4 * j]) = *reinterpret_cast<const uint4*>(py + xb + 8 * j);
                *reinterpret_cast<uint2*>(&s.u[4 * j]) = *reinterpret_cast<const uint2*>(pu + xb / 2 + 4 * j);
                *reinterpret_cast<uint2*>(&s.v[4 * j]) = *reinterpret_cast<const uint2*>(pv + xb / 2 + 4 * j);
            }
        }
        __syncthreads();
        uint4* row = reinterpret_cast<uint4*>(reinterpret_cast<char*>(out) + blockIdx.z * lay.frame_stride +
                                              (size_t)y * lay.pitch) + (size_t)blockIdx.x * kWire10Groups;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int g = tid + kColourBlock * k;
            if (g < ng) {   // (what lies behind the last pixel - fields of its group, whole groups of padding - is zero)
                int Y[6], U[3], V[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const bool have = 6 * g + 2 * i < npx;   // (npx is even: a pair of pixels and its chroma pair together)
                    const uint32_t p = have ? s.y[3 * g + i] : 0u;
                    Y[2 * i] = (int)min(p & 0xFFFFu, 1023u);
                    Y[2 * i + 1] = (int)min(p >> 16, 1023u);
                    U[i] = have ? min((int)s.u[3 * g + i], 1023) : 0;
                    V[i] = have ? min((int)s.v[3 * g + i], 1023) : 0;
                }
                uint32_t w[4];
                wire10_v210_join(Y, U, V, w);
                uint4 q;
                q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
                row[g] = q;
            }
        }
    } else if constexpr (P == FIUNET_PACK10_Y210) {
        const int j = blockIdx.x * kColourBlock + tid;
        if (4 * j >= W) return;
        uint2 yy = *reinterpret_cast<const uint2*>(py + 4 * (size_t)j);
        yy.x = wire10_up2(wire10_clamp2(yy.x));
        yy.y = wire10_up2(wire10_clamp2(yy.y));
        const uint32_t u = wire10_up2(wire10_clamp2(*reinterpret_cast<const uint32_t*>(pu + 2 * (size_t)j)));
        const uint32_t v = wire10_up2(wire10_clamp2(*reinterpret_cast<const uint32_t*>(pv + 2 * (size_t)j)));
        uint4 q;   // Y0 U0 | Y1 V0 | Y2 U1 | Y3 V1
        q.x = wire10_lo2(yy.x, u); q.y = wire10_hi2(yy.x, v << 16);
        q.z = wire10_lo2(yy.y, u >> 16); q.w = wire10_hi2(yy.y, v);
        reinterpret_cast<uint4*>(reinterpret_cast<char*>(out) + blockIdx.z * lay.frame_stride + (size_t)y * lay.pitch)[j] = q;
    } else {
        const int j = blockIdx.x * kColourBlock + tid;
        if (8 * j >= W) return;
        uint4 a = *reinterpret_cast<const uint4*>(py + 8 * (size_t)j);
        a.x = wire10_up2(wire10_clamp2(a.x)); a.y = wire10_up2(wire10_clamp2(a.y));
        a.z = wire10_up2(wire10_clamp2(a.z)); a.w = wire10_up2(wire10_clamp2(a.w));
        uint2 u = *reinterpret_cast<const uint2*>(pu + 4 * (size_t)j), v = *reinterpret_cast<const uint2*>(pv + 4 * (size_t)j);
        u.x = wire10_up2(wire10_clamp2(u.x)); u.y = wire10_up2(wire10_clamp2(u.y));
        v.x = wire10_up2(wire10_clamp2(v.x)); v.y = wire10_up2(wire10_clamp2(v.y));
        uint4 c;   // U0 V0 | U1 V1 | U2 V2 | U3 V3
        c.x = wire10_lo2(u.x, v.x); c.y = wire10_hi2(u.x, v.x);
        c.z = wire10_lo2(u.y, v.y); c.w = wire10_hi2(u.y, v.y);
        uint16_t* o = out + blockIdx.z * lay.frame_stride;
        *reinterpret_cast<uint4*>(o + (size_t)y * lay.pitch + 8 * (size_t)j) = a;
        *reinterpret_cast<uint4*>(o + lay.chroma_offset + (size_t)y * lay.chroma_pitch + 8 * (size_t)j) = c;
    }
}

// The pack of one thread on the per-sample path: row y, pixels 24t .. 24t+23 of frame blockIdx.z; v210: also the zeros
// behind the last pixel, up to the tight row size.
template <int P>
__device__ __forceinline__ void wire10_pack_scalar(const uint16_t* __restrict__ in, size_t in_frame_stride,
                                                   uint16_t* __restrict__ out, const Wire10Layout& lay, int H, int W)
{
    using S = ColourSample<uint16_t>;
    const int t = blockIdx.x * kColourBlock + threadIdx.x, y = blockIdx.y;
    const size_t x0 = (size_t)kWire10Unit * t;
    // (v210: the units of the tight row, which may end up to 42 pixels behind W)
    if (P == FIUNET_PACK10_V210 ? 4 * t >= wire10_row_groups(W) : x0 >= (size_t)W) return;
    const int Wc = (W + 1) >> 1;
    const int ny = max(min(kWire10Unit, W - (int)x0), 0), nc = max(min(kWire10Unit / 2, Wc - (int)(x0 / 2)), 0);
    const uint16_t* f = in + blockIdx.z * in_frame_stride;
    const uint16_t* py = f + (size_t)y * W + x0;
    const uint16_t* pu = f + (size_t)H * W + (size_t)y * Wc + x0 / 2;
    const uint16_t* pv = pu + (size_t)H * Wc;
    int Y[24], U[12], V[12];   // the codes of this unit; 0 past the end of the row
#pragma unroll
    for (int i = 0; i < 24; ++i) Y[i] = i < ny ? S::read(py[i]) : 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        U[k] = k < nc ? S::read(pu[k]) : 0;
        V[k] = k < nc ? S::read(pv[k]) : 0;
    }
    if (P == FIUNET_PACK10_V210) {
        uint16_t* row = out + (blockIdx.z * lay.frame_stride + (size_t)y * lay.pitch) / 2 + 32 * (size_t)t;
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // (a group behind the last pixel is all zeros: the padding of the tight row)
            uint32_t w[4];
            wire10_v210_join(Y + 6 * g, U + 3 * g, V + 3 * g, w);
#pragma unroll
            for (int i = 0; i < 4; ++i) wire10_store32(row + 8 * g + 2 * i, w[i]);
        }
    } else if (P == FIUNET_PACK10_Y210) {
        uint16_t* row = out + (blockIdx.z * lay.frame_stride + (size_t)y * lay.pitch) / 2 + 2 * x0;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < nc) {
                row[4 * k] = (uint16_t)(Y[2 * k] << 6);
                row[4 * k + 1] = (uint16_t)(U[k] << 6);
                row[4 * k + 2] = (uint16_t)(Y[2 * k + 1] << 6);
                row[4 * k + 3] = (uint16_t)(V[k] << 6);
            }
    } else {
        uint16_t* o = out + blockIdx.z * lay.frame_stride;
        uint16_t* oy = o + (size_t)y * lay.pitch + x0;
        uint16_t* oc = o + lay.chroma_offset + (size_t)y * lay.chroma_pitch + x0;
#pragma unroll
        for (int i = 0; i < 24; ++i)
            if (i < ny) oy[i] = (uint16_t)(Y[i] << 6);
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < nc) {
                oc[2 * k] = (uint16_t)(U[k] << 6);
                oc[2 * k + 1] = (uint16_t)(V[k] << 6);
            }
    }
}

// the same grid
template <int P, bool VEC>
__global__ __launch_bounds__(kColourBlock) void pack_422p10_kernel(const uint16_t* __restrict__ in, size_t in_frame_stride,
                                                                   uint16_t* __restrict__ out, Wire10Layout lay, int H,
                                                                   int W)
{
    if constexpr (VEC) wire10_pack_vec<P>(in, in_frame_stride, out, lay, H, W);
    else wire10_pack_scalar<P>(in, in_frame_stride, out, lay, H, W);
}

}  // namespace fiunet
