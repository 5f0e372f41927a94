// Packed (interleaved) RGB frames <-> the planar RGB uint8 [B, 3, H, W] the network's uint8 entry points take
// (DESIGN.md 3.3j).  What `ffmpeg -f rawvideo -pix_fmt rgb24 | bgr24 | rgba | bgra` pipes, what a screen grab, a render
// or cv2.imread (BGR, rows a line size apart) leaves in memory: a pixel is BPP = 3 or 4 consecutive bytes, R G B [A] or,
// with SWAP, B G R [A]; rows are `row_pitch` bytes apart, frames `frame_stride` bytes apart (PackedLayout, resolved by
// the caller: no zeros).  There is no arithmetic here but one: the alpha byte a 4-byte format is written with.
//   no alpha source     255
//   one packed source   its alpha byte (byte 3 of the same pixel)
//   two packed sources  (a1 + a2 + 1) >> 1, the rounded average the video loops give every sample they do not infer
// Both sources are frames of the format being written, in a layout of their own.
//
// Thread shape as in colour.hip.h: a thread covers 4 pixels of a row, grid = (ceil(ceil(W/4) / 128), H, B), so a wave
// moves 256 contiguous pixels of a row: 768 or 1024 contiguous bytes on the packed side, 256 on each plane.  With VEC -
// W % 4 == 0 and every pitch, stride and base a multiple of 4 bytes (the host decides: packed_vec in formats.hip) - the
// thread's 12 packed bytes are three dword accesses and its 16 packed bytes one 16-byte access, each plane quad one
// uchar4; the bytes change place in registers.  The 16-byte access is declared dword-aligned (PackedQuad below), which is
// all a global access wider than a dword needs on this hardware, so a pitch of W*4 + 4 keeps it.  Without VEC every
// access is one byte and the last thread of a row stops at W.  Bytes between W*BPP and row_pitch, and between frames,
// are never read and never written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "colour.hip.h"   // kColourBlock

namespace fiunet {

// every field in bytes, resolved by the caller
struct PackedLayout {
    size_t row_pitch, frame_stride;
};

// 16 packed bytes = 4 pixels of a 4-byte format, as one access that asks for dword alignment only
typedef uint32_t PackedQuad __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint32_t packed_byte(uint32_t w, int i) { return (w >> (8 * i)) & 0xFFu; }

// The 4 pixels a VEC thread owns, px[c][k] = byte k of pixel c, from / to their dwords (little endian).
template <int BPP>
__device__ __forceinline__ void packed_load4(const uint8_t* __restrict__ p, uint32_t px[4][4])
{
    if (BPP == 4) {
        const PackedQuad q = *reinterpret_cast<const PackedQuad*>(p);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) px[c][k] = packed_byte(w[c], k);
    } else {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(p);
        const uint32_t w[3] = {d[0], d[1], d[2]};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int i = 3 * c + k;   // byte i of the 12
                px[c][k] = packed_byte(w[i >> 2], i & 3);
            }
    }
}

template <int BPP>
__device__ __forceinline__ void packed_store4(uint8_t* __restrict__ p, const uint32_t px[4][4])
{
    if (BPP == 4) {
        PackedQuad q;
        q.x = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[0][3] << 24;
        q.y = px[1][0] | px[1][1] << 8 | px[1][2] << 16 | px[1][3] << 24;
        q.z = px[2][0] | px[2][1] << 8 | px[2][2] << 16 | px[2][3] << 24;
        q.w = px[3][0] | px[3][1] << 8 | px[3][2] << 16 | px[3][3] << 24;
        *reinterpret_cast<PackedQuad*>(p) = q;
    } else {
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int i = 3 * c + k;
                w[i >> 2] |= px[c][k] << (8 * (i & 3));
            }
        uint32_t* d = reinterpret_cast<uint32_t*>(p);
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
    }
}

// packed frames `in` in layout `li` -> planar RGB `out` [B, 3, H, W]; alpha (BPP 4, not NULL): also the alpha plane
// [B, H, W].  grid = (ceil(ceil(W/4) / 128), H, B)
template <int BPP, bool SWAP, bool VEC>
__global__ __launch_bounds__(kColourBlock) void packed_to_rgb_kernel(const uint8_t* __restrict__ in, PackedLayout li,
                                                                     uint8_t* __restrict__ out,
                                                                     uint8_t* __restrict__ alpha, int H, int W)
{
    const int t = blockIdx.x * kColourBlock + threadIdx.x, x0 = 4 * t, y = blockIdx.y;
    if (x0 >= W) return;
    const size_t plane = (size_t)H * W, at = (size_t)y * W + x0;
    const uint8_t* p = in + (size_t)blockIdx.z * li.frame_stride + (size_t)y * li.row_pitch + (size_t)x0 * BPP;
    uint8_t* o = out + (size_t)blockIdx.z * 3 * plane + at;
    uint8_t* oa = (BPP == 4 && alpha) ? alpha + (size_t)blockIdx.z * plane + at : nullptr;
    if (VEC) {
        uint32_t px[4][4];
        packed_load4<BPP>(p, px);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int k = SWAP ? 2 - ch : ch;
            *reinterpret_cast<uchar4*>(o + ch * plane) =
                make_uchar4((uint8_t)px[0][k], (uint8_t)px[1][k], (uint8_t)px[2][k], (uint8_t)px[3][k]);
        }
        if (BPP == 4 && oa)
            *reinterpret_cast<uchar4*>(oa) =
                make_uchar4((uint8_t)px[0][3], (uint8_t)px[1][3], (uint8_t)px[2][3], (uint8_t)px[3][3]);
    } else {
        const int n = min(4, W - x0);
        for (int c = 0; c < n; ++c) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch * plane + c] = p[c * BPP + (SWAP ? 2 - ch : ch)];
            if (BPP == 4 && oa) oa[c] = p[c * BPP + 3];
        }
    }
}

// planar RGB `in` [B, 3, H, W] -> packed frames `out` in layout `lo`.  BPP 4: a1, a2 (NULL, or packed frames of the same
// format in layout `la`) give the alpha byte by the rule at the head of this file.  The same grid.
template <int BPP, bool SWAP, bool VEC>
__global__ __launch_bounds__(kColourBlock) void rgb_to_packed_kernel(const uint8_t* __restrict__ in,
                                                                     uint8_t* __restrict__ out, PackedLayout lo,
                                                                     const uint8_t* a1, const uint8_t* a2,
                                                                     PackedLayout la,
                                                                     int H, int W)
{
    const int t = blockIdx.x * kColourBlock + threadIdx.x, x0 = 4 * t, y = blockIdx.y;
    if (x0 >= W) return;
    const size_t plane = (size_t)H * W;
    const uint8_t* s = in + (size_t)blockIdx.z * 3 * plane + (size_t)y * W + x0;
    uint8_t* p = out + (size_t)blockIdx.z * lo.frame_stride + (size_t)y * lo.row_pitch + (size_t)x0 * BPP;
    const size_t aoff = (size_t)blockIdx.z * la.frame_stride + (size_t)y * la.row_pitch + (size_t)x0 * BPP;
    if (VEC) {
        uint32_t px[4][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int k = SWAP ? 2 - ch : ch;
            const uchar4 v = *reinterpret_cast<const uchar4*>(s + ch * plane);
            px[0][k] = v.x; px[1][k] = v.y; px[2][k] = v.z; px[3][k] = v.w;
        }
        if (BPP == 4) {
            uint32_t pa[4][4] = {}, pb[4][4] = {};
            if (a1) packed_load4<4>(a1 + aoff, pa);
            if (a1 && a2) packed_load4<4>(a2 + aoff, pb);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                px[c][3] = !a1 ? 255u : !a2 ? pa[c][3] : (pa[c][3] + pb[c][3] + 1u) >> 1;
        }
        packed_store4<BPP>(p, px);
    } else {
        const int n = min(4, W - x0);
        for (int c = 0; c < n; ++c) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) p[c * BPP + (SWAP ? 2 - ch : ch)] = s[ch * plane + c];
            if (BPP == 4) {
                const uint32_t u = a1 ? a1[aoff + c * 4 + 3] : 255u;
                p[c * 4 + 3] = (uint8_t)(a2 && a1 ? (u + a2[aoff + c * 4 + 3] + 1u) >> 1 : u);
            }
        }
    }
}

}  // namespace fiunet
