// chroma.hip.h -- motion-guided chroma for the grayscale video route, gfx950 only.
//
// The definition is chroma.py's, in torch.  One inserted frame M between the stored frames A and B: the luma goes
// through the network, and the chroma of M is, 8x8 luma block by block, either the warp of A's and B's chroma to the
// middle of the interval along the luma flow A -> B (flow_warp_table_kernel's arithmetic at wn = 1, den = 2) or their
// rounded average.  The network's own luma YM decides: a block takes the warp iff the warped luma Ym is closer to YM
// than the averaged luma Ya is, in the sum of absolute differences over the 16x16 window around the block (indices
// clamped to the plane; a clamped index counts again; strict, so a tie takes the average).  No thresholds.
//
//   chroma_pick_kernel   one workgroup per tile of 16x8 blocks of one frame: Ym, Ya and the two absolute differences of
//                        every luma sample of the tile's windows (72 rows of 136 at most) are computed once, four
//                        samples of a row per thread, summed per 4-sample quad (v_sad_u8 at 8 bits) into LDS, then per 4x4 cell,
//                        then per block (16 cells) -> pick [n, ceil(h / 8), ceil(w / 8)] uint8.  A quad's and a cell's
//                        two sums travel as the halves of one dword (16 * 1023 < 2^16); a block's 256 terms fit int32.
//   chroma_fill_kernel   both chroma planes of n frames: one thread makes the samples of a row that fill a dword, as the
//                        warp kernel does; a thread none of whose samples is picked never touches the flow.
// Planes are read and written where they lie (FlowWarpPlane); the host has checked every index before the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow.hip.h"

namespace fiunet {

constexpr int CHROMA_BLOCK = 8;                                  // luma samples per block side
// blocks per tile, one workgroup: 16 x 8 puts 2448 quads on 256 threads (9.6 rounds of 10) and computes 19.5 % more
// samples than the tile holds; 8 x 8 measured 27.3 us a 1080p frame (1296 quads: 5.1 rounds of 6, 27 % more samples)
constexpr int CHROMA_TILE_X = 16, CHROMA_TILE_Y = 8;
constexpr int CHROMA_RH = CHROMA_BLOCK * CHROMA_TILE_Y + 8;      // luma rows under a tile's windows
constexpr int CHROMA_RQ = (CHROMA_BLOCK * CHROMA_TILE_X + 8) / 4;   // quads a row, cells a row

// grid = (ceil(pw / 16), ceil(ph / 8), n), block 256; flow [n, h, w, 2]
template <typename T>
__global__ __launch_bounds__(256) void chroma_pick_kernel(const T* __restrict__ a, FlowWarpPlane ap,
                                                          const T* __restrict__ b, FlowWarpPlane bp,
                                                          const T* __restrict__ m, FlowWarpPlane mp,
                                                          const float* __restrict__ flow, int h, int w, int ph, int pw,
                                                          uint8_t* __restrict__ pick)
{
    __shared__ uint32_t quad[CHROMA_RH][CHROMA_RQ];   // low half: sum of |Ym - YM| over 4 samples; high half: |Ya - YM|
    __shared__ uint32_t cell[CHROMA_RH / 4][CHROMA_RQ];
    const int f = blockIdx.z, tid = threadIdx.x;
    const T* pa = a + ap.off + (size_t)f * ap.fs;
    const T* pb = b + bp.off + (size_t)f * bp.fs;
    const T* pm = m + mp.off + (size_t)f * mp.fs;
    const float2* fl = reinterpret_cast<const float2*>(flow) + (size_t)f * h * w;
    const int nbx = min(CHROMA_TILE_X, pw - (int)blockIdx.x * CHROMA_TILE_X);   // blocks of this tile inside the map
    const int nby = min(CHROMA_TILE_Y, ph - (int)blockIdx.y * CHROMA_TILE_Y);
    const int nq = 2 * nbx + 2, rows = CHROMA_BLOCK * nby + 8;
    const int x00 = blockIdx.x * (CHROMA_BLOCK * CHROMA_TILE_X) - 4, y00 = blockIdx.y * (CHROMA_BLOCK * CHROMA_TILE_Y) - 4;
    for (int q = tid; q < rows * nq; q += 256) {
        const int r = q / nq, c = q - r * nq;
        const int y = flow_clampi(y00 + r, 0, h - 1);
        unsigned vm[4], va[4], vt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = flow_clampi(x00 + 4 * c + k, 0, w - 1);
            const float2 d = fl[(size_t)y * w + x];
            int sa, sb;
            flow_warp_pair<T>(pa, ap.pitch, ap.step, pb, bp.pitch, bp.step, h, w, x, y, d.x, d.y, 0.5f, 0.5f, sa, sb);
            vm[k] = (unsigned)(sa + sb + 1) >> 1;
            va[k] = (unsigned)(FlowSample<T>::code(pa[(size_t)y * ap.pitch + (size_t)x * ap.step]) +
                               FlowSample<T>::code(pb[(size_t)y * bp.pitch + (size_t)x * bp.step]) + 1) >> 1;
            vt[k] = (unsigned)FlowSample<T>::code(pm[(size_t)y * mp.pitch + (size_t)x * mp.step]);
        }
        unsigned dm, da;
        if constexpr (sizeof(T) == 1) {
            const unsigned wm = vm[0] | vm[1] << 8 | vm[2] << 16 | vm[3] << 24;
            const unsigned wa = va[0] | va[1] << 8 | va[2] << 16 | va[3] << 24;
            const unsigned wt = vt[0] | vt[1] << 8 | vt[2] << 16 | vt[3] << 24;
            dm = __builtin_amdgcn_sad_u8(wm, wt, 0u);
            da = __builtin_amdgcn_sad_u8(wa, wt, 0u);
        } else {
            dm = da = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dm += (unsigned)abs((int)vm[k] - (int)vt[k]);
                da += (unsigned)abs((int)va[k] - (int)vt[k]);
            }
        }
        quad[r][c] = dm | da << 16;   // each at most 4 * 1023
    }
    __syncthreads();
    for (int i = tid; i < (rows >> 2) * nq; i += 256) {
        const int cr = i / nq, cc = i - cr * nq;
        cell[cr][cc] = quad[4 * cr][cc] + quad[4 * cr + 1][cc] + quad[4 * cr + 2][cc] + quad[4 * cr + 3][cc];
    }
    __syncthreads();
    if (tid < CHROMA_TILE_X * CHROMA_TILE_Y) {
        const int by = tid / CHROMA_TILE_X, bx = tid % CHROMA_TILE_X;
        if (by < nby && bx < nbx) {
            unsigned cm = 0, ca = 0;   // 256 terms of at most 1023 each
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t v = cell[2 * by + j][2 * bx + i];
                    cm += v & 0xffffu;
                    ca += v >> 16;
                }
            pick[((size_t)f * ph + blockIdx.y * CHROMA_TILE_Y + by) * pw + blockIdx.x * CHROMA_TILE_X + bx] = cm < ca ? 1 : 0;
        }
    }
}

struct ChromaPlanes {   // the two chroma planes of A, of B and of the output
    FlowWarpPlane a[2], b[2], o[2];
};

// grid = (ceil(ceil(w / V) / 64), ceil(h / 4), 2 n), block (64, 4); h x w: a chroma plane; flow [n, fh, fw, 2] on the luma;
// pick [n, ph, pw]; (sy, sx): luma samples per chroma sample
template <typename T>
__global__ __launch_bounds__(256) void chroma_fill_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          const ChromaPlanes P, const float* __restrict__ flow, int fh,
                                                          int fw, float mulx, float muly,
                                                          const uint8_t* __restrict__ pick, int ph, int pw, int sy, int sx,
                                                          int h, int w, T* __restrict__ out)
{
    constexpr int V = FlowWarpVec<T>::V;
    const int f = blockIdx.z >> 1, p = blockIdx.z & 1;
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * V, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= w || y >= h) return;
    const FlowWarpPlane A = P.a[p], B = P.b[p], O = P.o[p];
    const T* pa = a + A.off + (size_t)f * A.fs;
    const T* pb = b + B.off + (size_t)f * B.fs;
    T* po = out + O.off + (size_t)f * O.fs + (size_t)y * O.pitch + (size_t)x0 * O.step;
    const float* fl = flow + (size_t)f * fh * fw * 2;
    const uint8_t* prow = pick + ((size_t)f * ph + ((y * sy) >> 3)) * pw;
    const bool same = fh == h && fw == w;
    int y0 = 0, y1 = 0;
    float ty = 0.f;
    if (!same) flow_axis(y, h, fh, y0, y1, ty);
    const int nv = min(V, w - x0);
    // The samples of a thread lie in one block or two.  Where none is picked the flow is never touched; where one is,
    // the warp of all of them runs without a branch between them, so that their loads are in flight together (with a
    // branch per sample the four chains ran one after the other: 18.2 us a 1080p frame against 12.5 for the same warps).
    bool pk[V], any = false;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        pk[k] = k < nv && prow[((x0 + k) * sx) >> 3] != 0;
        any |= pk[k];
    }
    unsigned v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int x = min(x0 + k, w - 1);   // (a sample past the row repeats the last one and is not stored)
        v[k] = (unsigned)(FlowSample<T>::code(pa[(size_t)y * A.pitch + (size_t)x * A.step]) +
                          FlowSample<T>::code(pb[(size_t)y * B.pitch + (size_t)x * B.step]) + 1) >> 1;
    }
    if (any) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int x = min(x0 + k, w - 1);
            float dx, dy;
            flow_fetch(fl, fh, fw, same, w, x, y, y0, y1, ty, mulx, muly, dx, dy);
            int sa, sb;
            flow_warp_pair<T>(pa, A.pitch, A.step, pb, B.pitch, B.step, h, w, x, y, dx, dy, 0.5f, 0.5f, sa, sb);
            if (pk[k]) v[k] = (unsigned)(sa + sb + 1) >> 1;
        }
    }
    if (O.step == 1 && nv == V && ((uintptr_t)po & (V * sizeof(T) - 1)) == 0) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) word |= v[k] << (8 * sizeof(T) * k);
        *reinterpret_cast<uint32_t*>(po) = word;
        return;
    }
    for (int k = 0; k < nv; ++k) po[(size_t)k * O.step] = (T)v[k];
}

}  // namespace fiunet
