// ivtc.hip.h -- inverse telecine: score the three field pairings of a frame, and weave fields into frames, gfx950 only.
//
// Hard-telecined film (24 fps carried as 29.97 fps interlaced video by 2:3 pulldown) holds every film frame whole, but two
// of every five video frames are woven from the fields of two different film frames.  The definition is our own, in
// integers, in the spirit of ffmpeg's fieldmatch + decimate and NOT pinned against ffmpeg (DESIGN.md 3.3x;
// tests/ivtc_ref.py restates it in numpy, and the kernels equal that restatement bit for bit).
//
// Candidates.  Frame F[t] keeps the rows of its first field's parity k (0 for tff, 1 for bff); candidate p / c / n takes the
// other rows from S = F[t-1] / F[t] / F[t+1], clamped to the window.  The comb score of a candidate W on an h x w plane,
// h >= 3, in int32: a sample (y, x), 1 <= y <= h - 2, is COMBED iff (W[y-1][x] - W[y][x]) * (W[y+1][x] - W[y][x]) > T * T
// (10-bit words above 1023 read as 1023); the score is the largest count of combed samples over the blocks of 16 rows x 64
// columns aligned to the plane's origin (row y in block row y / 16; the last block row and column may be partial).  With
// C = F[t], a centre row of parity k has m = C[y] and u, d = S[y-1], S[y+1]; a centre row of the other parity has
// u, d = C[y-1], C[y+1] and m = S[y]: the candidates share C and differ in S alone.
//
//   field_match_kernel<T, V>: one plane of the frames of a call, all three candidates.  grid = (wave columns, row groups,
//       frames); a wave takes one block row of its columns at a time (block rows striding over the grid's rows) and walks
//       it downwards with the rows y - 1, y, y + 1 of C, F[t-1] and F[t+1] rolling in registers: a row of C is loaded
//       once, a row of the neighbours only where it has the other parity (two frames of reads per frame scored).  Every
//       lane counts its own columns; the counts of a block meet by cross-lane moves, the wave keeps the largest, and lanes
//       0..2 issue ONE vector atomicMax for the three candidates at the end.  No LDS, no barrier, no scratch.
//       V = 16 / sizeof(T): the VECTOR path, for step-1 planes whose base, pitch and frame stride are multiples of 16
//       bytes: lane l holds the 16-byte vector l of a row, 64 / V lanes make a block column (DPP sums inside the lane
//       group); the columns behind the last whole vector are one lane's, loaded sample by sample into the same registers.
//       V = 1: the PER-SAMPLE path, for stepped or unaligned planes: lane l holds column l of a block, a wave a block.
//       A register of columns outside the plane holds zeros, which are never combed (0 > T * T is false): no lane masks
//       its count, so every lane is active in every exchange.
//   field_weave_kernel<T>: output frame blockIdx.z of 1..4 planes (blockIdx.y): the rows of parity `parity` from source
//       frame keep[z], the others from frame other[z]; bytes are moved and nothing else.  The entries travel IN THE
//       KERNEL'S ARGUMENTS, kWeaveMax frames a launch, as retime_table_kernel's do.  A wave takes a row, lanes stride along
//       it by 16-byte vectors (planes flagged `vec` by the host: step 1 and everything 16-byte aligned on both sides; the
//       columns behind the last whole vector sample by sample) or by samples.
//
// Both are memory-bound.  The host (video.hip) has checked the plane, the window, every entry and the ranges before a
// launch; the kernels form no address outside rows 0 .. h - 1 and columns 0 .. w - 1 of frames 0 .. n_src - 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deinterlace.hip.h"
#include "scene.hip.h"

namespace fiunet {

constexpr int kMatchBlock = 256;          // four waves: four block rows of one wave column
constexpr int kMatchRows = 16, kMatchCols = 64;
constexpr int kMatchMaxFrames = 65535;    // frames of a call (grid.z)
constexpr unsigned kMatchMaxRowGroups = 4096;
constexpr int kMatchMaxThreshold = 1023;  // T * T and every product stay below 2^23

struct MatchPlane {
    size_t off, pitch, fs;
    int h, w, step;
};

// the samples a lane holds of one row: a 16-byte vector as four words (10-bit words already read as at most 1023), or one
// sample
template <int V>
struct MatchRow {
    unsigned w[V > 1 ? 4 : 1];
};

template <typename T>
__device__ __forceinline__ unsigned match_read(T v)
{
    if constexpr (sizeof(T) == 1) return v;
    else return min((unsigned)v, 1023u);
}

template <typename T, int V>
__device__ __forceinline__ int match_get(const MatchRow<V>& r, int k)
{
    if constexpr (V == 1) return (int)r.w[0];
    else return deint_get<T>(r.w, k);
}

// columns x0 .. x0 + V - 1 of a row (pointer to its sample 0); zeros outside the plane
template <typename T, int V>
__device__ __forceinline__ MatchRow<V> match_load(const T* row, int x0, int w, size_t st)
{
    MatchRow<V> r;
    if constexpr (V == 1) {
        r.w[0] = x0 < w ? match_read<T>(row[(size_t)x0 * st]) : 0u;
    } else {
        r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;
        if (x0 + V <= w) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
            r.w[0] = v.x, r.w[1] = v.y, r.w[2] = v.z, r.w[3] = v.w;
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) r.w[k] = min(r.w[k] & 0xffffu, 1023u) | (min(r.w[k] >> 16, 1023u) << 16);
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (x0 + k < w) deint_put<T>(r.w, k, (int)match_read<T>(row[x0 + k]));
        }
    }
    return r;
}

__device__ __forceinline__ unsigned match_combed(int u, int m, int d, int t2) { return __mul24(u - m, d - m) > t2 ? 1u : 0u; }

// a centre row of the kept parity: m = C[y] for every candidate; u, d from the rows above and below of P, C, N
template <typename T, int V>
__device__ __forceinline__ void match_count_kept(unsigned (&cnt)[3], const MatchRow<V>& m, const MatchRow<V>& pu, const MatchRow<V>& pd,
                                                 const MatchRow<V>& cu, const MatchRow<V>& cd, const MatchRow<V>& nu,
                                                 const MatchRow<V>& nd, int t2)
{
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int mm = match_get<T, V>(m, k);
        cnt[0] += match_combed(match_get<T, V>(pu, k), mm, match_get<T, V>(pd, k), t2);
        cnt[1] += match_combed(match_get<T, V>(cu, k), mm, match_get<T, V>(cd, k), t2);
        cnt[2] += match_combed(match_get<T, V>(nu, k), mm, match_get<T, V>(nd, k), t2);
    }
}

// a centre row of the other parity: u, d = C[y - 1], C[y + 1] for every candidate; m from P, C, N
template <typename T, int V>
__device__ __forceinline__ void match_count_other(unsigned (&cnt)[3], const MatchRow<V>& u, const MatchRow<V>& d, const MatchRow<V>& pm,
                                                  const MatchRow<V>& cm, const MatchRow<V>& nm, int t2)
{
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int uu = match_get<T, V>(u, k), dd = match_get<T, V>(d, k);
        cnt[0] += match_combed(uu, match_get<T, V>(pm, k), dd, t2);
        cnt[1] += match_combed(uu, match_get<T, V>(cm, k), dd, t2);
        cnt[2] += match_combed(uu, match_get<T, V>(nm, k), dd, t2);
    }
}

// the sum of a block column's counts, in every lane of it (every lane of the wave active)
template <int V>
__device__ __forceinline__ unsigned match_block_sum(unsigned s)
{
    if constexpr (V == 1) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += (unsigned)__shfl_xor((int)s, o);
        return s;
    } else {
        return segment_sum<kMatchCols / V>(s);
    }
}

// src: the window of n_src frames; frame blockIdx.z of the call is window frame first + z, and its three scores are
// MAX-ACCUMULATED into scores[3 * z + {0: p, 1: c, 2: n}].  keep: the parity of the rows F[t] keeps; t2 = T * T.
template <typename T, int V>
__global__ __launch_bounds__(kMatchBlock) void field_match_kernel(const T* __restrict__ src, const MatchPlane P, int n_src,
                                                                  int first, int keep, int t2, unsigned* __restrict__ scores)
{
    const int z = (int)blockIdx.z, t = first + z;
    const int tp = max(t - 1, 0), tn = min(t + 1, n_src - 1);
    const T* cur = src + P.off + (size_t)t * P.fs;
    const T* prev = src + P.off + (size_t)tp * P.fs;
    const T* next = src + P.off + (size_t)tn * P.fs;
    const int h = P.h, w = P.w;
    const size_t pitch = P.pitch, st = (size_t)P.step;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int x0 = ((int)blockIdx.x * 64 + lane) * V;   // (w <= 2^24 and the grid covers it: no wrap)
    const int block_rows = (h + kMatchRows - 1) / kMatchRows;
    unsigned best[3] = {0u, 0u, 0u};
    for (int br = (int)blockIdx.y * 4 + wave; br < block_rows; br += (int)gridDim.y * 4) {   // wave-uniform
        const int ya = max(br * kMatchRows, 1), yb = min(br * kMatchRows + kMatchRows, h - 1);   // centre rows ya .. yb - 1
        if (ya >= yb) continue;
        unsigned cnt[3] = {0u, 0u, 0u};
        // rows y - 1 and y of the first centre row; a neighbour's row is read only where it has the other parity
        MatchRow<V> c0 = match_load<T, V>(cur + (size_t)(ya - 1) * pitch, x0, w, st), p0 = c0, n0 = c0;
        MatchRow<V> c1 = match_load<T, V>(cur + (size_t)ya * pitch, x0, w, st), p1 = c1, n1 = c1;
        if (((ya - 1) & 1) != keep) {
            p0 = match_load<T, V>(prev + (size_t)(ya - 1) * pitch, x0, w, st);
            n0 = match_load<T, V>(next + (size_t)(ya - 1) * pitch, x0, w, st);
        } else {
            p1 = match_load<T, V>(prev + (size_t)ya * pitch, x0, w, st);
            n1 = match_load<T, V>(next + (size_t)ya * pitch, x0, w, st);
        }
        for (int y = ya; y < yb; ++y) {
            const MatchRow<V> c2 = match_load<T, V>(cur + (size_t)(y + 1) * pitch, x0, w, st);
            MatchRow<V> p2 = c2, n2 = c2;
            if ((y & 1) == keep) {   // (wave-uniform) the rows above and below have the other parity
                p2 = match_load<T, V>(prev + (size_t)(y + 1) * pitch, x0, w, st);
                n2 = match_load<T, V>(next + (size_t)(y + 1) * pitch, x0, w, st);
                match_count_kept<T, V>(cnt, c1, p0, p2, c0, c2, n0, n2, t2);
            } else {
                match_count_other<T, V>(cnt, c0, c2, p1, c1, n1, t2);
            }
            c0 = c1, c1 = c2, p0 = p1, p1 = p2, n0 = n1, n1 = n2;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) best[c] = max(best[c], match_block_sum<V>(cnt[c]));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best[c] = max(best[c], (unsigned)__shfl_xor((int)best[c], o));
    }
    const unsigned mine = lane == 0 ? best[0] : lane == 1 ? best[1] : best[2];
    if (lane < 3 && mine) atomicMax(scores + (size_t)z * 3 + lane, mine);
}

// ---- weave ---------------------------------------------------------------------------------------------------------------
constexpr int kWeaveBlock = 256;
constexpr int kWeaveMax = 64;             // output frames of a launch: their entries are kernel arguments
constexpr int kWeaveMaxOut = 65535;
constexpr int kWeaveMaxPlanes = 4;
constexpr unsigned kWeaveMaxRowGroups = 1024;

struct WeavePlane {
    size_t src_off, src_pitch, src_fs, dst_off, dst_pitch, dst_fs;
    int h, w, sstep, dstep, vec;
};
struct WeaveArgs {
    WeavePlane p[kWeaveMaxPlanes];
    uint32_t keep[kWeaveMax], other[kWeaveMax];
};

// out: the first output frame of the launch.  grid = (row groups, planes, output frames <= kWeaveMax).
template <typename T>
__global__ __launch_bounds__(kWeaveBlock) void field_weave_kernel(const T* __restrict__ src, T* __restrict__ out,
                                                                  const WeaveArgs A, int parity)
{
    constexpr int V = 16 / (int)sizeof(T);
    const WeavePlane& P = A.p[blockIdx.y];
    const int z = (int)blockIdx.z;
    const T* from[2] = {src + P.src_off + (size_t)A.other[z] * P.src_fs, src + P.src_off + (size_t)A.keep[z] * P.src_fs};
    T* dst = out + P.dst_off + (size_t)z * P.dst_fs;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int h = P.h, w = P.w;
    for (int y = (int)blockIdx.x * 4 + wave; y < h; y += (int)gridDim.x * 4) {   // wave-uniform
        const T* s = ((y & 1) == parity ? from[1] : from[0]) + (size_t)y * P.src_pitch;
        T* o = dst + (size_t)y * P.dst_pitch;
        if (P.vec) {
            int x = lane * V;
            for (; x + V <= w; x += 64 * V) *reinterpret_cast<uint4*>(o + x) = *reinterpret_cast<const uint4*>(s + x);
            if (x < w && x + V > w)   // the lane behind the last whole vector
                for (; x < w; ++x) o[x] = s[x];
        } else {
            const size_t st = (size_t)P.sstep, dt = (size_t)P.dstep;
            for (int x = lane; x < w; x += 64) o[(size_t)x * dt] = s[(size_t)x * st];
        }
    }
}

}  // namespace fiunet
