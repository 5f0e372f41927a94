// deinterlace.hip.h -- motion-adaptive deinterlacing: the fields of interlaced frames to whole frames, gfx950 only.
//
// The definition is our own, in integers, in the spirit of yadif and NOT pinned against ffmpeg (DESIGN.md 3.3w;
// tests/deinterlace_ref.py restates it in numpy, and the kernels equal that restatement bit for bit).  Field i (0: the
// first in time) of frame t keeps the rows of parity p = (order == bff) ^ i, which are copied; a sample (y, x) of a row
// of the other parity is, with cur = F[t], prev = F[t-1], next = F[t+1] (clamped to the window), (prev2, next2) =
// (prev, cur) for i == 0 and (cur, next) for i == 1, ym = y - 1 (y + 1 at y == 0), yp = y + 1 (y - 1 at y == H - 1):
//
//   c = cur[ym][x], e = cur[yp][x], pred = (c + e) >> 1                                        "bob" stops here
//   d = (prev2[y][x] + next2[y][x]) >> 1, t0 = |prev2[y][x] - next2[y][x]|
//   t1 = (|prev[ym][x] - c| + |prev[yp][x] - e|) >> 1, t2 the same with next, diff = max(t0 >> 1, t1, t2)
//   3 <= x < W - 3: S(j) = sum_{k=-1..1} |cur[ym][x+k+j] - cur[yp][x+k-j]|, score = S(0) - 1; j = -1 is taken if
//                   S(-1) < score (score = S(-1), pred = (cur[ym][x-1] + cur[yp][x+1]) >> 1) and only then j = -2 is
//                   tried the same way; then j = +1 and, on success, j = +2 against the score as it stands
//   spatial check, 2 <= y < H - 2: b = (prev2[y-2][x] + next2[y-2][x]) >> 1, f the same at y + 2,
//                   mx = max(d - e, d - c, min(b - c, f - e)), mn = min(d - e, d - c, max(b - c, f - e)),
//                   diff = max(diff, mn, -mx)
//   out = min(max(pred, d - diff), d + diff)
//
// Everything is int32 and every shift acts on a non-negative value.  A result lies between the smallest and the largest
// input sample, so 16-bit words pass through unmasked.
//
//   deinterlace_kernel<T, V, METHOD, SPATIAL>: one plane of the output frames of a call.  grid = (column strips of 64 * V
//       samples, row groups, output frames); a wave takes the rows 2r and 2r + 1 of its strip, r striding over the grid's
//       rows: the kept row is copied, the other one computed.
//       V = 16 / sizeof(T): the VECTOR path, for step-1 planes whose bases, pitches and frame strides are multiples of
//       16 bytes: lane l holds the 16-byte vector l of every row it needs (consecutive lanes on consecutive vectors) and
//       stores one; the columns behind the last whole vector are one lane's, sample by sample.
//       V = 1: the PER-SAMPLE path, for stepped or unaligned planes: lane l holds sample l.
//       The direction search needs x - 3 .. x + 3 of two rows of cur: they come from the neighbouring lanes' registers
//       (__shfl_up / __shfl_down, executed by the whole wave before any lane diverges); only the lanes at the edge of a
//       wave fetch their three halo samples from memory.
//
// Memory-bound: a computed row reads up to twelve rows of three frames, all of which the neighbouring rows and the other
// field's output frame read too (L2), and writes one.  The host (video.hip) has checked every plane, the window and the
// ranges before a launch; the kernel forms no address outside rows 0 .. H - 1 and columns 0 .. W - 1 of frames
// 0 .. n_src - 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

constexpr int kDeintBlock = 256;         // four waves: four row pairs of one strip
constexpr int kDeintMaxOut = 65535;      // output frames of a call (grid.z)
constexpr unsigned kDeintMaxRowGroups = 4096;

struct DeintPlane {
    size_t src_off, src_pitch, src_fs, dst_off, dst_pitch, dst_fs;
    int h, w, sstep, dstep;
};

__device__ __forceinline__ int deint_abs(int v) { return v < 0 ? -v : v; }

// sample k of a 16-byte vector held as four words (k a constant after unrolling)
template <typename T>
__device__ __forceinline__ int deint_get(const unsigned (&w)[4], int k)
{
    if constexpr (sizeof(T) == 1) return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
    else return (int)((w[k >> 1] >> (16 * (k & 1))) & 65535u);
}

template <typename T>
__device__ __forceinline__ void deint_put(unsigned (&w)[4], int k, int v)
{
    if constexpr (sizeof(T) == 1) w[k >> 2] |= (unsigned)v << (8 * (k & 3));
    else w[k >> 1] |= (unsigned)v << (16 * (k & 1));
}

// The missing sample from its inputs: cw[3 + j] = cur[ym][x + j], ew[3 + j] = cur[yp][x + j] (only cw[3], ew[3] are read
// unless `dir`), pc / pe / nc / ne = prev and next at ym / yp, a / b = prev2 / next2 at y, am / bm and ap / bp the same
// at y - 2 and y + 2 (read under `sp` only).
template <int METHOD, bool SPATIAL>
__device__ __forceinline__ int deint_value(const int (&cw)[7], const int (&ew)[7], int pc, int pe, int nc, int ne, int a,
                                           int b, int am, int bm, int ap, int bp, bool dir, bool sp)
{
    const int c = cw[3], e = ew[3];
    int pred = (c + e) >> 1;
    if constexpr (METHOD == 0) return pred;
    const int d = (a + b) >> 1;
    const int t0 = deint_abs(a - b);
    const int t1 = (deint_abs(pc - c) + deint_abs(pe - e)) >> 1;
    const int t2 = (deint_abs(nc - c) + deint_abs(ne - e)) >> 1;
    int diff = max(t0 >> 1, max(t1, t2));
    if (dir) {
        // S(j) = sum_k |cw[3 + k + j] - ew[3 + k - j]|
        auto S = [&](int j) {
            return deint_abs(cw[2 + j] - ew[2 - j]) + deint_abs(cw[3 + j] - ew[3 - j]) + deint_abs(cw[4 + j] - ew[4 - j]);
        };
        int score = S(0) - 1;
        const int sm1 = S(-1), sm2 = S(-2), sp1 = S(1), sp2 = S(2);
        if (sm1 < score) {
            score = sm1, pred = (cw[2] + ew[4]) >> 1;
            if (sm2 < score) score = sm2, pred = (cw[1] + ew[5]) >> 1;
        }
        if (sp1 < score) {
            score = sp1, pred = (cw[4] + ew[2]) >> 1;
            if (sp2 < score) score = sp2, pred = (cw[5] + ew[1]) >> 1;
        }
    }
    if constexpr (SPATIAL) {
        if (sp) {
            const int bb = (am + bm) >> 1, ff = (ap + bp) >> 1;
            const int mx = max(max(d - e, d - c), min(bb - c, ff - e));
            const int mn = min(min(d - e, d - c), max(bb - c, ff - e));
            diff = max(diff, max(mn, -mx));
        }
    }
    return min(max(pred, d - diff), d + diff);
}

// The rows of one missing sample's inputs in one plane (pointers to sample 0 of each row; the spatial rows are those of y
// where there is no spatial check, and are not read then).
template <typename T>
struct DeintRows {
    const T *cc, *ce, *pc, *pe, *nc, *ne, *a, *b, *am, *bm, *ap, *bp;
};

// One sample, everything from memory: the tail columns of the vector path.
template <typename T, int METHOD, bool SPATIAL>
__device__ __forceinline__ int deint_sample(const DeintRows<T>& R, int x, int w, size_t st, bool sp)
{
    int cw[7] = {0, 0, 0, 0, 0, 0, 0}, ew[7] = {0, 0, 0, 0, 0, 0, 0};
    const bool dir = METHOD == 1 && x >= 3 && x < w - 3;
    cw[3] = R.cc[(size_t)x * st], ew[3] = R.ce[(size_t)x * st];
    if (dir) {
#pragma unroll
        for (int j = -3; j <= 3; ++j) cw[3 + j] = R.cc[(size_t)(x + j) * st], ew[3 + j] = R.ce[(size_t)(x + j) * st];
    }
    if constexpr (METHOD == 0) return deint_value<0, false>(cw, ew, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false, false);
    const size_t o = (size_t)x * st;
    int am = 0, bm = 0, ap = 0, bp = 0;
    if (SPATIAL && sp) am = R.am[o], bm = R.bm[o], ap = R.ap[o], bp = R.bp[o];
    return deint_value<METHOD, SPATIAL>(cw, ew, R.pc[o], R.pe[o], R.nc[o], R.ne[o], R.a[o], R.b[o], am, bm, ap, bp, dir, sp);
}

template <typename T>
__device__ __forceinline__ void deint_load(unsigned (&w)[4], const T* row, int x0)
{
    const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}

// src: the window of n_src frames; out: the first output frame of the call.  Output frame blockIdx.z is field i of window
// frame t: (first + z / 2, z & 1) at the field rate, (first + z, 0) at the frame rate.
template <typename T, int V, int METHOD, bool SPATIAL>
__global__ __launch_bounds__(kDeintBlock) void deinterlace_kernel(const T* __restrict__ src, T* __restrict__ out,
                                                                  const DeintPlane P, int n_src, int first, int bff,
                                                                  int field_rate)
{
    const int z = (int)blockIdx.z;
    const int t = first + (field_rate ? z >> 1 : z), i = field_rate ? z & 1 : 0;
    const int p = bff ^ i;   // the parity of the kept rows
    const int tp = max(t - 1, 0), tn = min(t + 1, n_src - 1);
    const T* cur = src + P.src_off + (size_t)t * P.src_fs;
    const T* prev = src + P.src_off + (size_t)tp * P.src_fs;
    const T* next = src + P.src_off + (size_t)tn * P.src_fs;
    const T* prev2 = i ? cur : prev;
    const T* next2 = i ? next : cur;
    T* dst = out + P.dst_off + (size_t)z * P.dst_fs;
    const int h = P.h, w = P.w;
    const size_t sp_ = P.src_pitch, st = (size_t)P.sstep, dt = (size_t)P.dstep;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int x0 = ((int)blockIdx.x * 64 + lane) * V;   // (w <= 2^24 and the strip covers it: no wrap)
    const bool full = x0 + V <= w;                        // this lane holds a whole vector (V == 1: a sample)
    const bool left_lane = lane > 0;                      // the lane to the left holds the V samples before x0
    const bool right_lane = lane < 63 && x0 + 2 * V <= w; // the lane to the right holds the V samples behind x0 + V
    const int pairs = (h + 1) >> 1;
    for (int r = (int)blockIdx.y * 4 + wave; r < pairs; r += (int)gridDim.y * 4) {   // wave-uniform
        const int yk = 2 * r + p, y = 2 * r + 1 - p;
        // ---- the kept row: a copy
        if (yk < h) {
            const T* s = cur + (size_t)yk * sp_;
            T* o = dst + (size_t)yk * P.dst_pitch;
            if constexpr (V > 1) {
                if (full) *reinterpret_cast<uint4*>(o + x0) = *reinterpret_cast<const uint4*>(s + x0);
                else
                    for (int x = x0; x < w; ++x) o[x] = s[x];
            } else if (full) {
                o[(size_t)x0 * dt] = s[(size_t)x0 * st];
            }
        }
        if (y >= h) continue;   // (wave-uniform: h odd, the last pair has one row)
        // ---- the missing row
        const int ym = y == 0 ? 1 : y - 1, yp = y == h - 1 ? y - 1 : y + 1;
        const bool sp = SPATIAL && y >= 2 && y + 2 < h;
        const int y0 = sp ? y - 2 : y, y1 = sp ? y + 2 : y;
        DeintRows<T> R;
        R.cc = cur + (size_t)ym * sp_, R.ce = cur + (size_t)yp * sp_;
        R.pc = prev + (size_t)ym * sp_, R.pe = prev + (size_t)yp * sp_;
        R.nc = next + (size_t)ym * sp_, R.ne = next + (size_t)yp * sp_;
        R.a = prev2 + (size_t)y * sp_, R.b = next2 + (size_t)y * sp_;
        R.am = prev2 + (size_t)y0 * sp_, R.bm = next2 + (size_t)y0 * sp_;
        R.ap = prev2 + (size_t)y1 * sp_, R.bp = next2 + (size_t)y1 * sp_;
        T* o = dst + (size_t)y * P.dst_pitch;

        if constexpr (V > 1) {
            unsigned C[4] = {0, 0, 0, 0}, E[4] = {0, 0, 0, 0};
            if (full) deint_load(C, R.cc, x0), deint_load(E, R.ce, x0);
            int lc[3] = {0, 0, 0}, le[3] = {0, 0, 0}, rc[3] = {0, 0, 0}, re[3] = {0, 0, 0};
            if constexpr (METHOD == 1) {
                // the halo from the neighbouring lanes: the whole wave is here
                unsigned LC[4], LE[4], RC[4], RE[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    LC[k] = __shfl_up(C[k], 1), LE[k] = __shfl_up(E[k], 1);
                    RC[k] = __shfl_down(C[k], 1), RE[k] = __shfl_down(E[k], 1);
                }
                if (full) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int xl = x0 - 3 + j, xr = x0 + V + j;
                        if (left_lane) lc[j] = deint_get<T>(LC, V - 3 + j), le[j] = deint_get<T>(LE, V - 3 + j);
                        else if (xl >= 0) lc[j] = R.cc[xl], le[j] = R.ce[xl];
                        if (right_lane) rc[j] = deint_get<T>(RC, j), re[j] = deint_get<T>(RE, j);
                        else if (xr < w) rc[j] = R.cc[xr], re[j] = R.ce[xr];
                    }
                }
            }
            if (full) {
                unsigned PC[4] = {}, PE[4] = {}, NC[4] = {}, NE[4] = {}, A[4] = {}, B[4] = {};
                unsigned AM[4] = {}, BM[4] = {}, AP[4] = {}, BP[4] = {};
                if constexpr (METHOD == 1) {
                    deint_load(PC, R.pc, x0), deint_load(PE, R.pe, x0), deint_load(NC, R.nc, x0), deint_load(NE, R.ne, x0);
                    deint_load(A, R.a, x0), deint_load(B, R.b, x0);
                    if (sp) deint_load(AM, R.am, x0), deint_load(BM, R.bm, x0), deint_load(AP, R.ap, x0), deint_load(BP, R.bp, x0);
                }
                unsigned O[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    int cw[7], ew[7];
#pragma unroll
                    for (int j = -3; j <= 3; ++j) {
                        const int q = k + j;   // (a constant after unrolling)
                        cw[3 + j] = q < 0 ? lc[q + 3] : q >= V ? rc[q - V] : deint_get<T>(C, q);
                        ew[3 + j] = q < 0 ? le[q + 3] : q >= V ? re[q - V] : deint_get<T>(E, q);
                    }
                    const int x = x0 + k;
                    const bool dir = METHOD == 1 && x >= 3 && x < w - 3;
                    const int v = deint_value<METHOD, SPATIAL>(cw, ew, deint_get<T>(PC, k), deint_get<T>(PE, k), deint_get<T>(NC, k),
                                                               deint_get<T>(NE, k), deint_get<T>(A, k), deint_get<T>(B, k),
                                                               deint_get<T>(AM, k), deint_get<T>(BM, k), deint_get<T>(AP, k),
                                                               deint_get<T>(BP, k), dir, sp);
                    deint_put<T>(O, k, v);
                }
                *reinterpret_cast<uint4*>(o + x0) = make_uint4(O[0], O[1], O[2], O[3]);
            } else {
                for (int x = x0; x < w; ++x) o[x] = (T)deint_sample<T, METHOD, SPATIAL>(R, x, w, 1, sp);
            }
        } else {
            // V == 1: lane l holds sample x0 of both rows of cur; x0 - 3 .. x0 + 3 from the lanes beside it
            const size_t xo = (size_t)x0 * st;
            int cw[7] = {0, 0, 0, 0, 0, 0, 0}, ew[7] = {0, 0, 0, 0, 0, 0, 0};
            if (full) cw[3] = R.cc[xo], ew[3] = R.ce[xo];
            if constexpr (METHOD == 1) {
#pragma unroll
                for (int j = 1; j <= 3; ++j) {
                    const int cl = __shfl_up(cw[3], j), el = __shfl_up(ew[3], j);
                    const int cr = __shfl_down(cw[3], j), er = __shfl_down(ew[3], j);
                    if (full) {
                        if (lane >= j) cw[3 - j] = cl, ew[3 - j] = el;
                        else if (x0 - j >= 0) cw[3 - j] = R.cc[(size_t)(x0 - j) * st], ew[3 - j] = R.ce[(size_t)(x0 - j) * st];
                        if (lane + j < 64 && x0 + j < w) cw[3 + j] = cr, ew[3 + j] = er;
                        else if (x0 + j < w) cw[3 + j] = R.cc[(size_t)(x0 + j) * st], ew[3 + j] = R.ce[(size_t)(x0 + j) * st];
                    }
                }
            }
            if (full) {
                int v;
                if constexpr (METHOD == 0) {
                    v = deint_value<0, false>(cw, ew, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false, false);
                } else {
                    int am = 0, bm = 0, ap = 0, bp = 0;
                    if (sp) am = R.am[xo], bm = R.bm[xo], ap = R.ap[xo], bp = R.bp[xo];
                    const bool dir = x0 >= 3 && x0 < w - 3;
                    v = deint_value<METHOD, SPATIAL>(cw, ew, R.pc[xo], R.pe[xo], R.nc[xo], R.ne[xo], R.a[xo], R.b[xo], am, bm, ap,
                                                     bp, dir, sp);
                }
                o[(size_t)x0 * dt] = (T)v;
            }
        }
    }
}

}  // namespace fiunet
