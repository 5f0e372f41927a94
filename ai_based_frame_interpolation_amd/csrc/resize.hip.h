// resize.hip.h -- bilinear and area resize of frame planes on the device, gfx950 only.
//
// A plane is (offset, h, w, row pitch, sample step, frame stride) in samples of a buffer of frames; the kernel resamples
// every frame of up to four source planes into the destination planes of the same index, each on its own grid.  The
// definition is tests/resize_ref.py, restated here:
//
//   axis     destination index d of n_dst over n_src: f = float(fp64((d + 0.5) * (n_src / n_dst)) - 0.5), the product and
//            the subtraction each rounded to fp64 (the library is compiled with -ffp-contract=off, and resize_tap says it
//            again), the scale n_src / n_dst one IEEE fp64 division made on the host; i0 = floor(f), frac = f - i0 in
//            fp32; i0 < 0: (0, frac 0); i0 >= n_src - 1: (n_src - 1, frac 0); i1 = min(i0 + 1, n_src - 1);
//            c1 = rint(frac * 2048), c0 = rint((1.f - frac) * 2048), half to even
//   8 bits   S = a0 * p[x0] + a1 * p[x1] per source row;
//            out = min((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, 255): imageio_lite.resize_linear_u8,
//            the project's statement of cv2.resize(INTER_LINEAR) on uchar, to the last bit
//   10 bits  samples above 1023 read as 1023; the same S; out = min((b0 * S0 + b1 * S1 + 2^21) >> 22, 1023)
//   equal    a destination plane of the source's h and w is a copy, sample for sample (10-bit words above 1023 included)
//
// Ranges.  c0 + c1 is 2048 except where 1.f - frac rounds across a tie of the other coefficient, where it is 2047 or 2049;
// so S <= 2049 * 1023 < 2^21 + 2^11 and, at 8 bits, b * (S >> 4) <= 2049 * ((2049 * 255) >> 4) < 2^27: int.  At 10 bits
// b0 * S0 + b1 * S1 + 2^21 <= 2049 * 2049 * 1023 + 2^21 = 4294964223 + 2097152 > 2^32, so that sum is taken in 64 bits
// (two v_mad_u64_u32); with c0 + c1 == 2048 on both axes it would be at most 1023 * 2^22 + 2^21 = 4292870144 < 2^32.
//
//   resize_planes_kernel<T> : grid = (workgroups, planes).  A thread makes kVec (16 bytes of) neighbouring destination
//            samples of one row: two y taps once, two x taps per sample, four loads per sample straight from global
//            memory (a down-scale's loads are scattered, an up-scale's hit L1 / L2; no LDS).  Where the destination step
//            is 1 the chunks of a row start at its first 16-byte boundary: chunk 0 is the scalar head, the last the
//            scalar tail, every whole chunk between them one 16-byte store.  A stepped destination takes scalar stores.
//            All addressing is in 64 bits (size_t offsets from the two base pointers); only the item count of one
//            launch is 32-bit, which the host guarantees by launching frames in batches.
//
// HBM / L2-bound.  Nothing is staged, no table is built: the taps are recomputed per sample (two fp64 operations and a
// handful of fp32 ones), which is less than the four scattered loads cost.
//
// The area filter (FIUNET_RESIZE_AREA; the definition is tests/resize_area_ref.py), down-scaling only, in
// integers:
//
//   axis     in units of 1 / n_dst of a source sample, destination d covers [d * n_src, (d + 1) * n_src) and source j
//            covers [j * n_dst, (j + 1) * n_dst); w(d, j) is the length of their overlap.  It is non-zero for cnt
//            neighbouring j from j0 = floor(d * n_src / n_dst): n_dst - (d * n_src - j0 * n_dst) for the first, n_dst for
//            every one between, the rest of n_src for the last; the weights of one d sum to n_src
//   plane    N = sum_y wy(r, y) * sum_x wx(c, x) * v(y, x), D = sw * sh, out = (N + D / 2) / D: exact, half up, never above
//            the largest sample; at 10 bits samples above 1023 read as 1023
//
// Ranges.  n <= 2^24, so d * n_src < 2^48 (exact in fp64: resize_area_div); a row sum is at most sw * 1023 < 2^34 and
// N + D / 2 < 2^59: 64 bits.  D is one constant per plane: the quotient (<= 1023) is estimated in fp64 (relative error of
// the product below 2^-51, so the floor is off by at most one) and put right by two 64-bit multiply-compares.
//
//   resize_area_kernel<T> : grid = (workgroups, planes).  The store chunks are those of resize_planes_kernel, but kVec
//            neighbouring lanes share one chunk, a lane per destination sample: neighbouring lanes read neighbouring runs
//            of sw / dw source samples, so one load instruction of a wave covers a contiguous 64 * sw / dw samples of a
//            source row, and the loop over the rows of the span reads every source sample exactly once.  A whole chunk is
//            packed across its lanes (an OR over the lanes of a word, then three shifts of whole words down to the
//            chunk's first lane) and stored as 16 bytes by that lane; head, tail and stepped destinations store a sample
//            per lane.  The ratio limit (64 on either axis) bounds one lane's work at 66 x 66 samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

constexpr int kResizeBlock = 256;
constexpr int kResizeMaxPlanes = 4;
constexpr int kResizeMaxSize = 1 << 24;   // an fp32 coordinate holds every index below it exactly

struct ResizeTap {
    int i0, i1, c0, c1;
};

// (i0, i1, c0, c1) of destination index d; scale = (double)n_src / (double)n_dst from the host.  0 <= i0 <= i1 < n_src.
__device__ __forceinline__ ResizeTap resize_tap(int d, int n_src, double scale)
{
#pragma clang fp contract(off)
    const double prod = ((double)d + 0.5) * scale;   // (d + 0.5 is exact)
    const float f = (float)(prod - 0.5);
    const float fl = floorf(f);
    int i0 = (int)fl;
    float frac = f - fl;
    if (i0 < 0) i0 = 0, frac = 0.f;
    if (i0 >= n_src - 1) i0 = n_src - 1, frac = 0.f;
    const float inv = 1.f - frac;
    ResizeTap t;
    t.i0 = i0;
    t.i1 = min(i0 + 1, n_src - 1);
    t.c1 = (int)rintf(frac * 2048.f);   // (a power of two: exact)
    t.c0 = (int)rintf(inv * 2048.f);
    return t;
}

template <typename T>
struct ResizeSample;
template <>
struct ResizeSample<uint8_t> {
    static constexpr int kVec = 16;
    __device__ static __forceinline__ int read(uint8_t v) { return v; }
    __device__ static __forceinline__ unsigned blend(int s0, int s1, int b0, int b1)
    {
        return (unsigned)min((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2, 255);
    }
};
template <>
struct ResizeSample<uint16_t> {
    static constexpr int kVec = 8;
    __device__ static __forceinline__ int read(uint16_t v) { return min((int)v, 1023); }
    __device__ static __forceinline__ unsigned blend(int s0, int s1, int b0, int b1)
    {
        // up to 2049 * 2049 * 1023 + 2^21 > 2^32 (see the head of the file): 64 bits
        const unsigned long long n = (unsigned long long)(unsigned)b0 * (unsigned)s0 +
                                     (unsigned long long)(unsigned)b1 * (unsigned)s1 + (1ull << 21);
        return (unsigned)min(n >> 22, 1023ull);
    }
};

// One plane pair of a launch.  The host has checked: 1 <= sizes <= kResizeMaxSize, steps 1..4, pitches cover a row, every
// plane inside its frame stride, and items = frames * dh * chunks < 2^31.
struct ResizePlane {
    size_t src_off, src_pitch, src_fs;   // in samples; the offsets include the first frame of this launch
    size_t dst_off, dst_pitch, dst_fs;
    double sx, sy;                       // sw / dw and sh / dh
    int sh, sw, dh, dw;
    int sstep, dstep;
    unsigned chunks;                     // store chunks per destination row: ceil(dw / kVec), + 1 at dstep 1 (the head)
    unsigned items;                      // frames * dh * chunks
    double inv_dw, inv_dh, inv_chunks;   // 1 / dw, 1 / dh, 1 / chunks (resize_area_kernel divides with them)
};
struct ResizeArgs {
    ResizePlane p[kResizeMaxPlanes];
};

template <typename T>
__global__ __launch_bounds__(kResizeBlock) void resize_planes_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                                     const ResizeArgs args)
{
    using S = ResizeSample<T>;
    constexpr int V = S::kVec;
    const ResizePlane& P = args.p[blockIdx.y];
    const bool copy = P.sh == P.dh && P.sw == P.dw;
    const unsigned stride = gridDim.x * kResizeBlock;   // (items < 2^31 and stride <= 2^31: item + stride fits)
    for (unsigned item = blockIdx.x * kResizeBlock + threadIdx.x; item < P.items; item += stride) {
        const unsigned c = item % P.chunks, fr = item / P.chunks;
        const int r = (int)(fr % (unsigned)P.dh);
        const size_t frame = fr / (unsigned)P.dh;
        T* drow = dst + P.dst_off + frame * P.dst_fs + (size_t)r * P.dst_pitch;
        const T* sbase = src + P.src_off + frame * P.src_fs;
        // this thread's samples [x0, x1) of the row
        int x0, x1;
        if (P.dstep == 1) {
            const int head = min((int)(((16u - (unsigned)((uintptr_t)drow & 15u)) & 15u) / sizeof(T)), P.dw);
            x0 = c == 0 ? 0 : head + (int)(c - 1) * V;
            x1 = c == 0 ? head : min(P.dw, x0 + V);
        } else {
            x0 = (int)c * V;
            x1 = min(P.dw, x0 + V);
        }
        if (x0 >= x1) continue;
        const bool whole = P.dstep == 1 && x1 - x0 == V;   // (then drow + x0 lies on a 16-byte boundary)
        T o[V];
        if (copy) {
            const T* srow = sbase + (size_t)r * P.src_pitch;
            if (whole && P.sstep == 1 && ((uintptr_t)(srow + x0) & 15) == 0) {
                *reinterpret_cast<uint4*>(drow + x0) = *reinterpret_cast<const uint4*>(srow + x0);
                continue;
            }
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (x0 + k < x1) o[k] = srow[(size_t)(x0 + k) * P.sstep];
        } else {
            const ResizeTap ty = resize_tap(r, P.sh, P.sy);
            const T* r0 = sbase + (size_t)ty.i0 * P.src_pitch;
            const T* r1 = sbase + (size_t)ty.i1 * P.src_pitch;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (x0 + k < x1) {
                    const ResizeTap tx = resize_tap(x0 + k, P.sw, P.sx);
                    const size_t a = (size_t)tx.i0 * P.sstep, b = (size_t)tx.i1 * P.sstep;
                    const int s0 = tx.c0 * S::read(r0[a]) + tx.c1 * S::read(r0[b]);
                    const int s1 = tx.c0 * S::read(r1[a]) + tx.c1 * S::read(r1[b]);
                    o[k] = (T)S::blend(s0, s1, ty.c0, ty.c1);
                }
            }
        }
        if (whole) {
            unsigned wd[4] = {0, 0, 0, 0};
            constexpr int kPerWord = 4 / sizeof(T);
#pragma unroll
            for (int k = 0; k < V; ++k) wd[k / kPerWord] |= (unsigned)o[k] << (8 * sizeof(T) * (k % kPerWord));
            *reinterpret_cast<uint4*>(drow + x0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (x0 + k < x1) drow[(size_t)(x0 + k) * P.dstep] = o[k];
        }
    }
}

// ---- the area filter ------------------------------------------------------------------------------------------------
constexpr int kResizeAreaMaxRatio = 64;

struct ResizeSpan {
    unsigned j0, cnt, wf, wl;   // source indices j0 .. j0 + cnt - 1; weights wf, n_dst ..., wl (cnt == 1: wf alone)
};

// x / n and the remainder, without the integer division hipcc would expand to some thirty instructions (seven of them
// per sample otherwise): the quotient is estimated as fp64(x) * inv with inv = 1 / (double)n from the host.  x is exact
// in fp64 (below 2^53) and the product is off by less than 2^-51 of itself, under one for a quotient below 2^48: the
// floor is off by at most one either way, and the remainder, which then lies in (-n, 2 n), says which.  It is taken from
// the low 32 bits alone (every n here is at most 2^24, so it fits an int whatever x is).
__device__ __forceinline__ unsigned resize_area_div(double x, unsigned x_lo, unsigned n, double inv, unsigned& rem)
{
    unsigned q = (unsigned)(x * inv);
    int r = (int)(x_lo - q * n);
    if (r < 0) --q, r += (int)n;
    else if (r >= (int)n) ++q, r -= (int)n;
    rem = (unsigned)r;
    return q;
}

// The span of destination index d; 1 <= n_dst <= n_src <= 2^24, inv_dst = 1 / (double)n_dst.
__device__ __forceinline__ ResizeSpan resize_area_span(unsigned d, unsigned n_src, unsigned n_dst, double inv_dst)
{
    ResizeSpan s;
    unsigned rem;
    s.j0 = resize_area_div((double)d * (double)n_src, d * n_src, n_dst, inv_dst, rem);   // d * n_src < 2^48: exact
    s.wf = n_dst - rem;   // 1 .. n_dst (<= n_src)
    const unsigned rest = n_src - s.wf, up = rest + n_dst - 1;
    const unsigned more = resize_area_div((double)up, up, n_dst, inv_dst, rem);
    s.cnt = 1 + more;
    s.wl = more ? rest - (more - 1) * n_dst : 0;   // 1 .. n_dst
    return s;
}

// (n + D / 2) / D for a quotient of at most 1023: n = N + D / 2 < 2^59, inv_d = 1 / (double)D.
__device__ __forceinline__ unsigned resize_area_quotient(unsigned long long n, unsigned long long D, double inv_d)
{
    unsigned q = (unsigned)((double)n * inv_d);
    if ((unsigned long long)q * D > n) --q;
    else if ((unsigned long long)(q + 1) * D <= n) ++q;
    return q;
}

template <typename T>
__global__ __launch_bounds__(kResizeBlock) void resize_area_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                                   const ResizeArgs args)
{
    using S = ResizeSample<T>;
    constexpr int V = S::kVec;
    constexpr unsigned kGroups = kResizeBlock / V;   // store chunks per workgroup and pass
    constexpr int kPerWord = 4 / sizeof(T);
    const ResizePlane& P = args.p[blockIdx.y];
    const unsigned long long D = (unsigned long long)P.sw * (unsigned long long)P.sh;
    const double inv_d = 1.0 / (double)D;
    const int sub = (int)(threadIdx.x % V);
    // (the bound of the loop is the workgroup's: every lane of a wave reaches the shuffles below)
    for (unsigned base = blockIdx.x * kGroups; base < P.items; base += gridDim.x * kGroups) {
        const unsigned item = base + threadIdx.x / V;
        const bool valid = item < P.items;
        unsigned o = 0;
        bool whole = false, mine = false;
        T* dptr = dst;
        if (valid) {
            unsigned c, ur;
            const unsigned fr = resize_area_div((double)item, item, P.chunks, P.inv_chunks, c);
            const size_t frame = resize_area_div((double)fr, fr, (unsigned)P.dh, P.inv_dh, ur);
            const int r = (int)ur;
            T* drow = dst + P.dst_off + frame * P.dst_fs + (size_t)r * P.dst_pitch;
            int x0, x1;
            if (P.dstep == 1) {
                const int head = min((int)(((16u - (unsigned)((uintptr_t)drow & 15u)) & 15u) / sizeof(T)), P.dw);
                x0 = c == 0 ? 0 : head + (int)(c - 1) * V;
                x1 = c == 0 ? head : min(P.dw, x0 + V);
            } else {
                x0 = (int)c * V;
                x1 = min(P.dw, x0 + V);
            }
            whole = P.dstep == 1 && x1 - x0 == V;   // (then drow + x0 lies on a 16-byte boundary)
            const int x = x0 + sub;
            mine = x < x1;
            dptr = drow + (size_t)x * P.dstep;
            if (mine) {
                const ResizeSpan sy = resize_area_span((unsigned)r, (unsigned)P.sh, (unsigned)P.dh, P.inv_dh);
                const ResizeSpan sx = resize_area_span((unsigned)x, (unsigned)P.sw, (unsigned)P.dw, P.inv_dw);
                const T* p = src + P.src_off + frame * P.src_fs + (size_t)sy.j0 * P.src_pitch + (size_t)sx.j0 * P.sstep;
                const size_t last = (size_t)(sx.cnt - 1) * P.sstep;
                unsigned long long n = D >> 1;
                for (unsigned yy = 0; yy < sy.cnt; ++yy, p += P.src_pitch) {
                    unsigned inner = 0;   // <= 64 * 1023
                    for (unsigned k = 1; k + 1 < sx.cnt; ++k) inner += (unsigned)S::read(p[(size_t)k * P.sstep]);
                    unsigned long long row = (unsigned long long)(unsigned)P.dw * inner +
                                             (unsigned long long)sx.wf * (unsigned)S::read(p[0]);
                    if (sx.cnt > 1) row += (unsigned long long)sx.wl * (unsigned)S::read(p[last]);
                    const unsigned wy = yy == 0 ? sy.wf : yy + 1 == sy.cnt ? sy.wl : (unsigned)P.dh;
                    n += wy * row;   // row < 2^34, the weights of a span sum to sh <= 2^24
                }
                o = resize_area_quotient(n, D, inv_d);
            }
        }
        // a whole chunk: the samples of a word meet in every lane of it, the words in the chunk's first lane
        unsigned word = o << (8 * sizeof(T) * (sub % kPerWord));
#pragma unroll
        for (int m = 1; m < kPerWord; m <<= 1) word |= (unsigned)__shfl_xor((int)word, m);
        const unsigned w1 = (unsigned)__shfl_down((int)word, kPerWord);
        const unsigned w2 = (unsigned)__shfl_down((int)word, 2 * kPerWord);
        const unsigned w3 = (unsigned)__shfl_down((int)word, 3 * kPerWord);
        if (whole) {
            if (sub == 0) *reinterpret_cast<uint4*>(dptr) = make_uint4(word, w1, w2, w3);
        } else if (mine) {
            *dptr = (T)o;
        }
    }
}

}  // namespace fiunet
