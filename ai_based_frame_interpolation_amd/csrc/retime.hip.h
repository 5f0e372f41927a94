// retime.hip.h -- frame-rate conversion: resample the frames of a recursive bisection to any higher rate, gfx950 only.
//
// The network gives the middle of a pair only, so a D-level bisection gives frames at the times i + m / G of a clip
// (G = 2^D, the "grid": row i*G + m).  An output rate Fo > Fi puts output frame j at input time j * p / q, with
// Fi / Fo = p / q reduced, 0 < p < q <= 2^20.  The definition is our own:
//
//   i  = (j * p) / q,  r = (j * p) % q         the input interval of frame j and its phase r / q in it
//   lo = (r * G) / q,  wn = (r * G) % q        the grid row below the frame and the weight of the row above, wn / q
//   blend    out = (A * (q - wn) + B * wn + q / 2) / q per sample in integers, A = grid[i*G + lo], B the row after it;
//            10-bit words above 1023 read as 1023; wn == 0: a byte copy of A (B is not read)
//   nearest  a byte copy of B if 2 * wn > q, else of A
//   cut      interval i flagged and r != 0: a byte copy of grid row i*G (the frame before the cut), whatever lo and wn
//
//   retime_kernel<T> : output frame j0 + blockIdx.y per grid row of workgroups; i / r / lo / wn come from (j, p, q, D)
//                      once per workgroup in 64-bit integers, so nothing is uploaded per call and the flags are read on
//                      the device.  grid = (blocks per frame, output frames).
//
// HBM-bound: a blended frame reads two frames and writes one, a copied frame reads one and writes one.
//
// The division by q.  N = A * (q - wn) + B * wn + q / 2 with A, B <= 1023 and wn < q <= 2^20 is below 1024 * q <= 2^30,
// so N fits 32 bits and N / q < 1024.  retime_div estimates e = trunc(float(N) * rq), rq = 1.0f / q, and corrects it by
// one step each way.  float(N) is N (1 + d1) with |d1| <= 2^-24; rq is (1 / q)(1 + d2) with |d2| <= 2^-22 whether the
// reciprocal is the IEEE division or v_rcp_f32 (1 ulp); the product rounds once more, |d3| <= 2^-24.  So the product is
// (N / q)(1 + d) with |d| < 2^-21, and its distance from N / q is below 1024 * 2^-21 = 2^-11 < 1.  A real number less
// than 1 away from N / q truncates to floor(N / q) - 1, floor(N / q) or floor(N / q) + 1; e * q <= 1025 * 2^20 fits 32
// bits; the two corrections (e * q > N: one down; N - e * q >= q: one up) therefore leave exactly floor(N / q).
// tests/test_gpu_retime.py compares every path with Python integers, with q = 2^20 and q = 3 among the ratios.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

constexpr int kRetimeBlock = 256;
constexpr uint32_t kRetimeMaxQ = 1u << 20;

__device__ __forceinline__ unsigned retime_div(unsigned n, unsigned q, float rq)
{
    unsigned e = (unsigned)((float)n * rq);
    if (e * q > n) --e;
    if (n - e * q >= q) ++e;
    return e;
}

template <typename T>
struct RetimeSample;
template <>
struct RetimeSample<uint8_t> {
    __device__ static __forceinline__ unsigned read(uint8_t v) { return v; }
    // the four bytes of a word, each blended
    __device__ static __forceinline__ unsigned blend_word(unsigned a, unsigned b, unsigned wa, unsigned wb, unsigned q,
                                                          float rq)
    {
        unsigned o = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned n = ((a >> (8 * k)) & 255u) * wa + ((b >> (8 * k)) & 255u) * wb + (q >> 1);
            o |= retime_div(n, q, rq) << (8 * k);
        }
        return o;
    }
};
template <>
struct RetimeSample<uint16_t> {
    __device__ static __forceinline__ unsigned read(uint16_t v) { return min((unsigned)v, 1023u); }
    // the two 16-bit samples of a word, each read as at most 1023
    __device__ static __forceinline__ unsigned blend_word(unsigned a, unsigned b, unsigned wa, unsigned wb, unsigned q,
                                                          float rq)
    {
        const unsigned n0 = min(a & 0xffffu, 1023u) * wa + min(b & 0xffffu, 1023u) * wb + (q >> 1);
        const unsigned n1 = min(a >> 16, 1023u) * wa + min(b >> 16, 1023u) * wb + (q >> 1);
        return retime_div(n0, q, rq) | (retime_div(n1, q, rq) << 16);
    }
};

// grid: [(n_intervals << depth) + 1][n] covering clip intervals first_interval .. first_interval + n_intervals; out row
// blockIdx.y is clip output frame j0 + blockIdx.y.  The host has checked that every row read lies inside the grid.
template <typename T>
__global__ __launch_bounds__(kRetimeBlock) void retime_kernel(const T* __restrict__ grid, size_t n, int depth,
                                                              unsigned long long first_interval, unsigned long long j0,
                                                              unsigned p, unsigned q, int mode,
                                                              const uint8_t* __restrict__ flags, T* __restrict__ out)
{
    using S = RetimeSample<T>;
    const unsigned long long t = (j0 + blockIdx.y) * p;
    const size_t li = (size_t)(t / q - first_interval);   // the interval, counted from the grid's first
    const unsigned r = (unsigned)(t % q);
    const unsigned rg = r << depth;                       // r < 2^20, depth <= 4
    unsigned lo = rg / q, wn = rg % q;
    if (r != 0 && flags != nullptr && flags[li]) lo = 0, wn = 0;   // cut: the frame before it
    if (mode == 1) lo += 2 * wn > q ? 1u : 0u, wn = 0;             // nearest: a tie goes to the earlier frame
    const T* pa = grid + ((li << depth) + lo) * n;
    T* po = out + (size_t)blockIdx.y * n;
    constexpr size_t kPerVec = 16 / sizeof(T);
    const size_t step = (size_t)gridDim.x * kRetimeBlock;
    const size_t first = (size_t)blockIdx.x * kRetimeBlock + threadIdx.x;
    if (wn == 0) {   // a copy of A: B is not read
        const bool vec = (((uintptr_t)pa | (uintptr_t)po) & 15) == 0;
        const size_t nv = vec ? n / kPerVec : 0;
        for (size_t i = first; i < nv; i += step) reinterpret_cast<uint4*>(po)[i] = reinterpret_cast<const uint4*>(pa)[i];
        for (size_t i = nv * kPerVec + first; i < n; i += step) po[i] = pa[i];
        return;
    }
    const T* pb = pa + n;
    const unsigned wa = q - wn, wb = wn;
    const float rq = 1.0f / (float)q;
    // 16 bytes per lane per step where the three bases allow it, single samples otherwise and at the tail
    const bool vec = (((uintptr_t)pa | (uintptr_t)pb | (uintptr_t)po) & 15) == 0;
    const size_t nv = vec ? n / kPerVec : 0;
    for (size_t i = first; i < nv; i += step) {
        const uint4 va = reinterpret_cast<const uint4*>(pa)[i], vb = reinterpret_cast<const uint4*>(pb)[i];
        uint4 vo;
        vo.x = S::blend_word(va.x, vb.x, wa, wb, q, rq);
        vo.y = S::blend_word(va.y, vb.y, wa, wb, q, rq);
        vo.z = S::blend_word(va.z, vb.z, wa, wb, q, rq);
        vo.w = S::blend_word(va.w, vb.w, wa, wb, q, rq);
        reinterpret_cast<uint4*>(po)[i] = vo;
    }
    for (size_t i = nv * kPerVec + first; i < n; i += step)
        po[i] = (T)retime_div(S::read(pa[i]) * wa + S::read(pb[i]) * wb + (q >> 1), q, rq);
}

// The table-driven form (repeated frames): where an output frame comes from is decided on the host, frame
// by frame, and arrives as one entry per frame IN THE KERNEL'S ARGUMENTS (at most kRetimeTableMax per launch): there is
// no device table, nothing is copied, and the kernel reads no index it was not handed.  Output row blockIdx.y is
//   wn == 0   a byte copy of grid row `row`
//   else      (A * (den - wn) + B * wn + den / 2) / den per sample, A = grid row `row`, B = the row after it
// The host has checked row (+ 1 when wn > 0) < n_rows, wn < den and 1 <= den <= 2^20 for every entry before the first
// launch, so retime_div's proof above holds with q = den.  Mode and cut flags are resolved into the entries on the host.
constexpr int kRetimeTableMax = 64;
struct RetimeEntry {
    uint32_t row, wn, den;
};
struct RetimeTable {
    RetimeEntry e[kRetimeTableMax];
};

template <typename T>
__global__ __launch_bounds__(kRetimeBlock) void retime_table_kernel(const T* __restrict__ grid, size_t n,
                                                                    const RetimeTable table, T* __restrict__ out)
{
    using S = RetimeSample<T>;
    const RetimeEntry e = table.e[blockIdx.y];   // gridDim.y <= kRetimeTableMax
    const unsigned wn = e.wn, q = e.den;
    const T* pa = grid + (size_t)e.row * n;
    T* po = out + (size_t)blockIdx.y * n;
    constexpr size_t kPerVec = 16 / sizeof(T);
    const size_t step = (size_t)gridDim.x * kRetimeBlock;
    const size_t first = (size_t)blockIdx.x * kRetimeBlock + threadIdx.x;
    if (wn == 0) {   // a copy of A: B is not read
        const bool vec = (((uintptr_t)pa | (uintptr_t)po) & 15) == 0;
        const size_t nv = vec ? n / kPerVec : 0;
        for (size_t i = first; i < nv; i += step) reinterpret_cast<uint4*>(po)[i] = reinterpret_cast<const uint4*>(pa)[i];
        for (size_t i = nv * kPerVec + first; i < n; i += step) po[i] = pa[i];
        return;
    }
    const T* pb = pa + n;
    const unsigned wa = q - wn, wb = wn;
    const float rq = 1.0f / (float)q;
    const bool vec = (((uintptr_t)pa | (uintptr_t)pb | (uintptr_t)po) & 15) == 0;
    const size_t nv = vec ? n / kPerVec : 0;
    for (size_t i = first; i < nv; i += step) {
        const uint4 va = reinterpret_cast<const uint4*>(pa)[i], vb = reinterpret_cast<const uint4*>(pb)[i];
        uint4 vo;
        vo.x = S::blend_word(va.x, vb.x, wa, wb, q, rq);
        vo.y = S::blend_word(va.y, vb.y, wa, wb, q, rq);
        vo.z = S::blend_word(va.z, vb.z, wa, wb, q, rq);
        vo.w = S::blend_word(va.w, vb.w, wa, wb, q, rq);
        reinterpret_cast<uint4*>(po)[i] = vo;
    }
    for (size_t i = nv * kPerVec + first; i < n; i += step)
        po[i] = (T)retime_div(S::read(pa[i]) * wa + S::read(pb[i]) * wb + (q >> 1), q, rq);
}

}  // namespace fiunet
