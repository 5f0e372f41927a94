// shutter.hip.h -- a synthesized shutter: every output frame is a weighted mean of consecutive grid rows, gfx950 only.
//
// Conversion to a LOWER frame rate: an output frame is the clip averaged over the time its shutter is
// open.  Where the window lies and what each grid row weighs is decided on the host in exact rationals (retime.py,
// `shutter_entries`) and quantised to 20 bits, so that the weights of a frame sum to D = 2^20 exactly:
//
//   out = (sum_t w[t] * x[first_row + t] + D / 2) >> 20   per sample; 10-bit words above 1023 read as 1023
//   n_taps == 1 (the weight is D)                          a byte copy of the row, as wn == 0 in retime.hip.h
//   w[t] == 0                                              row first_row + t is not read (a hole, or a dropped row)
//
// With x <= 1023 and sum w == 2^20 the sum stays below 2^30: 32-bit arithmetic holds, and nothing is divided.
//
//   shutter_kernel<T> : output frame blockIdx.y per grid row of workgroups.  The entries travel IN THE KERNEL'S ARGUMENTS
//                       (ShutterArgs, below HIP's 4 KB): no device table, nothing uploaded, so a call captures into a
//                       graph.  A frame's row, tap count and weights are indexed by blockIdx.y and the tap loop's counter
//                       only, both wave-uniform: they are scalar loads from the argument block, and the entry is never
//                       copied into a private array.  The accumulators of a lane's 16 bytes stay in registers across
//                       the tap loop; four taps are loaded before they are summed, so that a lane has 64 bytes in flight.
//                       No LDS, no barrier, no atomics.
//
// HBM-bound: a frame of n_taps live taps reads n_taps frames and writes one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

constexpr int kShutterBlock = 256;
constexpr int kShutterMaxTaps = 48;        // per output frame
constexpr int kShutterMaxFrames = 32;      // per launch
constexpr int kShutterMaxWeights = 864;    // per launch: 18 frames of 48 taps, 32 frames of 27
constexpr uint32_t kShutterOne = 1u << 20; // D
constexpr int kShutterShift = 20;

// 128 + 64 + 64 + 3456 = 3712 bytes; with the two pointers and the size the argument block is 3736 bytes
struct ShutterArgs {
    uint32_t row[kShutterMaxFrames];    // first tap row of output frame k
    uint16_t off[kShutterMaxFrames];    // where its weights start in w
    uint16_t taps[kShutterMaxFrames];   // 1 .. kShutterMaxTaps
    uint32_t w[kShutterMaxWeights];
};
static_assert(sizeof(ShutterArgs) + 2 * sizeof(void*) + sizeof(size_t) < 4096, "the argument block must stay below 4 KB");

template <typename T>
struct ShutterSample;
template <>
struct ShutterSample<uint8_t> {
    static constexpr int kPerWord = 4;
    __device__ static __forceinline__ unsigned read(uint8_t v) { return v; }
    __device__ static __forceinline__ void add_word(unsigned* acc, unsigned v, unsigned w)
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += __umul24((v >> (8 * k)) & 255u, w);   // (w <= 2^20: the 24-bit multiply is exact)
    }
    __device__ static __forceinline__ unsigned pack_word(const unsigned* acc)
    {
        unsigned o = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) o |= ((acc[k] + (kShutterOne >> 1)) >> kShutterShift) << (8 * k);
        return o;
    }
};
template <>
struct ShutterSample<uint16_t> {
    static constexpr int kPerWord = 2;
    __device__ static __forceinline__ unsigned read(uint16_t v) { return min((unsigned)v, 1023u); }
    __device__ static __forceinline__ void add_word(unsigned* acc, unsigned v, unsigned w)
    {
        acc[0] += __umul24(min(v & 0xffffu, 1023u), w);
        acc[1] += __umul24(min(v >> 16, 1023u), w);
    }
    __device__ static __forceinline__ unsigned pack_word(const unsigned* acc)
    {
        return ((acc[0] + (kShutterOne >> 1)) >> kShutterShift) | (((acc[1] + (kShutterOne >> 1)) >> kShutterShift) << 16);
    }
};

template <typename T>
__device__ __forceinline__ void shutter_add(unsigned* acc, const uint4& v, unsigned w)
{
    using S = ShutterSample<T>;
    S::add_word(acc, v.x, w);
    S::add_word(acc + S::kPerWord, v.y, w);
    S::add_word(acc + 2 * S::kPerWord, v.z, w);
    S::add_word(acc + 3 * S::kPerWord, v.w, w);
}

// grid: [n_rows][n]; out row blockIdx.y is the frame of entry blockIdx.y.  The host has checked, for every entry, that the
// rows first_row .. first_row + n_taps - 1 lie inside the grid, 1 <= n_taps <= kShutterMaxTaps and sum w == 2^20.
template <typename T>
__global__ __launch_bounds__(kShutterBlock) void shutter_kernel(const T* __restrict__ grid, size_t n, const ShutterArgs args,
                                                                T* __restrict__ out)
{
    using S = ShutterSample<T>;
    const unsigned f = blockIdx.y;   // gridDim.y <= kShutterMaxFrames
    const unsigned taps = args.taps[f], off = args.off[f];
    const T* pa = grid + (size_t)args.row[f] * n;
    T* po = out + (size_t)f * n;
    constexpr size_t kPerVec = 16 / sizeof(T);
    const size_t step = (size_t)gridDim.x * kShutterBlock;
    const size_t first = (size_t)blockIdx.x * kShutterBlock + threadIdx.x;
    if (taps == 1) {   // the weight is D: a copy of the row
        const bool vec = (((uintptr_t)pa | (uintptr_t)po) & 15) == 0;
        const size_t nv = vec ? n / kPerVec : 0;
        for (size_t i = first; i < nv; i += step) reinterpret_cast<uint4*>(po)[i] = reinterpret_cast<const uint4*>(pa)[i];
        for (size_t i = nv * kPerVec + first; i < n; i += step) po[i] = pa[i];
        return;
    }
    // 16 bytes per lane per step where the first row, the row pitch (so every tap row) and the output allow it
    const bool vec = (((uintptr_t)pa | (uintptr_t)po | (uintptr_t)(n * sizeof(T))) & 15) == 0;
    const size_t nv = vec ? n / kPerVec : 0;
    const size_t pitch = n / kPerVec;   // a row in vectors (vec: n is a whole number of them)
    for (size_t i = first; i < nv; i += step) {
        unsigned acc[kPerVec];
#pragma unroll
        for (int k = 0; k < (int)kPerVec; ++k) acc[k] = 0;
        const uint4* p = reinterpret_cast<const uint4*>(pa) + i;   // walks down the tap rows
        unsigned t = 0;
        for (; t + 4 <= taps; t += 4, p += 4 * pitch) {
            const unsigned w0 = args.w[off + t], w1 = args.w[off + t + 1], w2 = args.w[off + t + 2], w3 = args.w[off + t + 3];
            if (w0 && w1 && w2 && w3) {   // (uniform) four loads in flight, then the sums
                const uint4 v0 = p[0], v1 = p[pitch], v2 = p[2 * pitch], v3 = p[3 * pitch];
                shutter_add<T>(acc, v0, w0);
                shutter_add<T>(acc, v1, w1);
                shutter_add<T>(acc, v2, w2);
                shutter_add<T>(acc, v3, w3);
            } else {
                if (w0) shutter_add<T>(acc, p[0], w0);
                if (w1) shutter_add<T>(acc, p[pitch], w1);
                if (w2) shutter_add<T>(acc, p[2 * pitch], w2);
                if (w3) shutter_add<T>(acc, p[3 * pitch], w3);
            }
        }
        for (; t < taps; ++t, p += pitch) {
            const unsigned w = args.w[off + t];
            if (w) shutter_add<T>(acc, *p, w);
        }
        uint4 vo;
        vo.x = S::pack_word(acc);
        vo.y = S::pack_word(acc + S::kPerWord);
        vo.z = S::pack_word(acc + 2 * S::kPerWord);
        vo.w = S::pack_word(acc + 3 * S::kPerWord);
        reinterpret_cast<uint4*>(po)[i] = vo;
    }
    for (size_t i = nv * kPerVec + first; i < n; i += step) {
        unsigned acc = 0;
        for (unsigned t = 0; t < taps; ++t) {
            const unsigned w = args.w[off + t];
            if (w) acc += __umul24(S::read(pa[(size_t)t * n + i]), w);
        }
        po[i] = (T)((acc + (kShutterOne >> 1)) >> kShutterShift);
    }
}

}  // namespace fiunet
