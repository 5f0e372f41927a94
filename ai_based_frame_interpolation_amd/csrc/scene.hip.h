// scene.hip.h -- scene-cut detection and the sample-and-hold of cut intervals in the video loops, gfx950 only.
//
// The reference has no video loop, so the definition is our own.  For
// a clip of N frames and the N-1 intervals i between F[i] and F[i+1]:
//
//   sad[i]   sum over every sample of the frame as stored (all planes) of |F[i+1] - F[i]|, exact in 64 bits;
//            10-bit samples above 1023 read as 1023
//   mafd[i]  sad[i] * 100.0 / count / 2^bits in IEEE double, in that order (count = samples per frame): FFmpeg
//            scdet's 0-100 scale
//   score[i] min(mafd[i], |mafd[i] - mafd[i-1]|, |mafd[i] - mafd[i+1]|), a missing neighbour left out
//   cut      score[i] >= threshold
//
//   pair_sad_kernel<T>     : accumulates sad into sums[n-1] (zeroed by the caller), so that one sad can span the
//                            separate Y / U / V stacks of a planar layout.  grid = (blocks per pair, pairs).
//   pair_peak_kernel<T>    : repeated frames: max-accumulates the largest 64-sample segment sum of
//                            |F[i+1] - F[i]| into peaks[n-1] (zeroed by the caller); same grid
//   scene_cuts_kernel      : one thread per interval -> scores (fp64) and flags (uint8)
//   hold_cut_frames_kernel : on the interleaved result of a factor-`factor` loop, copies F[i] into its factor-1
//                            successors for every flagged interval; the flags are read on the device, so the hold
//                            needs no host round trip.  grid = (kHoldBlocks * (factor - 1), intervals).
//
// All three are HBM-bound.  The sums are integer atomics, one per workgroup, so the result is exact in any order
// (as sqdiff_kernel in metrics.hip.h).  The library is built with -ffp-contract=off, so the multiply and the two
// divisions of mafd are separate IEEE operations (v_mul_f64 and the div_scale / div_fmas / div_fixup sequence).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

constexpr int kSceneBlock = 256;
constexpr int kHoldBlocks = 16;   // workgroups per (interval, inserted frame)

template <typename T>
struct SceneSample;
template <>
struct SceneSample<uint8_t> {
    __device__ static __forceinline__ unsigned read(uint8_t v) { return v; }
    // |a - b| summed over the four bytes of a word
    __device__ static __forceinline__ unsigned sad_word(unsigned a, unsigned b)
    {
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = (int)((a >> (8 * j)) & 255u) - (int)((b >> (8 * j)) & 255u);
            s += (unsigned)abs(d);
        }
        return s;
    }
};
template <>
struct SceneSample<uint16_t> {
    __device__ static __forceinline__ unsigned read(uint16_t v) { return min((unsigned)v, 1023u); }
    // the two 16-bit samples of a word, each read as at most 1023
    __device__ static __forceinline__ unsigned sad_word(unsigned a, unsigned b)
    {
        const int d0 = (int)min(a & 0xffffu, 1023u) - (int)min(b & 0xffffu, 1023u);
        const int d1 = (int)min(a >> 16, 1023u) - (int)min(b >> 16, 1023u);
        return (unsigned)abs(d0) + (unsigned)abs(d1);
    }
};

// Pair i = blockIdx.y: frames i and i+1 of a contiguous stack of frames `n` samples apart.
template <typename T>
__global__ __launch_bounds__(kSceneBlock) void pair_sad_kernel(const T* __restrict__ frames, size_t n,
                                                               unsigned long long* __restrict__ sums)
{
    using S = SceneSample<T>;
    const size_t pair = blockIdx.y;
    const T* pa = frames + pair * n;
    const T* pb = pa + n;
    unsigned long long s = 0;
    // 16 bytes per lane per step where both frame bases allow it, single samples otherwise and at the tail
    constexpr size_t kPerVec = 16 / sizeof(T);
    const bool vec = (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
    const size_t nv = vec ? n / kPerVec : 0;
    const size_t step = (size_t)gridDim.x * kSceneBlock;
    for (size_t i = (size_t)blockIdx.x * kSceneBlock + threadIdx.x; i < nv; i += step) {
        const uint4 va = reinterpret_cast<const uint4*>(pa)[i], vb = reinterpret_cast<const uint4*>(pb)[i];
        s += S::sad_word(va.x, vb.x) + S::sad_word(va.y, vb.y) + S::sad_word(va.z, vb.z) + S::sad_word(va.w, vb.w);
    }
    for (size_t i = nv * kPerVec + (size_t)blockIdx.x * kSceneBlock + threadIdx.x; i < n; i += step) {
        const int d = (int)S::read(pa[i]) - (int)S::read(pb[i]);
        s += (unsigned)abs(d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __shared__ unsigned long long part[kSceneBlock / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kSceneBlock / 64; ++w) t += part[w];
        if (t) atomicAdd(sums + pair, t);
    }
}

// Repeated frames.  Pair i = blockIdx.y as above; peak[i] = the largest sum of |F[i+1] - F[i]| over the
// aligned 64-sample segments of the frame, counted from its first sample (the last one may be short).  Max-accumulates
// into peaks[pair] (zeroed by the caller): the maximum is order-independent, so one integer atomicMax per workgroup is
// exact, and several stacks of the same frames share one result.  A segment sum is at most 64 * 1023 < 2^16.
//   vector path   both frame bases 16-byte aligned: the n / 64 whole segments, 16 bytes per lane, kSegLanes = 4 (8-bit)
//                 or 8 (10-bit) adjacent lanes per segment, summed inside the lane group (segment_sum); the loop runs
//                 on a wave-uniform base with the load predicated, so every lane is active in every exchange
//   sample path   a wave per segment, a lane per sample, summed over the wave: the short last segment after the vector
//                 path, every segment where a base is unaligned (an odd n misaligns every second pair)
// The sum of s over the aligned group of kLanes (4 or 8) adjacent lanes, in every lane of the group, with every lane of
// the wave active: DPP moves on the VALU (lanes 1 and 2 apart inside a quad, then the other quad of the 8 by the mirror of
// the half row, whose lanes all hold their quad's sum by then), where __shfl_xor would go through the LDS crossbar once
// per 16 bytes loaded.
template <int kLanes>
__device__ __forceinline__ unsigned segment_sum(unsigned s)
{
    static_assert(kLanes == 4 || kLanes == 8, "a segment is 4 or 8 lanes");
    s += (unsigned)__builtin_amdgcn_update_dpp(0, (int)s, 0xB1, 0xF, 0xF, true);        // quad_perm [1, 0, 3, 2]
    s += (unsigned)__builtin_amdgcn_update_dpp(0, (int)s, 0x4E, 0xF, 0xF, true);        // quad_perm [2, 3, 0, 1]
    if (kLanes == 8) s += (unsigned)__builtin_amdgcn_update_dpp(0, (int)s, 0x141, 0xF, 0xF, true);   // row_half_mirror
    return s;
}

template <typename T>
__global__ __launch_bounds__(kSceneBlock) void pair_peak_kernel(const T* __restrict__ frames, size_t n,
                                                                unsigned* __restrict__ peaks)
{
    using S = SceneSample<T>;
    const size_t pair = blockIdx.y;
    const T* pa = frames + pair * n;
    const T* pb = pa + n;
    constexpr size_t kPerVec = 16 / sizeof(T);
    constexpr int kSegLanes = (int)(64 / kPerVec);
    const bool vec = (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
    const size_t vseg = vec ? n / 64 : 0;      // whole segments of the vector path
    const size_t nseg = (n + 63) / 64;
    const unsigned lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * (kSceneBlock / 64) + (threadIdx.x >> 6);
    const size_t waves = (size_t)gridDim.x * (kSceneBlock / 64);
    unsigned m = 0;
    const size_t nv = vseg * kSegLanes;        // vectors of the vector path: a multiple of kSegLanes
    for (size_t base = wave * 64; base < nv; base += waves * 64) {
        const size_t i = base + lane;
        unsigned s = 0;
        if (i < nv) {
            const uint4 va = reinterpret_cast<const uint4*>(pa)[i], vb = reinterpret_cast<const uint4*>(pb)[i];
            s = S::sad_word(va.x, vb.x) + S::sad_word(va.y, vb.y) + S::sad_word(va.z, vb.z) + S::sad_word(va.w, vb.w);
        }
        m = max(m, segment_sum<kSegLanes>(s));
    }
    for (size_t seg = vseg + wave; seg < nseg; seg += waves) {
        const size_t k = seg * 64 + lane;
        unsigned s = 0;
        if (k < n) {
            const int d = (int)S::read(pa[k]) - (int)S::read(pb[k]);
            s = (unsigned)abs(d);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        m = max(m, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor(m, o));
    __shared__ unsigned part[kSceneBlock / 64];
    if (lane == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < kSceneBlock / 64; ++w) t = max(t, part[w]);
        if (t) atomicMax(peaks + pair, t);
    }
}

__device__ __forceinline__ double scene_mafd(long long sad, double count, double scale)
{
    return (double)sad * 100.0 / count / scale;
}

// intervals = n_frames - 1; scale = 2^bits
__global__ void scene_cuts_kernel(const long long* __restrict__ sums, int intervals, double count, double scale,
                                  double threshold, double* __restrict__ scores, uint8_t* __restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= intervals) return;
    const double m = scene_mafd(sums[i], count, scale);
    double s = m;
    if (i > 0) s = fmin(s, fabs(m - scene_mafd(sums[i - 1], count, scale)));
    if (i + 1 < intervals) s = fmin(s, fabs(m - scene_mafd(sums[i + 1], count, scale)));
    scores[i] = s;
    flags[i] = s >= threshold ? 1 : 0;
}

// Interval i = blockIdx.y, inserted frame k = blockIdx.x / kHoldBlocks + 1 of that interval: frame i*factor + k of the
// result becomes a copy of frame i*factor (both `frame_bytes` long).
__global__ __launch_bounds__(kSceneBlock) void hold_cut_frames_kernel(uint8_t* __restrict__ video, size_t frame_bytes,
                                                                      int factor, const uint8_t* __restrict__ flags)
{
    const size_t interval = blockIdx.y;
    if (!flags[interval]) return;
    const int k = blockIdx.x / kHoldBlocks + 1, part = blockIdx.x % kHoldBlocks;
    const uint8_t* src = video + interval * (size_t)factor * frame_bytes;
    uint8_t* dst = const_cast<uint8_t*>(src) + (size_t)k * frame_bytes;
    const size_t step = (size_t)kHoldBlocks * kSceneBlock;
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const size_t nv = vec ? frame_bytes / 16 : 0;
    for (size_t i = (size_t)part * kSceneBlock + threadIdx.x; i < nv; i += step)
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    for (size_t i = nv * 16 + (size_t)part * kSceneBlock + threadIdx.x; i < frame_bytes; i += step) dst[i] = src[i];
}

}  // namespace fiunet
