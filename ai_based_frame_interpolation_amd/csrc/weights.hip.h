// weights.hip.h -- the checkpoint -> kernel-layout step on the device (fiunet_load_weights_device, fiunet.hip).
//
// Input: the raw state-dict tensors of the reference (model/unet.py:11-18, :42-44, :60) in device memory, fp32,
// contiguous.  Output: bit for bit every buffer the host loop of fiunet_load_weights produces -
//   scale / shift   eval-mode BatchNorm folded: inv = 1 / sqrt(var + 1e-5), scale = gamma * inv, shift = beta - mean * scale
//   w_f32           [cin/16][slot][cout][16] of w * scale, slot = kx*3 + ky, rows in natural cout order (conv 0: the stem,
//                   [tap][cin][64] of w itself)
//   w_bf16          [cin/32][slot][cout][32], packed row R holds cout bf16_row_to_cout(R); rounded to nearest
//                   (FIUNET_OPT_RNE_WEIGHTS) or with the per-filter error feedback of f32_to_bf16_feedback
//   stem_w_split    the gray fused stem's hi/lo copy [2][64][32]
//   the ConvTranspose2d packs [tap][cin/PL][cout][PL] (no BatchNorm, natural rows)
// The arithmetic is the host's, operation for operation: the library is built with -ffp-contract=off (no product fuses
// with an add), division and square root are the correctly rounded ones (hipcc's default; never the approximate
// reciprocal square root), and the three rounding helpers below are ONE definition compiled for both sides.
//
// All layers of the network go through each kernel in one launch: the layer table travels by value as the kernel
// argument (1.6 KB) and blockIdx.y picks the layer, so a load is four launches (five for the gray network, which has the
// fused stem's copy), not five per layer.
//
// The error-feedback pack is serial along a filter (the choice at each weight depends on the carry of all before it), so
// it runs one filter per thread: at most 1024 filters x 9216 weights in a layer (2048 x 1024 for a ConvTranspose2d),
// ~4.5 k filters in the whole network, all in flight at once.  What bounds it is the longest filter's walk - 9216 dependent
// double-precision add / compare steps - not the 17 M weights' bandwidth (a whole warm load measures 2.5 ms).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

// bf16 kernels: packed weight row R (= MFMA A row within its 32-cout group) holds this cout, so
// that accumulator tiles 2g and 2g+1 give a lane 8 consecutive couts (conv3x3_mfma.hip.h epilogue)
__host__ __device__ inline int bf16_row_to_cout(int R)
{
    const int r = R & 15;
    return (R & ~31) + (r >> 2) * 8 + ((R >> 4) & 1) * 4 + (r & 3);
}

__host__ __device__ inline uint16_t f32_to_bf16_rne(float f)
{
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// bf16 rounding of a conv filter's weights with error feedback: each weight goes to one of its two
// bf16 neighbours (per-weight error < 1 ulp instead of <= 1/2), whichever keeps the filter's running sum
// of rounding errors `carry` closest to zero.  Round-to-nearest leaves every filter with a random net
// error of ~0.29 ulp * sqrt(9 Cin), i.e. a fixed gain / offset error per output channel that the
// (positive, smooth) post-ReLU inputs turn into a systematic error of the layer; with the feedback the
// summed error of a filter stays below one ulp.  Measured on the bf16 path (540x960 / 1080p): output
// rel-L2 vs fp32 1.26 -> 0.64 % (seeded checkpoint), 3.3 -> 2.4 % (bench network); PSNR difference to
// the CPU reference on the interpolating checkpoint 0.042-0.072 -> 0.025-0.048 dB.  The carry runs over
// the whole filter (all input channels, taps innermost); restarting it per input channel is worse.
__host__ __device__ inline uint16_t f32_to_bf16_feedback(float v, double& carry)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7f800000u) == 0x7f800000u) return f32_to_bf16_rne(v);  // inf / NaN
    const uint16_t toward0 = (uint16_t)(u >> 16);
    const float f0 = __builtin_bit_cast(float, (uint32_t)toward0 << 16);
    if (f0 == v) return toward0;  // representable (zeros stay zeros)
    const uint16_t away = (uint16_t)(toward0 + 1);
    const float f1 = __builtin_bit_cast(float, (uint32_t)away << 16);
    const double e0 = (double)v - f0, e1 = (double)v - f1;
    const bool pick0 = __builtin_fabs(carry + e0) <= __builtin_fabs(carry + e1);
    carry += pick0 ? e0 : e1;
    return pick0 ? toward0 : away;
}

// OIHW tap t = ky*3 + kx <-> packed slot kx*3 + ky (a transposition: the same formula both ways)
__host__ __device__ inline int tap_slot(int t) { return (t % 3) * 3 + t / 3; }

constexpr int kWpConvs = 18, kWpConvTs = 4;

struct WpConv {   // one Conv2d(3x3, no bias) + BatchNorm2d: raw tensors in, prepared buffers out
    const float *w, *gamma, *beta, *mean, *var;
    float *scale, *shift, *w_f32;
    uint16_t* w_bf16;   // (conv 0, the stem: none)
    int cin, cout;
};
struct WpConvT {  // one ConvTranspose2d(2x2, stride 2) weight [cin][cout][2][2]
    const float* w;
    float* w_f32;
    uint16_t* w_bf16;
    int cin, cout;
};
struct WpTable {
    WpConv conv[kWpConvs];
    WpConvT convt[kWpConvTs];
    uint16_t* stem_split;   // gray network only, else nullptr
    int nconvt;             // 0 (bilinear decoder) or 4
};

// grid (ceil(1024 / 256), 18)
__global__ __launch_bounds__(256) void wp_fold_bn_kernel(WpTable t)
{
    const WpConv& L = t.conv[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= L.cout) return;
    // sqrtf and the plain quotient are the correctly rounded ones (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt);
    // __fsqrt_rn is NOT: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map it to the native, 1-ulp square root
    const float inv = 1.0f / sqrtf(L.var[c] + 1e-5f);
    const float sc = L.gamma[c] * inv;
    L.scale[c] = sc;
    L.shift[c] = L.beta[c] - L.mean[c] * sc;
}

// grid (any, 18 + nconvt): one thread per packed fp32 element (coalesced writes), after wp_fold_bn_kernel
__global__ __launch_bounds__(256) void wp_pack_f32_kernel(WpTable t)
{
    const int y = blockIdx.y;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    if (y >= kWpConvs) {
        const WpConvT& L = t.convt[y - kWpConvs];
        const size_t total = (size_t)4 * L.cin * L.cout;
        for (size_t i = first; i < total; i += step) {
            size_t r = i;
            const int k = (int)(r % 16); r /= 16;
            const int co = (int)(r % L.cout); r /= L.cout;
            const int plane = (int)(r % (L.cin / 16)), tap = (int)(r / (L.cin / 16));
            const int ci = plane * 16 + k;
            L.w_f32[i] = L.w[((size_t)ci * L.cout + co) * 4 + tap];
        }
        return;
    }
    const WpConv& L = t.conv[y];
    const size_t total = (size_t)9 * L.cin * L.cout;
    if (y == 0) {   // the stem: [tap][cin][64], BatchNorm applied by the stem kernels
        for (size_t i = first; i < total; i += step) {
            size_t r = i;
            const int co = (int)(r % 64); r /= 64;
            const int ci = (int)(r % L.cin), tap = (int)(r / L.cin);
            L.w_f32[i] = L.w[((size_t)co * L.cin + ci) * 9 + tap];
        }
        return;
    }
    for (size_t i = first; i < total; i += step) {
        size_t r = i;
        const int k = (int)(r % 16); r /= 16;
        const int R = (int)(r % L.cout); r /= L.cout;
        const int slot = (int)(r % 9), plane = (int)(r / 9);
        const int ci = plane * 16 + k;
        L.w_f32[i] = L.w[((size_t)R * L.cin + ci) * 9 + tap_slot(slot)] * L.scale[R];
    }
}

// grid (any, 17 + nconvt), FIUNET_OPT_RNE_WEIGHTS: one thread per packed bf16 element, after wp_fold_bn_kernel
__global__ __launch_bounds__(256) void wp_pack_bf16_rne_kernel(WpTable t)
{
    const int y = blockIdx.y;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    if (y >= kWpConvs - 1) {
        const WpConvT& L = t.convt[y - (kWpConvs - 1)];
        const size_t total = (size_t)4 * L.cin * L.cout;
        for (size_t i = first; i < total; i += step) {
            size_t r = i;
            const int k = (int)(r % 32); r /= 32;
            const int co = (int)(r % L.cout); r /= L.cout;
            const int plane = (int)(r % (L.cin / 32)), tap = (int)(r / (L.cin / 32));
            const int ci = plane * 32 + k;
            L.w_bf16[i] = f32_to_bf16_rne(L.w[((size_t)ci * L.cout + co) * 4 + tap]);
        }
        return;
    }
    const WpConv& L = t.conv[y + 1];
    const size_t total = (size_t)9 * L.cin * L.cout;
    for (size_t i = first; i < total; i += step) {
        size_t r = i;
        const int k = (int)(r % 32); r /= 32;
        const int R = (int)(r % L.cout); r /= L.cout;
        const int slot = (int)(r % 9), plane = (int)(r / 9);
        const int ci = plane * 32 + k, co = bf16_row_to_cout(R);
        L.w_bf16[i] = f32_to_bf16_rne(L.w[((size_t)co * L.cin + ci) * 9 + tap_slot(slot)] * L.scale[co]);
    }
}

// grid (ceil(2048 / 64), 17 + nconvt), the default rounding: one FILTER per thread (its carry is serial), one wave per
// workgroup so that a layer's filters spread over the chip; after wp_fold_bn_kernel.  A wave's lanes are consecutive
// packed rows: their 2-byte stores of one step lie 64 B apart and fill whole lines over 32 input channels (L2 merges them)
__global__ __launch_bounds__(64) void wp_pack_bf16_feedback_kernel(WpTable t)
{
    const int y = blockIdx.y, f = blockIdx.x * 64 + threadIdx.x;
    double carry = 0.0;  // running sum of (exact - rounded) over this filter's bf16 weights
    if (y >= kWpConvs - 1) {   // ConvTranspose2d: one filter = one (cout, tap), walked over cin
        const WpConvT& L = t.convt[y - (kWpConvs - 1)];
        if (f >= 4 * L.cout) return;
        const int co = f >> 2, tap = f & 3;   // (lanes read consecutive floats)
        for (int ci = 0; ci < L.cin; ++ci)
            L.w_bf16[(((size_t)tap * (L.cin / 32) + ci / 32) * L.cout + co) * 32 + ci % 32] =
                f32_to_bf16_feedback(L.w[((size_t)ci * L.cout + co) * 4 + tap], carry);
        return;
    }
    const WpConv& L = t.conv[y + 1];
    if (f >= L.cout) return;
    const int R = f, co = bf16_row_to_cout(R);
    const float sc = L.scale[co];
    const float* __restrict__ w = L.w + (size_t)co * L.cin * 9;
    for (int ci = 0; ci < L.cin; ++ci) {   // input channels outermost, OIHW taps 0..8 innermost: the host's order
        uint16_t* dst = L.w_bf16 + ((size_t)(ci / 32) * 9 * L.cout + R) * 32 + ci % 32;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
            dst[(size_t)tap_slot(tp) * L.cout * 32] = f32_to_bf16_feedback(w[ci * 9 + tp] * sc, carry);
    }
}

// grid 1 x 64 threads, gray network only, after wp_fold_bn_kernel: the fused stem's copy, w * scale = hi + lo in bf16,
// [hi|lo][packed row P][k]; k = lane group*8 + dx*2 + frame with lane groups 0, 1, 2 <-> dy = 0, 2, 1, k = 24 = the
// BatchNorm shift, every other k zero (fiunet_load_weights has the layout's reasons)
__global__ __launch_bounds__(64) void wp_stem_split_kernel(WpTable t)
{
    const WpConv& L = t.conv[0];
    const int P = threadIdx.x, co = bf16_row_to_cout(P);
    const float sc = L.scale[co];
    uint16_t hi[32], lo[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) hi[k] = lo[k] = 0;
    auto put = [&](int k, float v) {
        hi[k] = f32_to_bf16_rne(v);
        lo[k] = f32_to_bf16_rne(v - __builtin_bit_cast(float, (uint32_t)hi[k] << 16));
    };
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int f = 0; f < 2; ++f)  // BatchNorm scale folded in
                put((dy == 0 ? 0 : dy == 1 ? 2 : 1) * 8 + dx * 2 + f, L.w[((size_t)co * 2 + f) * 9 + dy * 3 + dx] * sc);
    put(24, L.shift[co]);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        t.stem_split[P * 32 + k] = hi[k];
        t.stem_split[64 * 32 + P * 32 + k] = lo[k];
    }
}

}  // namespace fiunet
