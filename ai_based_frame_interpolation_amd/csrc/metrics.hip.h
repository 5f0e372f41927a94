// metrics.hip.h -- image-quality metrics of the evaluation path on device, gfx950 only.
//
// The reference scores every interpolated frame on the HOST with scikit-image
// (/root/reference/model/evaluation.py:194-218, evaluation_simple.py:134-156:
// peak_signal_noise_ratio(target, pred, data_range=255), structural_similarity(target, pred,
// data_range=255)) after postprocess_image has produced the uint8 frame.  With the forward on the
// GPU those two host passes (plus the device->host copy of every frame) become the bottleneck of an
// evaluation run, so both are computed here from the uint8 frames fiunet_forward_u8 leaves in HBM.
//
//   sqdiff_kernel / psnr_finalize_kernel : sum (a-b)^2 as an exact 64-bit integer, then
//                                          10*log10(peak^2 / (sum/n)) in fp64
//   SSIM_OF_TILE / ssim_finalize_kernel  : skimage's default SSIM: 7x7 uniform window, sample covariance
//                                          (49/48), K1 = 0.01, K2 = 0.03, data_range = the peak, mean over
//                                          the image minus a 3-pixel border.  Window sums of a, b, a^2, b^2,
//                                          ab are exact int32; the per-pixel map and its mean are fp64 in a
//                                          fixed order (deterministic).
// Both are HBM-bound (2 bytes read per pixel).
//
// Each is written ONCE, over the sample type and the layout, and every metric entry point runs it: the contiguous
// uint8 batch of the evaluators (fiunet_psnr_u8 / fiunet_ssim_u8) is the tight layout of the planes hold-out scoring
// (holdout.py) reads where they lie - images `image stride` samples apart, rows `row pitch` samples apart, 8-bit
// samples (uint8_t, peak 255) or 10-bit codes in 16-bit words (uint16_t, peak 1023; a word above 1023 reads as 1023,
// as in every 10-bit kernel here, so every sum below stays inside int32).  The evaluators' numbers and the hold-out
// scorer's are therefore the same to the last bit (tests/test_gpu_metrics_bits.py pins them).  SSIM has two kernels
// around its one text, because the tight layout's address arithmetic is measurably cheaper (see ssim_u8_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fiunet {

template <typename T> struct PlaneSample;
template <> struct PlaneSample<uint8_t> {
    static constexpr int PEAK = 255;
    static __device__ __forceinline__ int get(unsigned v) { return (int)v; }
};
template <> struct PlaneSample<uint16_t> {
    static constexpr int PEAK = 1023;
    static __device__ __forceinline__ int get(unsigned v) { return (int)min(v, 1023u); }
};

// ---------------------------------------------------------------------------------------------------
// Squared error.  A row is W*S samples and the sample at position p belongs to component p % S: S = 1 is a plane of
// its own, S = 2..4 interleaved components (U V of NV12, R G B [A] of packed RGB, the byte positions of uyvy422 /
// yuyv422), with S sums per lane, so one pass over the bytes gives every component.  One wave per row at a time.  A
// row whose two base addresses sit at the same offset inside a 16-byte line goes 16 bytes per lane from the first
// aligned sample on, with a scalar head and tail; any other row (an I420 chroma plane against a contiguous copy, an
// odd pitch on one side) is read sample by sample.  Where the rows follow each other on both sides the host cuts the
// run into pieces of sqdiff_seg(S) samples, a multiple of S and of 16 bytes: every row and every piece starts at
// component 0, and every piece of an aligned run keeps the 16-byte path.
__host__ __device__ constexpr unsigned sqdiff_seg(int S) { return S == 3 ? 3072u : 4096u; }

// (a-b)^2 of sample J of a 16-byte vector pair
template <typename T, int J> __device__ __forceinline__ unsigned sqdiff_at(const unsigned (&wa)[4], const unsigned (&wb)[4])
{
    constexpr int BITS = 8 * sizeof(T), N = 4 / sizeof(T);
    constexpr unsigned MASK = (1u << BITS) - 1u;
    const int d = PlaneSample<T>::get((wa[J / N] >> (BITS * (J % N))) & MASK) -
                  PlaneSample<T>::get((wb[J / N] >> (BITS * (J % N))) & MASK);
    return (unsigned)(d * d);
}

template <typename T, int S, int J = 0> struct VecSlots {   // slot[j % S] += (a-b)^2 of sample j, j = J .. VEC-1
    static __device__ __forceinline__ void add(const unsigned (&wa)[4], const unsigned (&wb)[4], unsigned (&slot)[S])
    {
        slot[J % S] += sqdiff_at<T, J>(wa, wb);
        VecSlots<T, S, J + 1>::add(wa, wb, slot);
    }
};
template <typename T, int S> struct VecSlots<T, S, (int)(16 / sizeof(T))> {
    static __device__ __forceinline__ void add(const unsigned (&)[4], const unsigned (&)[4], unsigned (&)[S]) {}
};

// grid = (blocks per image, images); `sums` [images * S] zeroed by the caller, image-major.  Integer atomics, one per
// workgroup and component (the per-image counters are a serialisation point in L2): exact in any order.
template <typename T, int S>
__global__ __launch_bounds__(256) void sqdiff_kernel(const T* __restrict__ a, size_t a_image, size_t a_pitch,
                                                     const T* __restrict__ b, size_t b_image, size_t b_pitch,
                                                     unsigned rows, unsigned L, unsigned l_last,
                                                     unsigned long long* __restrict__ sums)
{
    constexpr unsigned VEC = 16 / sizeof(T);
    const size_t img = blockIdx.y;
    const T* ia = a + img * a_image;
    const T* ib = b + img * b_image;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long s[S];
#pragma unroll
    for (int c = 0; c < S; ++c) s[c] = 0;
    for (unsigned r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
        const T* pa = ia + (size_t)r * a_pitch;
        const T* pb = ib + (size_t)r * b_pitch;
        const unsigned len = r + 1 == rows ? l_last : L;
        const bool same = (((uintptr_t)pa ^ (uintptr_t)pb) & 15) == 0;
        const unsigned head = same ? min(len, (unsigned)(((16 - ((uintptr_t)pa & 15)) & 15) / sizeof(T))) : len;
        const unsigned nv = (len - head) / VEC;
        // head (the whole row where the vector path does not apply): position i is component i % S
        for (unsigned i = lane; i < head; i += 64) {
            const int d = PlaneSample<T>::get(pa[i]) - PlaneSample<T>::get(pb[i]);
            const unsigned q = (unsigned)(d * d), c0 = i % S;
#pragma unroll
            for (int c = 0; c < S; ++c) s[c] += c0 == (unsigned)c ? q : 0u;
        }
        const uint4* qa = reinterpret_cast<const uint4*>(pa + head);
        const uint4* qb = reinterpret_cast<const uint4*>(pb + head);
        for (unsigned i = lane; i < nv; i += 64) {
            const uint4 va = qa[i], vb = qb[i];
            const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
            unsigned slot[S];   // by position inside the vector: <= 16 * 255^2, 8 * 1023^2
#pragma unroll
            for (int c = 0; c < S; ++c) slot[c] = 0;
            VecSlots<T, S>::add(wa, wb, slot);
            // the vector's first sample is position head + i * VEC of the row: at S = 3 that phase turns from one
            // vector to the next and again when the lane advances by 64 vectors; at S = 2, 4 it is head % S
            const unsigned phase = (head + i * VEC) % S;
#pragma unroll
            for (int c = 0; c < S; ++c) {   // component c sits in slot (c - phase) mod S
                unsigned v = 0;
#pragma unroll
                for (int k = 0; k < S; ++k) v = (phase + k) % S == (unsigned)c ? slot[k] : v;
                s[c] += v;
            }
        }
        for (unsigned i = head + nv * VEC + lane; i < len; i += 64) {
            const int d = PlaneSample<T>::get(pa[i]) - PlaneSample<T>::get(pb[i]);
            const unsigned q = (unsigned)(d * d), c0 = i % S;
#pragma unroll
            for (int c = 0; c < S; ++c) s[c] += c0 == (unsigned)c ? q : 0u;
        }
    }
    __shared__ unsigned long long part[4][S];
#pragma unroll
    for (int c = 0; c < S; ++c) {
        unsigned long long v = s[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) part[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < S) {
        const unsigned long long t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                     part[3][threadIdx.x];
        if (t) atomicAdd(sums + img * S + threadIdx.x, t);
    }
}

// one thread per sum; +inf for identical planes, as skimage; out_sse (may be NULL) receives the integer sums
__global__ void psnr_finalize_kernel(const unsigned long long* __restrict__ sums, size_t n, double peak,
                                     double* __restrict__ out, unsigned long long* __restrict__ out_sse, int images)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= images) return;
    const double mse = (double)sums[i] / (double)n;
    out[i] = sums[i] == 0 ? __longlong_as_double(0x7ff0000000000000LL) : 10.0 * log10((peak * peak) / mse);
    if (out_sse) out_sse[i] = sums[i];
}

// ---------------------------------------------------------------------------------------------------
// SSIM.  A kernel loads its workgroup's tile of both images into LDS, which is all that depends on where the samples
// lie; the arithmetic is FIUNET_SSIM_OF_TILE, one text for every kernel.
constexpr int SSIM_WIN = 7, SSIM_PAD = 3;
constexpr int SSIM_TX = 64, SSIM_TY = 16;  // output pixels per workgroup
constexpr int SSIM_IW = SSIM_TX + SSIM_WIN - 1, SSIM_IH = SSIM_TY + SSIM_WIN - 1, SSIM_IWP = SSIM_IW + 2;  // the tile

// S over the valid-window pixels of the tile in ta, tb (output pixel (oy, ox) of the cropped map <-> window rows
// oy..oy+6, cols ox..ox+6 of the image), summed in a fixed order into partial[img][tile]: everything after a kernel's
// tile load.  It expands in the kernel, on the kernel's own names (ta, tb, hs, red, tid, oy0, ox0, H, W, img, tile,
// partial), and is not a function on purpose: inlined from one, the same statements compile to other code (another
// prologue order, six more VGPRs at uint16), and this kernel's time moves by 1 % with as little as that
// (profiles/metrics_unify_ab.txt).  Expanded in place, every kernel is byte for byte what it was when each carried its
// own copy (profiles/metrics_unify_kernel_compare.txt), so the speed is unchanged by construction.
#define FIUNET_SSIM_OF_TILE(T)                                                                                     \
    const int OH = H - 2 * SSIM_PAD, OW = W - 2 * SSIM_PAD;                                                        \
    __syncthreads();                                                                                               \
    for (int i = tid; i < IH * SSIM_TX; i += 256) {                                                                \
        const int r = i / SSIM_TX, c = i - r * SSIM_TX;                                                            \
        int sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;                                                             \
        _Pragma("unroll") for (int k = 0; k < SSIM_WIN; ++k) {                                                     \
            const int va = ta[r * IWP + c + k], vb = tb[r * IWP + c + k];                                          \
            sa += va; sb += vb; saa += va * va; sbb += vb * vb; sab += va * vb;                                    \
        }                                                                                                          \
        hs[0][r][c] = sa; hs[1][r][c] = sb; hs[2][r][c] = saa; hs[3][r][c] = sbb; hs[4][r][c] = sab;               \
    }                                                                                                              \
    __syncthreads();                                                                                               \
    constexpr double PEAK = (double)PlaneSample<T>::PEAK;                                                          \
    const double NP = 49.0, cov_norm = NP / (NP - 1.0);                                                            \
    const double C1 = (0.01 * PEAK) * (0.01 * PEAK), C2 = (0.03 * PEAK) * (0.03 * PEAK);                           \
    double acc = 0.0;                                                                                              \
    for (int i = tid; i < SSIM_TY * SSIM_TX; i += 256) {                                                           \
        const int r = i / SSIM_TX, c = i - r * SSIM_TX;                                                            \
        if (oy0 + r >= OH || ox0 + c >= OW) continue;                                                              \
        int s[5] = {0, 0, 0, 0, 0}; /* <= 49 * 1023^2 = 51,279,921 */                                              \
        _Pragma("unroll") for (int k = 0; k < SSIM_WIN; ++k)                                                       \
            _Pragma("unroll") for (int q = 0; q < 5; ++q) s[q] += hs[q][r + k][c];                                 \
        const double ux = (double)s[0] / NP, uy = (double)s[1] / NP;                                               \
        const double uxx = (double)s[2] / NP, uyy = (double)s[3] / NP, uxy = (double)s[4] / NP;                    \
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy);                             \
        const double vxy = cov_norm * (uxy - ux * uy);                                                             \
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;                                                 \
        const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;                                               \
        acc += (A1 * A2) / (B1 * B2);                                                                              \
    }                                                                                                              \
    red[tid] = acc;                                                                                                \
    __syncthreads();                                                                                               \
    for (int o = 128; o > 0; o >>= 1) {                                                                            \
        if (tid < o) red[tid] += red[tid + o];                                                                     \
        __syncthreads();                                                                                           \
    }                                                                                                              \
    if (tid == 0) partial[img * gridDim.x + tile] = red[0];

// The evaluators' contiguous uint8 batch: images of H rows of W samples, one after the other.  grid = (tiles_x *
// tiles_y, images) -> partial[img][tile].  A kernel of its own because one 32 x 32-bit row offset shared by both sides
// is measurably cheaper in the tile load than two 64-bit pitches and two steps: fiunet_ssim_u8 through
// ssim_kernel<uint8_t> took 2.5 % longer (profiles/metrics_unify_ab.txt).
__global__ __launch_bounds__(256) void ssim_u8_kernel(const uint8_t* __restrict__ a,
                                                      const uint8_t* __restrict__ b, int H, int W,
                                                      int tiles_x, double* __restrict__ partial)
{
    constexpr int IW = SSIM_IW, IH = SSIM_IH, IWP = SSIM_IWP;
    __shared__ uint8_t ta[IH * IWP], tb[IH * IWP];
    __shared__ int hs[5][IH][SSIM_TX];  // horizontal 7-sums of a, b, a^2, b^2, ab
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const size_t img = blockIdx.y;
    const uint8_t* pa = a + img * (size_t)H * W;
    const uint8_t* pb = b + img * (size_t)H * W;
    const int oy0 = ty * SSIM_TY, ox0 = tx * SSIM_TX;
    for (int i = tid; i < IH * IW; i += 256) {
        const int r = i / IW, c = i - r * IW;
        const int y = min(oy0 + r, H - 1), x = min(ox0 + c, W - 1);
        ta[r * IWP + c] = pa[(size_t)y * W + x];
        tb[r * IWP + c] = pb[(size_t)y * W + x];
    }
    FIUNET_SSIM_OF_TILE(uint8_t)
}

// Planes where they lie, either depth, same grid: sample (y, x) of an image lies at y * pitch + x * step (step 1: a
// plane of its own; 2..4: one component of interleaved samples, the U of NV12, a byte of packed RGB, the Y of uyvy422).
template <typename T>
__global__ __launch_bounds__(256) void ssim_kernel(const T* __restrict__ a, size_t a_image, size_t a_pitch,
                                                   unsigned a_step, const T* __restrict__ b, size_t b_image,
                                                   size_t b_pitch, unsigned b_step, int H, int W, int tiles_x,
                                                   double* __restrict__ partial)
{
    constexpr int IW = SSIM_IW, IH = SSIM_IH, IWP = SSIM_IWP;
    __shared__ T ta[IH * IWP], tb[IH * IWP];
    __shared__ int hs[5][IH][SSIM_TX];  // horizontal 7-sums of a, b, a^2, b^2, ab (<= 7 * 1023^2)
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const size_t img = blockIdx.y;
    const T* pa = a + img * a_image;
    const T* pb = b + img * b_image;
    const int oy0 = ty * SSIM_TY, ox0 = tx * SSIM_TX;
    for (int i = tid; i < IH * IW; i += 256) {
        const int r = i / IW, c = i - r * IW;
        const int y = min(oy0 + r, H - 1), x = min(ox0 + c, W - 1);
        ta[r * IWP + c] = (T)PlaneSample<T>::get(pa[(size_t)y * a_pitch + (size_t)x * a_step]);
        tb[r * IWP + c] = (T)PlaneSample<T>::get(pb[(size_t)y * b_pitch + (size_t)x * b_step]);
    }
    FIUNET_SSIM_OF_TILE(T)
}
#undef FIUNET_SSIM_OF_TILE

// one workgroup per image: fixed-order sum of the tile partials, then the mean
__global__ __launch_bounds__(256) void ssim_finalize_kernel(const double* __restrict__ partial, int tiles,
                                                            double count, double* __restrict__ out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const double* p = partial + (size_t)blockIdx.x * tiles;
    double acc = 0.0;
    for (int i = tid; i < tiles; i += 256) acc += p[i];
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0] / count;
}

// ---------------------------------------------------------------------------------------------------
// Gaussian-window SSIM of the training loss (/root/reference/model/train.py:18-73, SSIMLoss._ssim):
// depth-wise conv2d of img1, img2, img1*img1, img2*img2, img1*img2 with the normalised
// window_size x window_size Gaussian (sigma 1.5, :27-35), ZERO padding window_size//2 (:38-46),
// C1 = 0.01^2, C2 = 0.03^2 (:48-49), map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2))
// (:51), then a mean (:53-56).  fp32 planes in the caller's value range (the loss is applied to [0,1]
// tensors, train.py:142,192).  The reference's window is the outer product of the normalised 1-D
// Gaussian, so the filter is evaluated separably: horizontal 11-tap sums into LDS, vertical 11-tap sums
// in registers.  The three products are rounded to fp32 first, as the reference's `img1*img1` tensors
// are; all sums, the map and its mean are fp64 in a fixed order (deterministic; the reference's own fp32
// conv carries ~1e-7 of rounding that this does not reproduce, far below the 1e-5 the tests ask for).
// The same pass also returns sum (img1 - img2)^2 per plane for CombinedLoss' MSE term (train.py:75-87).
// Roofline: HBM (8 bytes read per pixel).
// Tile of 16 x 32 output pixels: 36 KiB of LDS per workgroup, four workgroups per CU.  The first version
// (64 x 16 tiles, 82 KiB, ONE workgroup per CU) was latency-bound at one wave per SIMD: 0.69 ms for 8 x 1080p
// frames against 0.30 ms now (-DFIUNET_GSSIM_TX / _TY sweep: 32x16 0.36, 32x32 0.35, 64x8 0.51, 16x48 0.31,
// 16x64 0.34, 8x64 0.31, 8x32 0.33 ms).
#ifndef FIUNET_GSSIM_TX
#define FIUNET_GSSIM_TX 16
#define FIUNET_GSSIM_TY 32
#endif
constexpr int GSSIM_TX = FIUNET_GSSIM_TX, GSSIM_TY = FIUNET_GSSIM_TY, GSSIM_MAXR = 15;
struct GaussWindow { float g[2 * GSSIM_MAXR + 1]; };  // by value in the kernel arguments

// grid = (tiles_x * tiles_y, planes); dynamic LDS: 2 fp32 input tiles + 5 fp64 row-sum planes.
// RT > 0: window radius known at compile time (the reference only ever uses 5); RT == 0: runtime r.
template <int RT>
__global__ __launch_bounds__(256) void ssim_gauss_f32_kernel(const float* __restrict__ a,
                                                             const float* __restrict__ b, int H, int W,
                                                             int tiles_x, int r_arg, GaussWindow win,
                                                             double* __restrict__ partial)
{
    const int R = RT > 0 ? RT : r_arg;
    const int IW = GSSIM_TX + 2 * R, IH = GSSIM_TY + 2 * R, IWP = IW + 1;
    extern __shared__ double gssim_lds[];
    double* hs = gssim_lds;                                    // [5][IH][TX]
    float* ta = reinterpret_cast<float*>(hs + 5 * IH * GSSIM_TX);  // [IH][IWP]
    float* tb = ta + IH * IWP;
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const size_t img = blockIdx.y;
    const float* pa = a + img * (size_t)H * W;
    const float* pb = b + img * (size_t)H * W;
    const int oy0 = ty * GSSIM_TY, ox0 = tx * GSSIM_TX;
    double sq = 0.0;
    for (int i = tid; i < IH * IW; i += 256) {
        const int rr = i / IW, c = i - rr * IW;
        const int y = oy0 + rr - R, x = ox0 + c - R;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;  // F.conv2d padding: zeros
        const float va = in ? pa[(size_t)y * W + x] : 0.f, vb = in ? pb[(size_t)y * W + x] : 0.f;
        ta[rr * IWP + c] = va;
        tb[rr * IWP + c] = vb;
        // every image pixel belongs to exactly one tile's interior
        if (in && rr >= R && rr < R + GSSIM_TY && c >= R && c < R + GSSIM_TX) {
            const float d = va - vb;  // nn.MSELoss: fp32 difference
            sq += (double)d * (double)d;
        }
    }
    __syncthreads();
    for (int i = tid; i < IH * GSSIM_TX; i += 256) {
        const int rr = i / GSSIM_TX, c = i - rr * GSSIM_TX;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int k = 0; k < 2 * R + 1; ++k) {
            const float va = ta[rr * IWP + c + k], vb = tb[rr * IWP + c + k];
            const double g = (double)win.g[k];
            s0 = fma(g, (double)va, s0);
            s1 = fma(g, (double)vb, s1);
            s2 = fma(g, (double)(va * va), s2);
            s3 = fma(g, (double)(vb * vb), s3);
            s4 = fma(g, (double)(va * vb), s4);
        }
        hs[(0 * IH + rr) * GSSIM_TX + c] = s0;
        hs[(1 * IH + rr) * GSSIM_TX + c] = s1;
        hs[(2 * IH + rr) * GSSIM_TX + c] = s2;
        hs[(3 * IH + rr) * GSSIM_TX + c] = s3;
        hs[(4 * IH + rr) * GSSIM_TX + c] = s4;
    }
    __syncthreads();
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double acc = 0.0;
    for (int i = tid; i < GSSIM_TY * GSSIM_TX; i += 256) {
        const int rr = i / GSSIM_TX, c = i - rr * GSSIM_TX;
        if (oy0 + rr >= H || ox0 + c >= W) continue;
        double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 2 * R + 1; ++k) {
            const double g = (double)win.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) s[q] = fma(g, hs[(q * IH + rr + k) * GSSIM_TX + c], s[q]);
        }
        const double mu1 = s[0], mu2 = s[1];
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const double s1 = s[2] - mu1_sq, s2 = s[3] - mu2_sq, s12 = s[4] - mu1_mu2;
        acc += ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
    }
    red[0][tid] = acc;
    red[1][tid] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        partial[(img * gridDim.x + tile) * 2 + 0] = red[0][0];
        partial[(img * gridDim.x + tile) * 2 + 1] = red[1][0];
    }
}

// one workgroup per plane: fixed-order sums of the tile partials -> mean SSIM map, sum of squared error
__global__ __launch_bounds__(256) void ssim_gauss_finalize_kernel(const double* __restrict__ partial, int tiles,
                                                                  double count, double* __restrict__ out_ssim,
                                                                  double* __restrict__ out_sqerr)
{
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    const double* p = partial + (size_t)blockIdx.x * tiles * 2;
    double acc = 0.0, sq = 0.0;
    for (int i = tid; i < tiles; i += 256) {
        acc += p[2 * i];
        sq += p[2 * i + 1];
    }
    red[0][tid] = acc;
    red[1][tid] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out_ssim[blockIdx.x] = red[0][0] / count;
        if (out_sqerr) out_sqerr[blockIdx.x] = red[1][0];
    }
}

}  // namespace fiunet
