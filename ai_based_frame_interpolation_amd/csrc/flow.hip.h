// flow.hip.h -- dense optical flow (Farneback) and flow-compensated frame warps on device, gfx950 only.
//
// The definition is the one optical_flow.py states in torch (G. Farneback, "Two-Frame Motion Estimation Based on
// Polynomial Expansion", SCIA 2003, with the parameters the reference's evaluators pass: pyr_scale 0.5, 3 levels,
// winsize 15, 3 iterations, poly_n 5, poly_sigma 1.1, box window, min_size 32; evaluation_simple.py:76-103).  One
// kernel per stage, batched over frame pairs with blockIdx.z; intermediates are planar fp32 ([B, 5, h, w] polynomial
// coefficients and normal equations, [B, 2, h, w] flow).  No pair reads anything of another pair and no sum depends on
// the launch shape, so a pair's flow is the same to the last bit alone and at any position of any batch.
//
//   flow_blur_kernel             separable Gaussian of the full-resolution frame, read where it lies (uint8, or
//                                uint16 holding 10-bit codes, which enter as code / 4 so that the regulariser and the
//                                border constants keep their meaning); reflect-101 border, replicate where the image
//                                is not larger than the radius
//   flow_resize_kernel           cv2.resize-style linear resampling, (dst + 0.5) * scale - 0.5 with weight 0 outside
//                                the image, times a factor per channel: the pyramid level of the blurred frame, the
//                                flow of the coarser level times 1 / pyr_scale
//   flow_polyexp_kernel          vertical 11-tap pass with g, x g, x^2 g, then the horizontal pass, replicated
//                                borders, from an LDS tile with a 5-pixel halo -> the five channels of poly_exp
//   flow_update_matrices_kernel  bilinear gather of R1 at the displaced position, the `inside` rule, the border
//                                attenuation, the five normal-equation channels
//   flow_boxsolve_kernel         15x15 box mean with replicated border and the 2x2 solve (+1e-3, IEEE division)
//   flow_warp_kernel             remap's fixed-point bilinear sampling at p + s * flow(p) / 2: coordinates clamped to
//                                the image in fp32, rounded half-to-even to 1/32 pixel, 15-bit integer weights,
//                                (acc + 2^14) >> 15.  The four weights of the cell (a, b) / 32 are 32 (32-a)(32-b),
//                                32 a (32-b), 32 (32-a) b, 32 a b: the products remap_bilinear_u8 rounds are whole
//                                numbers that sum to 2^15, so its rounding and its correction never act and no table
//                                is needed (tests/test_flow_host.py compares all 1024 cells with the Python code).
//                                A flow field of another size than the plane (luma flow, chroma plane) is resampled
//                                at the pixel with flow_resize_kernel's arithmetic and scaled per axis.
//   flow_warp_table_kernel       motion-compensated resampling: one plane of up to 64 output frames,
//                                each warped along the flow between two neighbouring grid rows to its own time
//                                wn / den; planes are read and written where they lie (offset, pitch, step)
//   flow_fetch, flow_warp_pair   the warp's arithmetic at one sample, stated once: flow_warp_table_kernel and the chroma
//                                kernels of chroma.hip.h go through them
// Every one is a stencil or a gather: HBM- or LDS-bound, no MFMA, no atomics.  The build has -ffp-contract=off, so
// every product and sum below rounds on its own, in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "retime.hip.h"   // retime_div: the blend's exact division by den

namespace fiunet {

constexpr int FLOW_TX = 64, FLOW_TY = 16;          // output pixels per workgroup of the tiled kernels
constexpr int FLOW_BLUR_MAXR = 9;                  // level 3: ksize 19
constexpr int FLOW_POLY_N = 5, FLOW_WIN = 15, FLOW_WIN_R = FLOW_WIN / 2;

struct FlowBlurTaps {   // by value in the kernel arguments
    float k[2 * FLOW_BLUR_MAXR + 1];
    int r, reflect;
};
struct FlowPolyTaps {
    float g[2 * FLOW_POLY_N + 1], xg[2 * FLOW_POLY_N + 1], xxg[2 * FLOW_POLY_N + 1];
    float ig11, ig03, ig33, ig55;
};

template <typename T> struct FlowSample;
template <> struct FlowSample<uint8_t> {
    static constexpr int PEAK = 255;
    static __device__ __forceinline__ int code(unsigned v) { return (int)v; }
    static __device__ __forceinline__ float get(unsigned v) { return (float)v; }
};
template <> struct FlowSample<uint16_t> {   // (a word above 1023 reads as 1023, as in every 10-bit kernel here)
    static constexpr int PEAK = 1023;
    static __device__ __forceinline__ int code(unsigned v) { return (int)min(v, 1023u); }
    static __device__ __forceinline__ float get(unsigned v) { return (float)min(v, 1023u) * 0.25f; }
};

__device__ __forceinline__ int flow_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// BORDER_REFLECT_101 (needs n > radius) or replicate; then clamped, for the tile positions past the image whose
// results are never stored
__device__ __forceinline__ int flow_border(int i, int n, int reflect)
{
    if (reflect) i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return flow_clampi(i, 0, n - 1);
}

// grid = (tiles_x, tiles_y, B); dst [B, H, W]
template <typename T>
__global__ __launch_bounds__(256) void flow_blur_kernel(const T* __restrict__ src, size_t image_stride, size_t row_pitch,
                                                        int H, int W, FlowBlurTaps taps, float* __restrict__ dst)
{
    constexpr int MIW = FLOW_TX + 2 * FLOW_BLUR_MAXR, MIH = FLOW_TY + 2 * FLOW_BLUR_MAXR;
    __shared__ float tin[MIH][MIW + 1];
    __shared__ float hs[MIH][FLOW_TX];
    const int tid = threadIdx.x, r = taps.r, IW = FLOW_TX + 2 * r, IH = FLOW_TY + 2 * r;
    const int x0 = blockIdx.x * FLOW_TX, y0 = blockIdx.y * FLOW_TY;
    const T* p = src + (size_t)blockIdx.z * image_stride;
    for (int i = tid; i < IH * IW; i += 256) {
        const int rr = i / IW, c = i - rr * IW;
        const int y = flow_border(y0 + rr - r, H, taps.reflect), x = flow_border(x0 + c - r, W, taps.reflect);
        tin[rr][c] = FlowSample<T>::get(p[(size_t)y * row_pitch + x]);
    }
    __syncthreads();
    for (int i = tid; i < IH * FLOW_TX; i += 256) {
        const int rr = i / FLOW_TX, c = i - rr * FLOW_TX;
        float s = 0.f;
        for (int k = 0; k <= 2 * r; ++k) s += taps.k[k] * tin[rr][c + k];
        hs[rr][c] = s;
    }
    __syncthreads();
    float* o = dst + (size_t)blockIdx.z * H * W;
    for (int i = tid; i < FLOW_TY * FLOW_TX; i += 256) {
        const int rr = i / FLOW_TX, c = i - rr * FLOW_TX;
        if (y0 + rr >= H || x0 + c >= W) continue;
        float s = 0.f;
        for (int k = 0; k <= 2 * r; ++k) s += taps.k[k] * hs[rr + k][c];
        o[(size_t)(y0 + rr) * W + x0 + c] = s;
    }
}

// one axis of cv2.resize's INTER_LINEAR: source coordinate (d + 0.5) * n_src / n_dst - 0.5 in fp64, the two clamped
// indices and the fp32 weight of the second, 0 where the first index is outside [0, n_src - 2]
__device__ __forceinline__ void flow_axis(int d, int n_dst, int n_src, int& i0c, int& i1c, float& t)
{
    const double f = ((double)d + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
    const double fl = floor(f);
    const int i0 = (int)fl;
    t = (i0 < 0 || i0 >= n_src - 1) ? 0.f : (float)(f - fl);
    i0c = flow_clampi(i0, 0, n_src - 1);
    i1c = flow_clampi(i0 + 1, 0, n_src - 1);
}

// `pix` floats between neighbouring pixels of the source plane (1: planar, 2: one channel of an interleaved field)
__device__ __forceinline__ float flow_resample(const float* __restrict__ s, int ws, int pix, int y0, int y1, float ty,
                                               int x0, int x1, float tx)
{
    const float a = s[((size_t)y0 * ws + x0) * pix], b = s[((size_t)y0 * ws + x1) * pix];
    const float c = s[((size_t)y1 * ws + x0) * pix], d = s[((size_t)y1 * ws + x1) * pix];
    const float top = a * (1.f - tx) + b * tx, bot = c * (1.f - tx) + d * tx;
    return top * (1.f - ty) + bot * ty;
}

// grid = (ceil(wd / 64), ceil(hd / 4), B * C), block (64, 4); src [B, C, hs, ws] -> dst [B, C, hd, wd] times mul[c]
__global__ __launch_bounds__(256) void flow_resize_kernel(const float* __restrict__ src, int hs, int ws,
                                                          float* __restrict__ dst, int hd, int wd, int C, float mul0,
                                                          float mul1)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= wd || y >= hd) return;
    const int plane = blockIdx.z;
    int y0, y1, x0, x1;
    float ty, tx;
    flow_axis(y, hd, hs, y0, y1, ty);
    flow_axis(x, wd, ws, x0, x1, tx);
    const float v = flow_resample(src + (size_t)plane * hs * ws, ws, 1, y0, y1, ty, x0, x1, tx);
    dst[((size_t)plane * hd + y) * wd + x] = v * ((plane % C) == 0 ? mul0 : mul1);
}

// grid = (tiles_x, tiles_y, B); img [B, h, w] -> R [B, 5, h, w]
__global__ __launch_bounds__(256) void flow_polyexp_kernel(const float* __restrict__ img, int h, int w, FlowPolyTaps tp,
                                                           float* __restrict__ R)
{
    constexpr int N = FLOW_POLY_N, IW = FLOW_TX + 2 * N, IH = FLOW_TY + 2 * N;
    __shared__ float tin[IH][IW + 1];
    __shared__ float v0[FLOW_TY][IW + 1], v1[FLOW_TY][IW + 1], v2[FLOW_TY][IW + 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FLOW_TX, y0 = blockIdx.y * FLOW_TY;
    const float* p = img + (size_t)blockIdx.z * h * w;
    for (int i = tid; i < IH * IW; i += 256) {
        const int rr = i / IW, c = i - rr * IW;
        const int y = flow_clampi(y0 + rr - N, 0, h - 1), x = flow_clampi(x0 + c - N, 0, w - 1);
        tin[rr][c] = p[(size_t)y * w + x];
    }
    __syncthreads();
    // vertical pass: r0 = g * f, r1 = (y g) * f, r2 = (y^2 g) * f
    for (int i = tid; i < FLOW_TY * IW; i += 256) {
        const int rr = i / IW, c = i - rr * IW;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * N; ++k) {
            const float v = tin[rr + k][c];
            s0 += tp.g[k] * v;
            s1 += tp.xg[k] * v;
            s2 += tp.xxg[k] * v;
        }
        v0[rr][c] = s0; v1[rr][c] = s1; v2[rr][c] = s2;
    }
    __syncthreads();
    const size_t hw = (size_t)h * w;
    float* o = R + (size_t)blockIdx.z * 5 * hw;
    for (int i = tid; i < FLOW_TY * FLOW_TX; i += 256) {
        const int rr = i / FLOW_TX, c = i - rr * FLOW_TX;
        if (y0 + rr >= h || x0 + c >= w) continue;
        float b1 = 0.f, b2 = 0.f, b4 = 0.f, b3 = 0.f, b6 = 0.f, b5 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * N; ++k) {
            const float a0 = v0[rr][c + k], a1 = v1[rr][c + k], a2 = v2[rr][c + k];
            b1 += tp.g[k] * a0;
            b2 += tp.xg[k] * a0;
            b4 += tp.xxg[k] * a0;
            b3 += tp.g[k] * a1;
            b6 += tp.xg[k] * a1;
            b5 += tp.g[k] * a2;
        }
        const size_t q = (size_t)(y0 + rr) * w + x0 + c;
        o[q] = b3 * tp.ig11;
        o[hw + q] = b2 * tp.ig11;
        o[2 * hw + q] = b1 * tp.ig03 + b5 * tp.ig33;
        o[3 * hw + q] = b1 * tp.ig03 + b4 * tp.ig33;
        o[4 * hw + q] = b6 * tp.ig55;
    }
}

// the attenuation of the 5 outermost rows / columns (an axis shorter than 10 takes both ends' factors)
__device__ __forceinline__ float flow_border_scale(int i, int n)
{
    const int k = min(5, n), j = n - 1 - i;   // {0.14, 0.14, 0.4472, 0.4472, 0.4472} from either end
    float s = 1.f;
    if (i < k) s *= i < 2 ? 0.14f : 0.4472f;
    if (j < k) s *= j < 2 ? 0.14f : 0.4472f;
    return s;
}

// grid = (ceil(w / 64), ceil(h / 4), B), block (64, 4); R0, R1 [B, 5, h, w], flow [B, 2, h, w] -> M [B, 5, h, w]
__global__ __launch_bounds__(256) void flow_update_matrices_kernel(const float* __restrict__ R0,
                                                                   const float* __restrict__ R1,
                                                                   const float* __restrict__ flow, int h, int w,
                                                                   float* __restrict__ M)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t hw = (size_t)h * w, q = (size_t)y * w + x;
    const float* f = flow + (size_t)blockIdx.z * 2 * hw;
    const float* a = R0 + (size_t)blockIdx.z * 5 * hw;
    const float* b = R1 + (size_t)blockIdx.z * 5 * hw;
    const float dx = f[q], dy = f[hw + q];
    const float fx = (float)x + dx, fy = (float)y + dy;
    const float x1f = floorf(fx), y1f = floorf(fy);
    const float ax = fx - x1f, ay = fy - y1f;
    // (compared as floats: a NaN or a huge displacement is simply not inside, and is never converted)
    const bool inside = x1f >= 0.f && x1f < (float)(w - 1) && y1f >= 0.f && y1f < (float)(h - 1);
    float r2, r3, r4, r5, r6;
    if (inside) {
        const size_t g = (size_t)(int)y1f * w + (int)x1f;
        float s[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const float* pc = b + c * hw + g;
            s[c] = pc[0] * (1.f - ax) * (1.f - ay) + pc[1] * ax * (1.f - ay) + pc[w] * (1.f - ax) * ay +
                   pc[w + 1] * ax * ay;
        }
        r2 = s[0];
        r3 = s[1];
        r4 = (a[2 * hw + q] + s[2]) * 0.5f;
        r5 = (a[3 * hw + q] + s[3]) * 0.5f;
        r6 = (a[4 * hw + q] + s[4]) * 0.25f;
    } else {
        r2 = 0.f;
        r3 = 0.f;
        r4 = a[2 * hw + q];
        r5 = a[3 * hw + q];
        r6 = a[4 * hw + q] * 0.5f;
    }
    r2 = (a[q] - r2) * 0.5f;
    r3 = (a[hw + q] - r3) * 0.5f;
    r2 = r2 + r4 * dy + r6 * dx;
    r3 = r3 + r6 * dy + r5 * dx;
    const float sc = flow_border_scale(y, h) * flow_border_scale(x, w);
    r2 *= sc; r3 *= sc; r4 *= sc; r5 *= sc; r6 *= sc;
    float* o = M + (size_t)blockIdx.z * 5 * hw;
    o[q] = r4 * r4 + r6 * r6;
    o[hw + q] = (r4 + r5) * r6;
    o[2 * hw + q] = r5 * r5 + r6 * r6;
    o[3 * hw + q] = r4 * r2 + r6 * r3;
    o[4 * hw + q] = r6 * r2 + r5 * r3;
}

// grid = (tiles_x, tiles_y, B); M [B, 5, h, w] -> flow: (dx, dy) of pixel q of pair b at out[b * batch_stride +
// c * chan_stride + q * pix_stride] (planar [B, 2, h, w]: 2hw, hw, 1; interleaved [B, h, w, 2]: 2hw, 1, 2)
__global__ __launch_bounds__(256) void flow_boxsolve_kernel(const float* __restrict__ M, int h, int w,
                                                            float* __restrict__ out, size_t batch_stride,
                                                            size_t chan_stride, size_t pix_stride)
{
    constexpr int RW = FLOW_WIN_R, IW = FLOW_TX + 2 * RW, IH = FLOW_TY + 2 * RW;
    __shared__ float tin[IH][IW + 1];
    __shared__ float hs[IH][FLOW_TX];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FLOW_TX, y0 = blockIdx.y * FLOW_TY;
    const size_t hw = (size_t)h * w;
    constexpr int PER = FLOW_TY * FLOW_TX / 256;
    float S[5][PER];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const float* p = M + ((size_t)blockIdx.z * 5 + c) * hw;
        if (c) __syncthreads();   // the passes of the channel before have read both tiles
        for (int i = tid; i < IH * IW; i += 256) {
            const int rr = i / IW, cc = i - rr * IW;
            const int y = flow_clampi(y0 + rr - RW, 0, h - 1), x = flow_clampi(x0 + cc - RW, 0, w - 1);
            tin[rr][cc] = p[(size_t)y * w + x];
        }
        __syncthreads();
        for (int i = tid; i < IH * FLOW_TX; i += 256) {
            const int rr = i / FLOW_TX, cc = i - rr * FLOW_TX;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < FLOW_WIN; ++k) s += tin[rr][cc + k];
            hs[rr][cc] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * 256, rr = i / FLOW_TX, cc = i - rr * FLOW_TX;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < FLOW_WIN; ++k) s += hs[rr + k][cc];
            S[c][j] = s / (float)(FLOW_WIN * FLOW_WIN);
        }
    }
    float* o = out + (size_t)blockIdx.z * batch_stride;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * 256, rr = i / FLOW_TX, cc = i - rr * FLOW_TX;
        if (y0 + rr >= h || x0 + cc >= w) continue;
        const float g11 = S[0][j], g12 = S[1][j], g22 = S[2][j], h1 = S[3][j], h2 = S[4][j];
        const float idet = 1.0f / (g11 * g22 - g12 * g12 + 1e-3f);
        const size_t q = ((size_t)(y0 + rr) * w + x0 + cc) * pix_stride;
        o[q] = (g11 * h2 - g12 * h1) * idet;
        o[chan_stride + q] = (g22 * h1 - g12 * h2) * idet;
    }
}

// remap_bilinear_u8 at (mx, my), both already inside [0, w-1] x [0, h-1]
template <typename T>
__device__ __forceinline__ int flow_remap(const T* __restrict__ p, size_t pitch, int h, int w, float mx, float my)
{
    const int sx = (int)rintf(mx * 32.f), sy = (int)rintf(my * 32.f);   // round half to even, as torch.round
    const int xq = sx >> 5, yq = sy >> 5, a = sx & 31, b = sy & 31;
    const int xa = flow_clampi(xq, 0, w - 1), xb = flow_clampi(xq + 1, 0, w - 1);
    const int ya = flow_clampi(yq, 0, h - 1), yb = flow_clampi(yq + 1, 0, h - 1);
    const int acc = FlowSample<T>::code(p[(size_t)ya * pitch + xa]) * ((32 - a) * (32 - b) * 32) +
                    FlowSample<T>::code(p[(size_t)ya * pitch + xb]) * (a * (32 - b) * 32) +
                    FlowSample<T>::code(p[(size_t)yb * pitch + xa]) * ((32 - a) * b * 32) +
                    FlowSample<T>::code(p[(size_t)yb * pitch + xb]) * (a * b * 32);
    return (acc + (1 << 14)) >> 15;
}

__device__ __forceinline__ float flow_clampf(float v, float hi)
{
    return fminf(fmaxf(v, 0.f), hi);   // (a NaN comes out as 0: every index below stays inside the plane)
}

enum { FLOW_MODE_REFERENCE = 0, FLOW_MODE_MOTION = 1 };

// grid = (ceil(w / 64), ceil(h / 4), B), block (64, 4); flow [B, fh, fw, 2] = (dx, dy)
template <typename T>
__global__ __launch_bounds__(256) void flow_warp_kernel(const T* __restrict__ f0, const T* __restrict__ f1,
                                                        size_t image_stride, size_t row_pitch,
                                                        const float* __restrict__ flow, int fh, int fw, int mode, int h,
                                                        int w, float mulx, float muly, T* __restrict__ out,
                                                        size_t out_image_stride, size_t out_row_pitch)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float* fl = flow + (size_t)blockIdx.z * fh * fw * 2;
    float dx, dy;
    if (fh == h && fw == w) {
        const float2 v = reinterpret_cast<const float2*>(fl)[(size_t)y * w + x];
        dx = v.x;
        dy = v.y;
    } else {
        int y0, y1, x0, x1;
        float ty, tx;
        flow_axis(y, h, fh, y0, y1, ty);
        flow_axis(x, w, fw, x0, x1, tx);
        dx = flow_resample(fl, fw, 2, y0, y1, ty, x0, x1, tx) * mulx;
        dy = flow_resample(fl + 1, fw, 2, y0, y1, ty, x0, x1, tx) * muly;
    }
    const float hx = dx * 0.5f, hy = dy * 0.5f, xm = (float)(w - 1), ym = (float)(h - 1);
    const T* p0 = f0 + (size_t)blockIdx.z * image_stride;
    int v;
    if (mode == FLOW_MODE_REFERENCE) {
        v = flow_remap<T>(p0, row_pitch, h, w, flow_clampf((float)x + hx, xm), flow_clampf((float)y + hy, ym));
    } else {
        const T* p1 = f1 + (size_t)blockIdx.z * image_stride;
        const int a = flow_remap<T>(p0, row_pitch, h, w, flow_clampf((float)x - hx, xm), flow_clampf((float)y - hy, ym));
        const int b = flow_remap<T>(p1, row_pitch, h, w, flow_clampf((float)x + hx, xm), flow_clampf((float)y + hy, ym));
        v = (a + b + 1) >> 1;
    }
    out[(size_t)blockIdx.z * out_image_stride + (size_t)y * out_row_pitch + x] = (T)v;
}

// ---- motion-compensated resampling (retime "motion") ------------------------------------------------
// Output frame blockIdx.z of the launch is entry e = table.e[blockIdx.z]: A = grid row e.row, B = the row after it,
// (dx, dy) the flow A -> B at the sample (field e.flow of `flow`, resampled and scaled as in flow_warp_kernel where the
// plane is not the field's size), s0 = fp32(wn / den), s1 = fp32((den - wn) / den), both rounded once on the host:
//   a   = remap(A, clamp(x - s0 dx), clamp(y - s0 dy))        b = remap(B, clamp(x + s1 dx), clamp(y + s1 dy))
//   out = ((den - wn) a + wn b + den / 2) / den               (retime_div: a, b <= 1023 and den <= 2^20)
// every product rounded to fp32, then every sum (__fmul_rn / __fadd_rn / __fsub_rn: never contracted).  2 wn == den is
// flow_warp_kernel's FLOW_MODE_MOTION bit for bit, a zero flow is retime_table_kernel's blend; wn == 0 copies A's samples.
// An entry whose flag (e.flag >= 0: flags[e.flag] on the device) is set writes nothing.  The entries travel in the
// kernel's arguments, as RetimeTable does; the host has checked every index below before the launch.
// One thread makes the consecutive samples of a row that fill a dword (FlowWarpVec<T>: 4 bytes or 2 words); where the
// plane's samples are contiguous (step 1), all of them lie inside the row and the address is aligned, they leave as one
// 4-byte store (8 bytes a thread at 10 bits measured 17 % behind fiunet_flow_warp, a dword level with it).  Eight gathered loads per sample,
// no LDS, no atomics.
constexpr int kFlowWarpTableMax = 64;
template <typename T> struct FlowWarpVec { static constexpr int V = 4 / sizeof(T); };
struct FlowWarpEntry {
    uint32_t row, wn, den, flow;
    int32_t flag;
    float s0, s1;
};
struct FlowWarpTable {
    FlowWarpEntry e[kFlowWarpTableMax];
};
struct FlowWarpPlane {   // sample (y, x) of frame f at off + f * fs + y * pitch + x * step
    size_t off, pitch, fs;
    int step;
};

// remap on a plane whose samples lie `step` apart
template <typename T>
__device__ __forceinline__ int flow_remap_stepped(const T* __restrict__ p, size_t pitch, int step, int h, int w, float mx,
                                                  float my)
{
    const int sx = (int)rintf(mx * 32.f), sy = (int)rintf(my * 32.f);
    const int xq = sx >> 5, yq = sy >> 5, a = sx & 31, b = sy & 31;
    const size_t xa = (size_t)flow_clampi(xq, 0, w - 1) * step, xb = (size_t)flow_clampi(xq + 1, 0, w - 1) * step;
    const size_t ya = (size_t)flow_clampi(yq, 0, h - 1) * pitch, yb = (size_t)flow_clampi(yq + 1, 0, h - 1) * pitch;
    const int acc = FlowSample<T>::code(p[ya + xa]) * ((32 - a) * (32 - b) * 32) +
                    FlowSample<T>::code(p[ya + xb]) * (a * (32 - b) * 32) +
                    FlowSample<T>::code(p[yb + xa]) * ((32 - a) * b * 32) +
                    FlowSample<T>::code(p[yb + xb]) * (a * b * 32);
    return (acc + (1 << 14)) >> 15;
}

// (dx, dy) of the flow at sample (x, y) of a plane `w` wide: the field's own value where the field has the plane's size
// (`same`), else resampled and scaled as in flow_warp_kernel; (y0, y1, ty): flow_axis of the row, made once by the caller
__device__ __forceinline__ void flow_fetch(const float* __restrict__ fl, int fh, int fw, bool same, int w, int x, int y,
                                           int y0, int y1, float ty, float mulx, float muly, float& dx, float& dy)
{
    if (same) {
        const float2 f = reinterpret_cast<const float2*>(fl)[(size_t)y * w + x];
        dx = f.x;
        dy = f.y;
    } else {
        int xa, xb;
        float tx;
        flow_axis(x, w, fw, xa, xb, tx);
        dx = flow_resample(fl, fw, 2, y0, y1, ty, xa, xb, tx) * mulx;
        dy = flow_resample(fl + 1, fw, 2, y0, y1, ty, xa, xb, tx) * muly;
    }
}

// The warp's two samples at (x, y): a = remap(A, clamp(p - s0 d)), b = remap(B, clamp(p + s1 d)), every product rounded
// to fp32, then every sum.  The one statement of this arithmetic: flow_warp_table_kernel and the chroma kernels
// (chroma.hip.h) both go through it.
template <typename T>
__device__ __forceinline__ void flow_warp_pair(const T* __restrict__ pa, size_t pitch_a, int step_a,
                                               const T* __restrict__ pb, size_t pitch_b, int step_b, int h, int w, int x,
                                               int y, float dx, float dy, float s0, float s1, int& a, int& b)
{
    const float fx = (float)x, fy = (float)y, xm = (float)(w - 1), ym = (float)(h - 1);
    a = flow_remap_stepped<T>(pa, pitch_a, step_a, h, w, flow_clampf(__fsub_rn(fx, __fmul_rn(s0, dx)), xm),
                              flow_clampf(__fsub_rn(fy, __fmul_rn(s0, dy)), ym));
    b = flow_remap_stepped<T>(pb, pitch_b, step_b, h, w, flow_clampf(__fadd_rn(fx, __fmul_rn(s1, dx)), xm),
                              flow_clampf(__fadd_rn(fy, __fmul_rn(s1, dy)), ym));
}

// grid = (ceil(ceil(w / V) / 64), ceil(h / 4), entries of the launch), block (64, 4)
template <typename T>
__global__ __launch_bounds__(256) void flow_warp_table_kernel(const T* __restrict__ grid, FlowWarpPlane gp,
                                                              const float* __restrict__ flow, int fh, int fw,
                                                              float mulx, float muly, const uint8_t* __restrict__ flags,
                                                              const FlowWarpTable table, int h, int w,
                                                              T* __restrict__ out, FlowWarpPlane op)
{
    constexpr int V = FlowWarpVec<T>::V;
    const FlowWarpEntry e = table.e[blockIdx.z];   // gridDim.z <= kFlowWarpTableMax
    if (e.flag >= 0 && flags[e.flag]) return;      // (uniform over the workgroup)
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * V, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= w || y >= h) return;
    const T* pa = grid + gp.off + (size_t)e.row * gp.fs;
    const T* pb = pa + gp.fs;
    T* po = out + op.off + (size_t)blockIdx.z * op.fs + (size_t)y * op.pitch + (size_t)x0 * op.step;
    const float* fl = flow + (size_t)e.flow * fh * fw * 2;
    const float rq = 1.0f / (float)e.den;
    const unsigned wa = e.den - e.wn, wb = e.wn, half = e.den >> 1;
    const bool same = fh == h && fw == w;
    int y0 = 0, y1 = 0;
    float ty = 0.f;
    if (!same) flow_axis(y, h, fh, y0, y1, ty);
    const int nv = min(V, w - x0);
    unsigned v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        v[k] = 0;
        if (k >= nv) continue;
        const int x = x0 + k;
        if (wb == 0) {   // a copy of A's sample as it is stored
            v[k] = pa[(size_t)y * gp.pitch + (size_t)x * gp.step];
            continue;
        }
        float dx, dy;
        flow_fetch(fl, fh, fw, same, w, x, y, y0, y1, ty, mulx, muly, dx, dy);
        int a, b;
        flow_warp_pair<T>(pa, gp.pitch, gp.step, pb, gp.pitch, gp.step, h, w, x, y, dx, dy, e.s0, e.s1, a, b);
        v[k] = retime_div((unsigned)a * wa + (unsigned)b * wb + half, e.den, rq);
    }
    if (op.step == 1 && nv == V && ((uintptr_t)po & (V * sizeof(T) - 1)) == 0) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) word |= v[k] << (8 * sizeof(T) * k);
        *reinterpret_cast<uint32_t*>(po) = word;
        return;
    }
    for (int k = 0; k < nv; ++k) po[(size_t)k * op.step] = (T)v[k];
}

}  // namespace fiunet
