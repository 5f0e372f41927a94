// metrics.hip -- PSNR and SSIM on the GPU (metrics.hip.h): the uint8 batch metrics and the plane / interleaved / stepped
// metrics of hold-out scoring - each entry point its own argument checks, then the same launches - and the Gaussian SSIM
// of the training loss.
#include "fiunet_internal.h"
#include "plane_check.h"
#include "metrics.hip.h"

#include <cmath>

using namespace fiunet;

extern "C" {

static inline int ssim_tiles(int H, int W, int* tiles_x)
{
    const int ow = W - 2 * SSIM_PAD, oh = H - 2 * SSIM_PAD;
    const int tx = (ow + SSIM_TX - 1) / SSIM_TX, ty = (oh + SSIM_TY - 1) / SSIM_TY;
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

size_t fiunet_metrics_workspace_bytes(int images, int H, int W)
{
    if (images < 1 || H < 1 || W < 1) {
        last_error() = "fiunet_metrics_workspace_bytes: bad arguments";
        return 0;
    }
    const size_t tiles = (H >= SSIM_WIN && W >= SSIM_WIN) ? (size_t)ssim_tiles(H, W, nullptr) : 0;
    return align256((size_t)images * 8) + align256((size_t)images * tiles * 8);
}

// What every entry point does once its own checks have passed.  One side of a comparison: `images` images `image`
// samples apart, rows `pitch` samples apart, SSIM's samples `step` apart (the squared error has no step: its samples
// follow each other).
struct PlaneSide { const void* p; size_t image, pitch; unsigned step; };

extern "C++" {   // (templates over the sample type, inside this file's extern "C" part)
template <typename T, int S>
static int launch_sqdiff(const PlaneSide& a, const PlaneSide& b, int images, int H, int W, unsigned long long* sums,
                         hipStream_t s)
{
    // rows that follow each other on both sides are one run of H*W*S samples, cut into sqdiff_seg(S) pieces (a
    // multiple of S and of 16 bytes: a piece starts at component 0 and an aligned run keeps the 16-byte path).  (The
    // refusal needs more than 2^44 samples per plane, which no buffer holds: fiunet_psnr_u8, always flat, never
    // answers it in practice.)
    constexpr size_t SEG = sqdiff_seg(S);
    const size_t row = (size_t)W * S, n = (size_t)H * row;
    const bool flat = a.pitch == row && b.pitch == row;
    if (flat && (n + SEG - 1) / SEG > 0xffffffffull) return fail(FIUNET_ERR_INVALID_ARG, "plane too large");
    const unsigned rows = flat ? (unsigned)((n + SEG - 1) / SEG) : (unsigned)H;
    const unsigned len = flat ? (unsigned)SEG : (unsigned)row;
    const unsigned l_last = flat ? (unsigned)(n - (size_t)(rows - 1) * SEG) : (unsigned)row;
    const size_t pa = flat ? SEG : a.pitch, pb = flat ? SEG : b.pitch;
    // one wave per row and step, at most 128 workgroups (= atomics) per image
    const unsigned bx = std::min<unsigned>((rows + 3) / 4, 128u);
    hipLaunchKernelGGL((sqdiff_kernel<T, S>), dim3(bx, (unsigned)images), dim3(256), 0, s, (const T*)a.p, a.image, pa,
                       (const T*)b.p, b.image, pb, rows, len, l_last, sums);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

template <typename T>
static int launch_sqdiff(int S, const PlaneSide& a, const PlaneSide& b, int images, int H, int W,
                         unsigned long long* sums, hipStream_t s)
{
    if (S == 1) return launch_sqdiff<T, 1>(a, b, images, H, W, sums, s);
    if (S == 2) return launch_sqdiff<T, 2>(a, b, images, H, W, sums, s);
    if (S == 3) return launch_sqdiff<T, 3>(a, b, images, H, W, sums, s);
    return launch_sqdiff<T, 4>(a, b, images, H, W, sums, s);
}
}  // extern "C++"

// PSNR (and sse where out_sse is given) of the S components of every image: zero-fill, squared error, finalize.
// `workspace` holds the images * S sums.
static int run_psnr(const PlaneSide& a, const PlaneSide& b, int bits, int S, int images, int H, int W, double* out,
                    unsigned long long* out_sse, void* workspace, hipStream_t s)
{
    unsigned long long* sums = (unsigned long long*)workspace;
    const int planes = images * S;
    if (int rc = zero_fill_async(sums, (size_t)planes * 8, s)) return rc;
    if (int rc = bits == 10 ? launch_sqdiff<uint16_t>(S, a, b, images, H, W, sums, s)
                            : launch_sqdiff<uint8_t>(S, a, b, images, H, W, sums, s))
        return rc;
    hipLaunchKernelGGL(psnr_finalize_kernel, dim3((planes + 63) / 64), dim3(64), 0, s, sums, (size_t)H * W,
                       bits == 10 ? 1023.0 : 255.0, out, out_sse, planes);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

// SSIM of every image: the tile kernel into the partials behind the workspace's sums, then the finalize.
// tight: fiunet_ssim_u8's contiguous uint8 batch, both sides {p, H*W, W, 1}: ssim_u8_kernel takes the two pointers
// and forms that layout from H and W itself.
static int run_ssim(const PlaneSide& a, const PlaneSide& b, int bits, bool tight, int images, int H, int W,
                    double* out, void* workspace, hipStream_t s)
{
    int tx = 0;
    const int tiles = ssim_tiles(H, W, &tx);
    double* partial = (double*)((char*)workspace + align256((size_t)images * 8));
    const dim3 grid((unsigned)tiles, (unsigned)images);
    if (bits == 10)
        hipLaunchKernelGGL(ssim_kernel<uint16_t>, grid, dim3(256), 0, s, (const uint16_t*)a.p, a.image, a.pitch, a.step,
                           (const uint16_t*)b.p, b.image, b.pitch, b.step, H, W, tx, partial);
    else if (tight)
        hipLaunchKernelGGL(ssim_u8_kernel, grid, dim3(256), 0, s, (const uint8_t*)a.p, (const uint8_t*)b.p, H, W, tx,
                           partial);
    else
        hipLaunchKernelGGL(ssim_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)a.p, a.image, a.pitch, a.step,
                           (const uint8_t*)b.p, b.image, b.pitch, b.step, H, W, tx, partial);
    HIP_TRY(hipGetLastError());
    const double count = (double)(H - 2 * SSIM_PAD) * (double)(W - 2 * SSIM_PAD);
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3((unsigned)images), dim3(256), 0, s, partial, tiles, count, out);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_psnr_u8(const uint8_t* pred, const uint8_t* target, int images, int H, int W, double* out,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (!pred || !target || !out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (images < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_BAD_SHAPE, "bad image shape");
    if (images > 65535) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 planes per call");
    if (workspace_bytes < align256((size_t)images * 8)) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    const size_t n = (size_t)H * W;
    return run_psnr({pred, n, (size_t)W, 1}, {target, n, (size_t)W, 1}, 8, 1, images, H, W, out, nullptr, workspace,
                    (hipStream_t)stream);
}

int fiunet_ssim_u8(const uint8_t* pred, const uint8_t* target, int images, int H, int W, double* out,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (!pred || !target || !out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (images < 1) return fail(FIUNET_ERR_BAD_SHAPE, "bad image shape");
    if (H < SSIM_WIN || W < SSIM_WIN)
        return fail(FIUNET_ERR_BAD_SHAPE, "SSIM: the 7x7 window exceeds the image (skimage raises too)");
    if (images > 65535) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 planes per call");
    if (workspace_bytes < fiunet_metrics_workspace_bytes(images, H, W))
        return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    const size_t n = (size_t)H * W;
    return run_ssim({pred, n, (size_t)W, 1}, {target, n, (size_t)W, 1}, 8, true, images, H, W, out, workspace,
                    (hipStream_t)stream);
}

size_t fiunet_plane_metrics_workspace_bytes(int images, int H, int W)
{
    if (images < 1 || H < 1 || W < 1) {
        last_error() = "fiunet_plane_metrics_workspace_bytes: bad arguments";
        return 0;
    }
    return fiunet_metrics_workspace_bytes(images, H, W);
}

// The checks both plane metrics share; every refusal is FIUNET_ERR_INVALID_ARG and comes before any pointer is used.
// pred_row / target_row: the samples a row spans on each side (W; W*S interleaved; (W-1)*step + 1 stepped).
static int check_planes(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, const void* target,
                        size_t target_image_stride, size_t target_row_pitch, int bits, int images, int H, int W,
                        const void* out, const void* workspace, size_t workspace_bytes, size_t need,
                        size_t pred_row = 0, size_t target_row = 0)
{
    if (!pred || !target || !out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (images < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_INVALID_ARG, "bad plane shape");
    if (images > 65535) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 planes per call");
    const char* why = check_pitched(bits, images, H, pred_row ? pred_row : (size_t)W, pred_image_stride, pred_row_pitch, pred, pred);
    if (!why) why = check_pitched(bits, images, H, target_row ? target_row : (size_t)W, target_image_stride, target_row_pitch, target, target);
    if (why) return fail(FIUNET_ERR_INVALID_ARG, std::string("plane layout: ") + why);
    if (workspace_bytes < need) return fail(FIUNET_ERR_INVALID_ARG, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    return FIUNET_OK;
}

int fiunet_plane_psnr(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, const void* target,
                      size_t target_image_stride, size_t target_row_pitch, int bits, int images, int H, int W,
                      double* out_psnr, unsigned long long* out_sse, void* workspace, size_t workspace_bytes,
                      void* stream)
{
    const size_t need = images > 0 ? align256((size_t)images * 8) : 0;
    if (int rc = check_planes(pred, pred_image_stride, pred_row_pitch, target, target_image_stride, target_row_pitch,
                              bits, images, H, W, out_psnr, workspace, workspace_bytes, need))
        return rc;
    return run_psnr({pred, pred_image_stride, pred_row_pitch, 1}, {target, target_image_stride, target_row_pitch, 1},
                    bits, 1, images, H, W, out_psnr, out_sse, workspace, (hipStream_t)stream);
}

int fiunet_stepped_ssim(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, int pred_step,
                              const void* target, size_t target_image_stride, size_t target_row_pitch, int target_step,
                              int bits, int images, int H, int W, double* out_ssim, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    if (pred_step < 1 || pred_step > 4 || target_step < 1 || target_step > 4)
        return fail(FIUNET_ERR_INVALID_ARG, "sample step must be 1, 2, 3 or 4");
    if (H < SSIM_WIN || W < SSIM_WIN)
        return fail(FIUNET_ERR_INVALID_ARG, "SSIM: the 7x7 window exceeds the plane (skimage raises too)");
    const size_t need = images > 0 ? fiunet_metrics_workspace_bytes(images, H, W) : 0;
    if (int rc = check_planes(pred, pred_image_stride, pred_row_pitch, target, target_image_stride, target_row_pitch,
                              bits, images, H, W, out_ssim, workspace, workspace_bytes, need,
                              (size_t)(W - 1) * pred_step + 1, (size_t)(W - 1) * target_step + 1))
        return rc;
    return run_ssim({pred, pred_image_stride, pred_row_pitch, (unsigned)pred_step},
                    {target, target_image_stride, target_row_pitch, (unsigned)target_step}, bits, false, images, H,
                    W, out_ssim, workspace, (hipStream_t)stream);
}

int fiunet_plane_ssim(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, const void* target,
                      size_t target_image_stride, size_t target_row_pitch, int bits, int images, int H, int W,
                      double* out_ssim, void* workspace, size_t workspace_bytes, void* stream)
{
    return fiunet_stepped_ssim(pred, pred_image_stride, pred_row_pitch, 1, target, target_image_stride,
                                     target_row_pitch, 1, bits, images, H, W, out_ssim, workspace, workspace_bytes,
                                     stream);
}

int fiunet_interleaved_psnr(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, const void* target,
                            size_t target_image_stride, size_t target_row_pitch, int bits, int components, int images,
                            int H, int W, double* out_psnr, unsigned long long* out_sse, void* workspace,
                            size_t workspace_bytes, void* stream)
{
    if (components < 2 || components > 4) return fail(FIUNET_ERR_INVALID_ARG, "components must be 2, 3 or 4");
    if (W > (1 << 29)) return fail(FIUNET_ERR_INVALID_ARG, "bad plane shape");
    if (images > 65535 / components)
        return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 component planes (images x components) per call");
    const size_t row = W > 0 ? (size_t)W * components : 0;
    const size_t need = images > 0 ? align256((size_t)images * components * 8) : 0;
    if (int rc = check_planes(pred, pred_image_stride, pred_row_pitch, target, target_image_stride, target_row_pitch,
                              bits, images, H, W, out_psnr, workspace, workspace_bytes, need, row, row))
        return rc;
    return run_psnr({pred, pred_image_stride, pred_row_pitch, 1}, {target, target_image_stride, target_row_pitch, 1},
                    bits, components, images, H, W, out_psnr, out_sse, workspace, (hipStream_t)stream);
}

static inline int gssim_tiles(int H, int W, int* tiles_x)
{
    const int tx = (W + GSSIM_TX - 1) / GSSIM_TX, ty = (H + GSSIM_TY - 1) / GSSIM_TY;
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

size_t fiunet_ssim_gauss_workspace_bytes(int images, int H, int W)
{
    if (images < 1 || H < 1 || W < 1) {
        last_error() = "fiunet_ssim_gauss_workspace_bytes: bad arguments";
        return 0;
    }
    return align256((size_t)images * gssim_tiles(H, W, nullptr) * 2 * 8);
}

int fiunet_ssim_gauss_f32(const float* img1, const float* img2, int images, int H, int W, int window_size,
                          const float* window_1d, double* out_ssim, double* out_sqerr, void* workspace,
                          size_t workspace_bytes, void* stream)
{
    if (!img1 || !img2 || !out_ssim || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (images < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_BAD_SHAPE, "bad image shape");
    if (images > 65535) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 planes per call");
    if (window_size < 1 || window_size > 2 * GSSIM_MAXR + 1 || !(window_size & 1))
        return fail(FIUNET_ERR_UNSUPPORTED, "Gaussian SSIM: window_size must be odd and <= 31 (an even window "
                                            "changes the map size in the reference: padding = window_size//2)");
    if (workspace_bytes < fiunet_ssim_gauss_workspace_bytes(images, H, W))
        return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    // train.py:27-29: fp32 tensor of exp(-(x - ws//2)^2 / (2 sigma^2)) (evaluated in double by numpy), sigma =
    // 1.5 (:32), divided by its fp32 sum
    const int R = window_size / 2;
    GaussWindow win;
    float sum = 0.f;
    for (int x = 0; x < window_size; ++x) {
        win.g[x] = (float)std::exp(-(double)((x - R) * (x - R)) / (2.0 * 1.5 * 1.5));
        sum += win.g[x];
    }
    for (int x = 0; x < window_size; ++x) win.g[x] /= sum;
    // the caller's own normalised window (torch's `gauss / gauss.sum()`: its reduction order decides the last
    // bit of the sum, and the SSIM map's variance terms feel 1 ulp of the window's total at the 1e-7 level)
    if (window_1d)
        for (int x = 0; x < window_size; ++x) win.g[x] = window_1d[x];
    for (int x = window_size; x < 2 * GSSIM_MAXR + 1; ++x) win.g[x] = 0.f;
    hipStream_t s = (hipStream_t)stream;
    int tx = 0;
    const int tiles = gssim_tiles(H, W, &tx);
    double* partial = (double*)workspace;
    const int IH = GSSIM_TY + 2 * R, IW = GSSIM_TX + 2 * R;
    const size_t lds = (size_t)5 * IH * GSSIM_TX * 8 + (size_t)2 * IH * (IW + 1) * 4;
    if (R == 5)
        hipLaunchKernelGGL((ssim_gauss_f32_kernel<5>), dim3((unsigned)tiles, (unsigned)images), dim3(256), lds, s,
                           img1, img2, H, W, tx, R, win, partial);
    else
        hipLaunchKernelGGL((ssim_gauss_f32_kernel<0>), dim3((unsigned)tiles, (unsigned)images), dim3(256), lds, s,
                           img1, img2, H, W, tx, R, win, partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ssim_gauss_finalize_kernel, dim3((unsigned)images), dim3(256), 0, s, partial, tiles,
                       (double)H * (double)W, out_ssim, out_sqerr);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

}  // extern "C"
