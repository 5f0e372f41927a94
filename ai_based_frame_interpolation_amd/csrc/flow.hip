// flow.hip -- Farneback flow and flow-compensated warps (flow.hip.h), with the flow's debug entry points,
// and the motion-guided chroma that is built on the warp (chroma.hip.h).
#include "fiunet_internal.h"
#include "plane_check.h"
#include "flow.hip.h"
#include "chroma.hip.h"

#include <cmath>

using namespace fiunet;

extern "C" {

// ---------------------------------------------------------------------------------------------------
// Farneback flow and flow-compensated warps (flow.hip.h).  The level arithmetic is
// optical_flow.py's: Python's round() is round-half-to-even, which rint() is in the default rounding mode (a
// 130-wide frame has a 32-wide level 2, not 33).
extern "C++" {
namespace {
constexpr int kFlowLevels = 3, kFlowMinSize = 32, kFlowIters = 3;
constexpr size_t kFlowMaxBatch = 4096, kFlowMaxSide = 32768;

// a fiunet_resize_plane that plane_check has passed, as the warp kernels take it
inline FlowWarpPlane warp_plane(const fiunet_resize_plane& p) { return FlowWarpPlane{p.offset, p.pitch, p.frame_stride, p.step}; }

// a plane that is warped or read along a flow carries no filter; plane_check with the flow's bound on a side
const char* warp_plane_check(const fiunet_resize_plane& p)
{
    return p.filter != 0 ? "a plane's filter must be 0" : plane_check(p, (int)kFlowMaxSide);
}

struct FlowLevel { int h, w, ksize; double sigma; };

// -> number of pyramid levels above level 0 (0..3); lv[k] for k = 0..levels
int flow_levels(int H, int W, FlowLevel lv[kFlowLevels + 1])
{
    int levels = 0;
    double scale = 1.0;
    while (levels < kFlowLevels) {
        scale *= 0.5;
        if (W * scale < kFlowMinSize || H * scale < kFlowMinSize) break;
        ++levels;
    }
    for (int k = 0; k <= levels; ++k) {
        const double sc = std::ldexp(1.0, -k);
        lv[k].sigma = (1.0 / sc - 1.0) * 0.5;
        lv[k].ksize = std::max((int)std::rint(lv[k].sigma * 5) | 1, 3);
        lv[k].w = (int)std::rint(W * sc);
        lv[k].h = (int)std::rint(H * sc);
    }
    return levels;
}

// cv2.getGaussianKernel as optical_flow._gauss_kernel_cv states it (ksize 3 with sigma <= 0: the fixed kernel)
FlowBlurTaps flow_blur_taps(int ksize, double sigma, int H, int W)
{
    FlowBlurTaps t = {};
    t.r = ksize / 2;
    t.reflect = std::min(H, W) > t.r ? 1 : 0;
    if (sigma <= 0 && ksize == 3) {
        t.k[0] = 0.25f; t.k[1] = 0.5f; t.k[2] = 0.25f;
        return t;
    }
    if (sigma <= 0) sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
    double v[2 * FLOW_BLUR_MAXR + 1], sum = 0;
    for (int i = 0; i < ksize; ++i) {
        const double x = i - (ksize - 1) * 0.5;
        v[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += v[i];
    }
    for (int i = 0; i < ksize; ++i) t.k[i] = (float)(v[i] / sum);
    return t;
}

// FarnebackPrepareGaussian (optical_flow._poly_exp_setup): g, x g, x^2 g in fp32 and four entries of the inverse of
// the 6x6 Gram matrix of {1, x, y, x^2, y^2, xy} under g(x) g(y), all made in fp64
FlowPolyTaps flow_poly_taps()
{
    constexpr int N = FLOW_POLY_N, K = 2 * N + 1;
    const double sigma = 1.1;
    double g[K], sum = 0;
    for (int i = 0; i < K; ++i) {
        const double x = i - N;
        g[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += g[i];
    }
    FlowPolyTaps t = {};
    for (int i = 0; i < K; ++i) {
        const double x = i - N;
        g[i] /= sum;
        t.g[i] = (float)g[i];
        t.xg[i] = (float)(x * g[i]);
        t.xxg[i] = (float)(x * x * g[i]);
    }
    double G[6][12] = {};
    for (int iy = 0; iy < K; ++iy)
        for (int ix = 0; ix < K; ++ix) {
            const double x = ix - N, y = iy - N, wgt = g[iy] * g[ix];
            const double basis[6] = {1.0, x, y, x * x, y * y, x * y};
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) G[a][b] += wgt * basis[a] * basis[b];
        }
    for (int a = 0; a < 6; ++a) G[a][6 + a] = 1.0;
    for (int c = 0; c < 6; ++c) {   // Gauss-Jordan with partial pivoting
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (std::fabs(G[r][c]) > std::fabs(G[piv][c])) piv = r;
        for (int j = 0; j < 12; ++j) std::swap(G[c][j], G[piv][j]);
        const double d = G[c][c];
        for (int j = 0; j < 12; ++j) G[c][j] /= d;
        for (int r = 0; r < 6; ++r) {
            if (r == c) continue;
            const double f = G[r][c];
            for (int j = 0; j < 12; ++j) G[r][j] -= f * G[c][j];
        }
    }
    t.ig11 = (float)G[1][6 + 1];
    t.ig03 = (float)G[0][6 + 3];
    t.ig33 = (float)G[3][6 + 3];
    t.ig55 = (float)G[5][6 + 5];
    return t;
}

inline dim3 flow_tiles(int h, int w, int B) { return dim3((w + FLOW_TX - 1) / FLOW_TX, (h + FLOW_TY - 1) / FLOW_TY, B); }
inline dim3 flow_rows(int h, int w, int z) { return dim3((w + 63) / 64, (h + 3) / 4, z); }

int flow_check_frames(int bits, int B, int H, int W, size_t image_stride, size_t row_pitch, const void* a, const void* b)
{
    if (B < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_INVALID_ARG, "bad frame shape");
    if ((size_t)B > kFlowMaxBatch || (size_t)H > kFlowMaxSide || (size_t)W > kFlowMaxSide)
        return fail(FIUNET_ERR_INVALID_ARG, "flow: more than 4096 pairs per call or a side above 32768");
    if (const char* why = check_pitched(bits, B, H, (size_t)W, image_stride, row_pitch, a, b))
        return fail(FIUNET_ERR_INVALID_ARG, std::string("frame layout: ") + why);
    return FIUNET_OK;
}

int flow_launch_blur(const void* src, int bits, size_t image_stride, size_t row_pitch, int B, int H, int W,
                     const FlowBlurTaps& taps, float* dst, hipStream_t s)
{
    if (bits == 10)
        hipLaunchKernelGGL(flow_blur_kernel<uint16_t>, flow_tiles(H, W, B), dim3(256), 0, s, (const uint16_t*)src,
                           image_stride, row_pitch, H, W, taps, dst);
    else
        hipLaunchKernelGGL(flow_blur_kernel<uint8_t>, flow_tiles(H, W, B), dim3(256), 0, s, (const uint8_t*)src,
                           image_stride, row_pitch, H, W, taps, dst);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int flow_launch_resize(const float* src, int hs, int ws, float* dst, int hd, int wd, int B, int C, float m0, float m1,
                       hipStream_t s)
{
    hipLaunchKernelGGL(flow_resize_kernel, flow_rows(hd, wd, B * C), dim3(256), 0, s, src, hs, ws, dst, hd, wd, C, m0, m1);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int flow_launch_polyexp(const float* img, int h, int w, int B, const FlowPolyTaps& tp, float* R, hipStream_t s)
{
    hipLaunchKernelGGL(flow_polyexp_kernel, flow_tiles(h, w, B), dim3(256), 0, s, img, h, w, tp, R);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int flow_launch_matrices(const float* R0, const float* R1, const float* flow, int h, int w, int B, float* M, hipStream_t s)
{
    hipLaunchKernelGGL(flow_update_matrices_kernel, flow_rows(h, w, B), dim3(256), 0, s, R0, R1, flow, h, w, M);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int flow_launch_boxsolve(const float* M, int h, int w, int B, float* out, bool interleaved, hipStream_t s)
{
    const size_t hw = (size_t)h * w;
    hipLaunchKernelGGL(flow_boxsolve_kernel, flow_tiles(h, w, B), dim3(256), 0, s, M, h, w, out, 2 * hw,
                       interleaved ? (size_t)1 : hw, interleaved ? (size_t)2 : (size_t)1);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}
}  // namespace
}  // extern "C++"

size_t fiunet_flow_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1 || (size_t)B > kFlowMaxBatch || (size_t)H > kFlowMaxSide || (size_t)W > kFlowMaxSide) {
        last_error() = "fiunet_flow_workspace_bytes: bad arguments";
        return 0;
    }
    // blurred frame, level image, R0, R1, M (5 channels each), two flow fields (2 channels each)
    const size_t plane = align256((size_t)B * H * W * 4);
    return (2 + 3 * 5 + 2 * 2) * plane;
}

int fiunet_farneback_flow(const void* prev, const void* next, int bits, int B, int H, int W, size_t image_stride,
                          size_t row_pitch, float* flow_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!prev || !next || !flow_out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (int rc = flow_check_frames(bits, B, H, W, image_stride, row_pitch, prev, next)) return rc;
    if (workspace_bytes < fiunet_flow_workspace_bytes(B, H, W)) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    if ((uintptr_t)flow_out & 7) return fail(FIUNET_ERR_INVALID_ARG, "flow_out not 8-B aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t plane = align256((size_t)B * H * W * 4);
    char* base = (char*)workspace;
    float* blur = (float*)base;
    float* img = (float*)(base + plane);
    float* R[2] = {(float*)(base + 2 * plane), (float*)(base + 7 * plane)};
    float* M = (float*)(base + 12 * plane);
    float* fl[2] = {(float*)(base + 17 * plane), (float*)(base + 19 * plane)};
    FlowLevel lv[kFlowLevels + 1];
    const int levels = flow_levels(H, W, lv);
    const FlowPolyTaps tp = flow_poly_taps();
    const void* frames[2] = {prev, next};
    int cur = 0;   // fl[cur] holds the flow of the level being refined
    for (int k = levels; k >= 0; --k) {
        const int h = lv[k].h, w = lv[k].w;
        if (k == levels) {
            if (int rc = zero_fill_async(fl[cur], (size_t)B * 2 * h * w * 4, s)) return rc;
        } else {
            if (int rc = flow_launch_resize(fl[cur], lv[k + 1].h, lv[k + 1].w, fl[cur ^ 1], h, w, B, 2, 2.0f, 2.0f, s)) return rc;
            cur ^= 1;
        }
        const FlowBlurTaps taps = flow_blur_taps(lv[k].ksize, lv[k].sigma, H, W);
        for (int f = 0; f < 2; ++f) {
            if (int rc = flow_launch_blur(frames[f], bits, image_stride, row_pitch, B, H, W, taps, blur, s)) return rc;
            if (int rc = flow_launch_resize(blur, H, W, img, h, w, B, 1, 1.0f, 1.0f, s)) return rc;
            if (int rc = flow_launch_polyexp(img, h, w, B, tp, R[f], s)) return rc;
        }
        if (int rc = flow_launch_matrices(R[0], R[1], fl[cur], h, w, B, M, s)) return rc;
        for (int i = 0; i < kFlowIters; ++i) {
            const bool last = k == 0 && i == kFlowIters - 1;
            float* dst = last ? flow_out : fl[cur ^ 1];
            if (int rc = flow_launch_boxsolve(M, h, w, B, dst, last, s)) return rc;
            if (last) break;
            cur ^= 1;
            if (i < kFlowIters - 1)
                if (int rc = flow_launch_matrices(R[0], R[1], fl[cur], h, w, B, M, s)) return rc;
        }
    }
    return FIUNET_OK;
}

int fiunet_flow_warp(const void* frame0, const void* frame1, const float* flow, int mode, int bits, int B, int H, int W,
                     size_t image_stride, size_t row_pitch, int flow_h, int flow_w, void* out, size_t out_image_stride,
                     size_t out_row_pitch, void* stream)
{
    if (!frame0 || !frame1 || !flow || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (mode != FLOW_MODE_REFERENCE && mode != FLOW_MODE_MOTION)
        return fail(FIUNET_ERR_INVALID_ARG, "mode must be FIUNET_FLOW_REFERENCE or FIUNET_FLOW_MOTION");
    if (int rc = flow_check_frames(bits, B, H, W, image_stride, row_pitch, frame0, frame1)) return rc;
    if (int rc = flow_check_frames(bits, B, H, W, out_image_stride, out_row_pitch, out, out)) return rc;
    if (flow_h < 1 || flow_w < 1 || (size_t)flow_h > kFlowMaxSide || (size_t)flow_w > kFlowMaxSide)
        return fail(FIUNET_ERR_INVALID_ARG, "bad flow shape");
    if ((uintptr_t)flow & 7) return fail(FIUNET_ERR_INVALID_ARG, "flow not 8-B aligned");
    hipStream_t s = (hipStream_t)stream;
    const float mx = (float)((double)W / (double)flow_w), my = (float)((double)H / (double)flow_h);
    if (bits == 10)
        hipLaunchKernelGGL(flow_warp_kernel<uint16_t>, flow_rows(H, W, B), dim3(256), 0, s, (const uint16_t*)frame0,
                           (const uint16_t*)frame1, image_stride, row_pitch, flow, flow_h, flow_w, mode, H, W, mx, my,
                           (uint16_t*)out, out_image_stride, out_row_pitch);
    else
        hipLaunchKernelGGL(flow_warp_kernel<uint8_t>, flow_rows(H, W, B), dim3(256), 0, s, (const uint8_t*)frame0,
                           (const uint8_t*)frame1, image_stride, row_pitch, flow, flow_h, flow_w, mode, H, W, mx, my,
                           (uint8_t*)out, out_image_stride, out_row_pitch);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

// ---- motion-compensated resampling (flow_warp_table_kernel) -----------------------------------------
// Everything a thread indexes is checked here, on the host, before the first launch and before a pointer is used.
static_assert(sizeof(fiunet_warp_entry) == 20, "entry layout");

extern "C++" {
namespace {
template <typename T>
int flow_warp_table(const T* grid, int n_rows, const fiunet_resize_plane* gp, const float* flow, int n_flows, int flow_h,
                    int flow_w, const uint8_t* flags, int n_flags, const fiunet_warp_entry* entries, int n_out, T* out,
                    const fiunet_resize_plane* op, void* stream)
{
    if (!grid || !out || !gp || !op || !flow) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)grid | (uintptr_t)out) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n_rows < 0 || n_out < 0 || n_flows < 0 || n_flags < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (n_flags > 0 && !flags) return fail(FIUNET_ERR_INVALID_ARG, "NULL flags");
    for (const fiunet_resize_plane* p : {gp, op})
        if (const char* why = warp_plane_check(*p)) return fail(FIUNET_ERR_INVALID_ARG, why);
    if (gp->h != op->h || gp->w != op->w) return fail(FIUNET_ERR_INVALID_ARG, "the grid's plane and out's differ in size");
    if (flow_h < 1 || flow_w < 1 || (size_t)flow_h > kFlowMaxSide || (size_t)flow_w > kFlowMaxSide)
        return fail(FIUNET_ERR_INVALID_ARG, "bad flow shape");
    if ((uintptr_t)flow & 7) return fail(FIUNET_ERR_INVALID_ARG, "flow not 8-B aligned");
    if (n_out == 0) return FIUNET_OK;
    if (!entries) return fail(FIUNET_ERR_INVALID_ARG, "NULL entries");
    for (int k = 0; k < n_out; ++k) {
        const fiunet_warp_entry& e = entries[k];
        if (e.den < 1 || e.den > kRetimeMaxQ) return fail(FIUNET_ERR_INVALID_ARG, "entry: den outside 1..2^20");
        if (e.wn >= e.den) return fail(FIUNET_ERR_INVALID_ARG, "entry: wn >= den");
        if ((uint64_t)e.row + 1 >= (uint64_t)n_rows)
            return fail(FIUNET_ERR_INVALID_ARG, "entry: `row` and the row after it must lie inside the grid");
        if ((uint64_t)e.flow >= (uint64_t)n_flows) return fail(FIUNET_ERR_INVALID_ARG, "entry: flow outside the flow fields");
        if (e.flag != FIUNET_WARP_NO_FLAG && (e.flag < 0 || e.flag >= n_flags))
            return fail(FIUNET_ERR_INVALID_ARG, "entry: flag outside the flags");
    }
    // n_rows frames of the grid's plane and n_out of out's stay inside the address space and apart from each other
    uintptr_t g0, g1, o0, o1;
    if (!plane_range(grid, sizeof(T), *gp, n_rows, &g0, &g1) || !plane_range(out, sizeof(T), *op, n_out, &o0, &o1))
        return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
    if (ranges_overlap(g0, g1, o0, o1)) return fail(FIUNET_ERR_INVALID_ARG, "out overlaps the grid");
    const int h = gp->h, w = gp->w;
    const float mx = (float)((double)w / (double)flow_w), my = (float)((double)h / (double)flow_h);
    const FlowWarpPlane G = warp_plane(*gp);
    constexpr int V = FlowWarpVec<T>::V;
    const unsigned bx = (unsigned)(((w + V - 1) / V + 63) / 64), by = (unsigned)((h + 3) / 4);
    for (int k0 = 0; k0 < n_out; k0 += kFlowWarpTableMax) {
        const int nk = std::min(n_out - k0, kFlowWarpTableMax);
        FlowWarpTable table = {};
        for (int k = 0; k < nk; ++k) {
            const fiunet_warp_entry& e = entries[k0 + k];
            // s0, s1: computed in double, rounded once
            table.e[k] = FlowWarpEntry{e.row, e.wn, e.den, e.flow, e.flag, (float)((double)e.wn / (double)e.den),
                                       (float)((double)(e.den - e.wn) / (double)e.den)};
        }
        FlowWarpPlane O = warp_plane(*op);
        O.off += (size_t)k0 * op->frame_stride;
        hipLaunchKernelGGL(flow_warp_table_kernel<T>, dim3(bx, by, (unsigned)nk), dim3(256), 0, (hipStream_t)stream, grid,
                           G, flow, flow_h, flow_w, mx, my, flags, table, h, w, out, O);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // namespace
}  // extern "C++"

int fiunet_warp_table_u8(const uint8_t* grid, int n_rows, const fiunet_resize_plane* grid_plane, const float* flow,
                              int n_flows, int flow_h, int flow_w, const uint8_t* flags, int n_flags,
                              const fiunet_warp_entry* entries, int n_out, uint8_t* out,
                              const fiunet_resize_plane* out_plane, void* stream)
{
    return flow_warp_table(grid, n_rows, grid_plane, flow, n_flows, flow_h, flow_w, flags, n_flags, entries, n_out, out,
                           out_plane, stream);
}

int fiunet_warp_table_p10(const uint16_t* grid, int n_rows, const fiunet_resize_plane* grid_plane, const float* flow,
                               int n_flows, int flow_h, int flow_w, const uint8_t* flags, int n_flags,
                               const fiunet_warp_entry* entries, int n_out, uint16_t* out,
                               const fiunet_resize_plane* out_plane, void* stream)
{
    return flow_warp_table(grid, n_rows, grid_plane, flow, n_flows, flow_h, flow_w, flags, n_flags, entries, n_out, out,
                           out_plane, stream);
}

// ---- motion-guided chroma (chroma.hip.h) -----------------------------------------------------------------
// As above: everything a thread indexes is checked here, before the first launch and before a pointer is used.
extern "C++" {
namespace {
template <typename T>
int chroma_pick(const T* a, const fiunet_resize_plane* ap, const T* b, const fiunet_resize_plane* bp, const T* m,
                const fiunet_resize_plane* mp, const float* flow, int n, uint8_t* pick, void* stream)
{
    if (!a || !b || !m || !ap || !bp || !mp || !flow || !pick) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)m) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n < 0 || (size_t)n > kFlowMaxBatch) return fail(FIUNET_ERR_INVALID_ARG, "n must be 0..4096");
    for (const fiunet_resize_plane* p : {ap, bp, mp})
        if (const char* why = warp_plane_check(*p)) return fail(FIUNET_ERR_INVALID_ARG, why);
    if (ap->h != bp->h || ap->w != bp->w || ap->h != mp->h || ap->w != mp->w)
        return fail(FIUNET_ERR_INVALID_ARG, "the three luma planes differ in size");
    if ((uintptr_t)flow & 7) return fail(FIUNET_ERR_INVALID_ARG, "flow not 8-B aligned");
    if (n == 0) return FIUNET_OK;
    const int h = ap->h, w = ap->w, ph = (h + CHROMA_BLOCK - 1) / CHROMA_BLOCK, pw = (w + CHROMA_BLOCK - 1) / CHROMA_BLOCK;
    const uintptr_t k0 = (uintptr_t)pick, k1 = k0 + (size_t)n * ph * pw;
    if (k1 < k0) return fail(FIUNET_ERR_INVALID_ARG, "the pick map leaves the address space");
    const T* bases[3] = {a, b, m};
    const fiunet_resize_plane* planes[3] = {ap, bp, mp};
    for (int i = 0; i < 3; ++i) {
        uintptr_t p0, p1;
        if (!plane_range(bases[i], sizeof(T), *planes[i], n, &p0, &p1)) return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
        if (ranges_overlap(p0, p1, k0, k1)) return fail(FIUNET_ERR_INVALID_ARG, "the pick map overlaps a luma plane");
    }
    const dim3 grid((unsigned)((pw + CHROMA_TILE_X - 1) / CHROMA_TILE_X), (unsigned)((ph + CHROMA_TILE_Y - 1) / CHROMA_TILE_Y),
                    (unsigned)n);
    hipLaunchKernelGGL(chroma_pick_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, a, warp_plane(*ap), b,
                       warp_plane(*bp), m, warp_plane(*mp), flow, h, w, ph, pw, pick);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

template <typename T>
int chroma_fill(const T* a, const fiunet_resize_plane* ap, const T* b, const fiunet_resize_plane* bp, const float* flow,
                int flow_h, int flow_w, const uint8_t* pick, int sy, int sx, int n, T* out, const fiunet_resize_plane* op,
                void* stream)
{
    if (!a || !b || !ap || !bp || !flow || !pick || !out || !op) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n < 0 || (size_t)n > kFlowMaxBatch) return fail(FIUNET_ERR_INVALID_ARG, "n must be 0..4096");
    if ((sy != 1 && sy != 2) || (sx != 1 && sx != 2)) return fail(FIUNET_ERR_INVALID_ARG, "sy and sx must be 1 or 2");
    for (int i = 0; i < 2; ++i)
        for (const fiunet_resize_plane* p : {ap + i, bp + i, op + i}) {
            if (const char* why = warp_plane_check(*p)) return fail(FIUNET_ERR_INVALID_ARG, why);
            if (p->h != ap->h || p->w != ap->w) return fail(FIUNET_ERR_INVALID_ARG, "the chroma planes differ in size");
        }
    if (flow_h < 1 || flow_w < 1 || (size_t)flow_h > kFlowMaxSide || (size_t)flow_w > kFlowMaxSide)
        return fail(FIUNET_ERR_INVALID_ARG, "bad flow shape");
    if ((uintptr_t)flow & 7) return fail(FIUNET_ERR_INVALID_ARG, "flow not 8-B aligned");
    const int h = ap->h, w = ap->w;
    // the last chroma sample's luma position lies inside the flow's plane, so its block lies inside the pick map
    if ((int64_t)(h - 1) * sy >= flow_h || (int64_t)(w - 1) * sx >= flow_w)
        return fail(FIUNET_ERR_INVALID_ARG, "a chroma plane of this size and sub-sampling reaches past the luma plane");
    if (n == 0) return FIUNET_OK;
    const int ph = (flow_h + CHROMA_BLOCK - 1) / CHROMA_BLOCK, pw = (flow_w + CHROMA_BLOCK - 1) / CHROMA_BLOCK;
    uintptr_t o0[2], o1[2];
    for (int i = 0; i < 2; ++i)
        if (!plane_range(out, sizeof(T), op[i], n, &o0[i], &o1[i])) return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
    // U and V of a frame usually share a frame stride and lie side by side inside it: then one frame's two planes must
    // not overlap (each lies inside the stride, so frames do not meet); with two strides the whole ranges must not
    const int nuv = op[0].frame_stride == op[1].frame_stride ? 1 : n;   // (n frames fit: so do nuv)
    uintptr_t u0, u1, v0, v1;
    plane_range(out, sizeof(T), op[0], nuv, &u0, &u1), plane_range(out, sizeof(T), op[1], nuv, &v0, &v1);
    if (ranges_overlap(u0, u1, v0, v1) && (op[0].step == 1 || op[1].step == 1))
        return fail(FIUNET_ERR_INVALID_ARG, "out's two planes overlap");
    for (int i = 0; i < 4; ++i) {   // A's two planes, then B's, against out's two
        const bool is_b = i >= 2;
        uintptr_t p0, p1;
        if (!plane_range(is_b ? b : a, sizeof(T), (is_b ? bp : ap)[i & 1], n, &p0, &p1))
            return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
        for (int j = 0; j < 2; ++j)
            if (ranges_overlap(p0, p1, o0[j], o1[j])) return fail(FIUNET_ERR_INVALID_ARG, is_b ? "out overlaps B" : "out overlaps A");
    }
    ChromaPlanes P;
    for (int i = 0; i < 2; ++i) {
        P.a[i] = warp_plane(ap[i]);
        P.b[i] = warp_plane(bp[i]);
        P.o[i] = warp_plane(op[i]);
    }
    const float mx = (float)((double)w / (double)flow_w), my = (float)((double)h / (double)flow_h);
    constexpr int V = FlowWarpVec<T>::V;
    const dim3 grid((unsigned)(((w + V - 1) / V + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)(2 * n));
    hipLaunchKernelGGL(chroma_fill_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, a, b, P, flow, flow_h, flow_w, mx, my,
                       pick, ph, pw, sy, sx, h, w, out);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}
}  // namespace
}  // extern "C++"

int fiunet_chroma_pick_u8(const uint8_t* a, const fiunet_resize_plane* a_plane, const uint8_t* b,
                          const fiunet_resize_plane* b_plane, const uint8_t* m, const fiunet_resize_plane* m_plane,
                          const float* field, int n, uint8_t* pick, void* stream)
{
    return chroma_pick(a, a_plane, b, b_plane, m, m_plane, field, n, pick, stream);
}

int fiunet_chroma_pick_p10(const uint16_t* a, const fiunet_resize_plane* a_plane, const uint16_t* b,
                           const fiunet_resize_plane* b_plane, const uint16_t* m, const fiunet_resize_plane* m_plane,
                           const float* field, int n, uint8_t* pick, void* stream)
{
    return chroma_pick(a, a_plane, b, b_plane, m, m_plane, field, n, pick, stream);
}

int fiunet_chroma_fill_u8(const uint8_t* a, const fiunet_resize_plane* a_planes, const uint8_t* b,
                          const fiunet_resize_plane* b_planes, const float* field, int field_h, int field_w,
                          const uint8_t* pick, int sy, int sx, int n, uint8_t* out, const fiunet_resize_plane* out_planes,
                          void* stream)
{
    return chroma_fill(a, a_planes, b, b_planes, field, field_h, field_w, pick, sy, sx, n, out, out_planes, stream);
}

int fiunet_chroma_fill_p10(const uint16_t* a, const fiunet_resize_plane* a_planes, const uint16_t* b,
                           const fiunet_resize_plane* b_planes, const float* field, int field_h, int field_w,
                           const uint8_t* pick, int sy, int sx, int n, uint16_t* out,
                           const fiunet_resize_plane* out_planes, void* stream)
{
    return chroma_fill(a, a_planes, b, b_planes, field, field_h, field_w, pick, sy, sx, n, out, out_planes, stream);
}

// Diagnostic (tests; not part of the ABI): the pyramid of an H x W frame, pure host arithmetic.  dims[k] = {h, w,
// ksize}, sigma[k] for k = 0..*levels.
int fiunet_debug_flow_plan(int H, int W, int* levels, int dims[12], double sigma[4])
{
    if (H < 1 || W < 1 || !levels || !dims || !sigma) return fail(FIUNET_ERR_INVALID_ARG, "bad arguments");
    FlowLevel lv[kFlowLevels + 1];
    *levels = flow_levels(H, W, lv);
    for (int k = 0; k <= *levels; ++k) {
        dims[3 * k] = lv[k].h; dims[3 * k + 1] = lv[k].w; dims[3 * k + 2] = lv[k].ksize;
        sigma[k] = lv[k].sigma;
    }
    return FIUNET_OK;
}

// Diagnostic (tests; not part of the ABI): one stage of fiunet_farneback_flow on the caller's buffers, B pairs.
//   1 pyramid level `level` of B frames (in0: samples of `bits` with image_stride / row_pitch, H x W; scratch: fp32
//     [B, H, W]; out: fp32 [B, h, w], h x w the level's size)       2 polynomial expansion (in0 [B, h, w] -> [B, 5, h, w])
//   3 update matrices (in0 R0, in1 R1 [B, 5, h, w], in2 flow [B, 2, h, w] -> [B, 5, h, w])
//   4 box mean and solve (in0 [B, 5, h, w] -> flow [B, 2, h, w])    5 flow resize (in0 [B, 2, H, W] -> [B, 2, h, w] times
//     (mul0, mul1))
int fiunet_debug_flow_stage(int stage, const void* in0, const void* in1, const void* in2, void* out, void* scratch,
                            int bits, int level, int B, int H, int W, int h, int w, size_t image_stride,
                            size_t row_pitch, float mul0, float mul1, void* stream)
{
    if (!in0 || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (B < 1 || (size_t)B > kFlowMaxBatch || h < 1 || w < 1 || (size_t)h > kFlowMaxSide || (size_t)w > kFlowMaxSide)
        return fail(FIUNET_ERR_INVALID_ARG, "bad shape");
    hipStream_t s = (hipStream_t)stream;
    switch (stage) {
    case 1: {
        if (!scratch) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
        if (int rc = flow_check_frames(bits, B, H, W, image_stride, row_pitch, in0, in0)) return rc;
        FlowLevel lv[kFlowLevels + 1];
        const int levels = flow_levels(H, W, lv);
        if (level < 0 || level > levels || lv[level].h != h || lv[level].w != w)
            return fail(FIUNET_ERR_INVALID_ARG, "not a level of this frame size");
        const FlowBlurTaps taps = flow_blur_taps(lv[level].ksize, lv[level].sigma, H, W);
        if (int rc = flow_launch_blur(in0, bits, image_stride, row_pitch, B, H, W, taps, (float*)scratch, s)) return rc;
        return flow_launch_resize((const float*)scratch, H, W, (float*)out, h, w, B, 1, 1.0f, 1.0f, s);
    }
    case 2: return flow_launch_polyexp((const float*)in0, h, w, B, flow_poly_taps(), (float*)out, s);
    case 3:
        if (!in1 || !in2) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
        return flow_launch_matrices((const float*)in0, (const float*)in1, (const float*)in2, h, w, B, (float*)out, s);
    case 4: return flow_launch_boxsolve((const float*)in0, h, w, B, (float*)out, false, s);
    case 5:
        if (H < 1 || W < 1 || (size_t)H > kFlowMaxSide || (size_t)W > kFlowMaxSide) return fail(FIUNET_ERR_INVALID_ARG, "bad shape");
        return flow_launch_resize((const float*)in0, H, W, (float*)out, h, w, B, 2, mul0, mul1, s);
    }
    return fail(FIUNET_ERR_INVALID_ARG, "stage must be 1..5");
}

}  // extern "C"
