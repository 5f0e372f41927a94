// formats.hip -- the frame formats that go through the RGB network as staged planar RGB: packed I420
// at 8 and 10 bits, NV12 / P010 surfaces, YUV 4:2:2 / 4:4:4 and packed RGB - their conversions (colour.hip.h, yuv4xx.hip.h,
// packed.hip.h) and the fiunet_forward_<format> entry points around fiunet_forward_u8_strided / fiunet_forward_p10.
#include "fiunet_internal.h"
#include "plane_check.h"
#include "colour.hip.h"
#include "packed.hip.h"
#include "wire10.hip.h"
#include "yuv4xx.hip.h"

using namespace fiunet;

namespace {

// One of a format conversion's two instantiations on blocks of kColourBlock threads: the one with vector accesses where
// `vec` says that every base, pitch and stride allows them, the scalar one otherwise.
template <auto VecKernel, auto ScalarKernel, typename... Args>
int launch_vec(bool vec, dim3 grid, void* stream, Args... args)
{
    if (vec) hipLaunchKernelGGL(VecKernel, grid, dim3(kColourBlock), 0, (hipStream_t)stream, args...);
    else hipLaunchKernelGGL(ScalarKernel, grid, dim3(kColourBlock), 0, (hipStream_t)stream, args...);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

}  // namespace

extern "C" {

// ---- colour video (csrc/colour.hip.h): packed I420 <-> planar RGB, and the RGB network's forward between them ----
static inline size_t i420_frame_bytes(int H, int W)   // (samples per frame, at either depth)
{
    return (size_t)H * W + 2 * (size_t)((H + 1) / 2) * ((W + 1) / 2);
}

// `colour` at an entry point of `bits` bits: FIUNET_YUV_BT2020 is a 10-bit flag, and excludes FIUNET_YUV_BT709
static int check_colour_flags(unsigned colour, int bits)
{
    if (colour & ~(bits == 10 ? kColourFlagsP10 : kColourFlags))
        return fail(FIUNET_ERR_INVALID_ARG, "colour: unknown flag bits (FIUNET_YUV_BT2020 needs the 10-bit entry points)");
    if ((colour & FIUNET_YUV_BT709) && (colour & FIUNET_YUV_BT2020))
        return fail(FIUNET_ERR_INVALID_ARG, "colour: FIUNET_YUV_BT709 and FIUNET_YUV_BT2020 together");
    return FIUNET_OK;
}

static int check_colour_args(const void* in, const void* out, int B, int H, int W, unsigned colour, int bits)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_colour_flags(colour, bits)) return rc;
    if (const char* why = check_frame_shape(B, H, W)) return fail(FIUNET_ERR_BAD_SHAPE, why);
    return FIUNET_OK;
}

// the conversions' grid: a thread per four columns, `rows` rows (a chroma row covers two luma rows), B frames
static dim3 colour_grid(int W, int rows, int B)
{
    return dim3((unsigned)(((W + 3) / 4 + kColourBlock - 1) / kColourBlock), (unsigned)rows, (unsigned)B);
}

extern "C++" {   // (templates over the sample type, inside this file's extern "C" part)
// the caller's frame stride (0 = tight) -> the resolved one, refused where a frame does not fit; `which`: "in" / "out"
static int resolve_i420_stride(size_t* frame_stride, int H, int W, const char* which)
{
    const size_t fs = i420_frame_bytes(H, W);
    if (*frame_stride == 0) *frame_stride = fs;
    if (*frame_stride < fs) return fail(FIUNET_ERR_INVALID_ARG, std::string(which) + "_frame_stride smaller than one frame");
    return FIUNET_OK;
}

// one 4-sample access per luma quad and per chroma pair: W, the stride and both bases a multiple of 4 samples
template <typename T>
static bool i420_vec(int W, size_t frame_stride, const void* a, const void* b)
{
    return W % 4 == 0 && frame_stride % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & (4 * sizeof(T) - 1)) == 0;
}

template <typename T>
static int yuv420_to_rgb(const T* in, size_t in_frame_stride, T* out, int B, int H, int W, unsigned colour, int bits,
                         void* stream)
{
    int rc;
    if ((rc = check_colour_args(in, out, B, H, W, colour, bits))) return rc;
    if ((rc = resolve_i420_stride(&in_frame_stride, H, W, "in"))) return rc;
    return launch_vec<&yuv420_to_rgb_kernel<T, true>, &yuv420_to_rgb_kernel<T, false>>(
        i420_vec<T>(W, in_frame_stride, in, out), colour_grid(W, H, B), stream, in, in_frame_stride, out, H, W,
        colour_coef(colour, bits));
}

template <typename T>
static int rgb_to_yuv420(const T* in, T* out, size_t out_frame_stride, int B, int H, int W, unsigned colour, int bits,
                         void* stream)
{
    int rc;
    if ((rc = check_colour_args(in, out, B, H, W, colour, bits))) return rc;
    if ((rc = resolve_i420_stride(&out_frame_stride, H, W, "out"))) return rc;
    return launch_vec<&rgb_to_yuv420_kernel<T, true>, &rgb_to_yuv420_kernel<T, false>>(
        i420_vec<T>(W, out_frame_stride, in, out), colour_grid(W, (H + 1) / 2, B), stream, in, out, out_frame_stride, H, W,
        colour_coef(colour, bits));
}
}  // extern "C++"

int fiunet_yuv420_to_rgb_u8(const uint8_t* in, size_t in_frame_stride, uint8_t* out, int B, int H, int W,
                            unsigned colour, void* stream)
{
    return yuv420_to_rgb<uint8_t>(in, in_frame_stride, out, B, H, W, colour, 8, stream);
}

int fiunet_rgb_to_yuv420_u8(const uint8_t* in, uint8_t* out, size_t out_frame_stride, int B, int H, int W,
                            unsigned colour, void* stream)
{
    return rgb_to_yuv420<uint8_t>(in, out, out_frame_stride, B, H, W, colour, 8, stream);
}

int fiunet_yuv420p10_to_rgb_p10(const uint16_t* in, size_t in_frame_stride, uint16_t* out, int B, int H, int W,
                                unsigned colour, void* stream)
{
    return yuv420_to_rgb<uint16_t>(in, in_frame_stride, out, B, H, W, colour, 10, stream);
}

int fiunet_rgb_p10_to_yuv420p10(const uint16_t* in, uint16_t* out, size_t out_frame_stride, int B, int H, int W,
                                unsigned colour, void* stream)
{
    return rgb_to_yuv420<uint16_t>(in, out, out_frame_stride, B, H, W, colour, 10, stream);
}

// ---- the staged-RGB forward: how a frame format goes through the RGB network.  Every
//      fiunet_forward_<format> below is this chain with its own conversion pair; nothing else differs between them.
// [the inner forward's workspace | frame1 RGB | frame2 RGB | output RGB]: planar [B, 3, H, W] batches of `sample`-byte
// samples behind the workspace of fiunet_forward_u8 (1 byte) / fiunet_forward_p10 (2), every part rounded up to 256 B.
struct StagedWorkspace {
    size_t inner, rgb, total;   // total 0: bad arguments (the inner query has said which)
};

static StagedWorkspace staged_workspace(const fiunet_ctx* ctx, int B, int H, int W, int precision, size_t sample)
{
    const size_t inner = sample == 1 ? fiunet_workspace_bytes_u8(ctx, B, H, W, precision)
                                     : fiunet_workspace_bytes_p10(ctx, B, H, W, precision);
    if (inner == 0) return {0, 0, 0};
    const size_t base = align256(inner), rgb = align256((size_t)B * 3 * H * W * sample);
    return {base, rgb, base + 3 * rgb};
}

extern "C++" {
// T: uint8_t (through fiunet_forward_u8_strided) or uint16_t (through fiunet_forward_p10).  What a format supplies:
//   check()           host only: its format code, colour flags and both layouts (anything its conversions would refuse);
//   to_rgb(in, rgb)   its frames -> a planar RGB batch;
//   from_rgb(rgb)     a planar RGB batch -> `out` in its format.
// Every refusal comes before the first launch.  `name`: the entry point, for the wrong-network message.
template <typename T, typename Check, typename ToRgb, typename FromRgb>
static int forward_staged(const char* name, fiunet_ctx* ctx, const T* frame1, const T* frame2, const T* out, int B,
                          int H, int W, int precision, void* workspace, size_t workspace_bytes, void* stream,
                          Check check, ToRgb to_rgb, FromRgb from_rgb)
{
    if (!frame1 || !frame2 || !out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (H < 16 || W < 16) return fail(FIUNET_ERR_BAD_SHAPE, "H and W must be >= 16 (four 2x2 max-pools)");
    int rc;
    if ((rc = check())) return rc;
    if (!ctx) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (ctx->cf != 3)
        return fail(FIUNET_ERR_UNSUPPORTED, std::string(name) + " needs the RGB network (frame_channels 3)");
    if (!ctx->loaded) return fail(FIUNET_ERR_NOT_LOADED, "fiunet_forward before fiunet_load_weights");
    const StagedWorkspace ws = staged_workspace(ctx, B, H, W, precision, sizeof(T));
    if (ws.total == 0) return fail(FIUNET_ERR_INVALID_ARG, "bad precision or shape");
    if (workspace_bytes < ws.total) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    T* a = (T*)((char*)workspace + ws.inner);
    T* b = (T*)((char*)a + ws.rgb);
    T* o = (T*)((char*)b + ws.rgb);
    if ((rc = to_rgb(frame1, a)) || (rc = to_rgb(frame2, b))) return rc;
    if constexpr (sizeof(T) == 1)
        rc = fiunet_forward_u8_strided(ctx, a, b, o, 0, B, H, W, precision, workspace, ws.inner, stream);
    else
        rc = fiunet_forward_p10(ctx, a, b, o, 0, B, H, W, precision, workspace, ws.inner, stream);
    return rc ? rc : from_rgb(o);
}

template <typename T>
static int forward_yuv420(const char* name, int bits, fiunet_ctx* ctx, const T* frame1, const T* frame2, T* out,
                          size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision, void* workspace,
                          size_t workspace_bytes, void* stream)
{
    return forward_staged<T>(
        name, ctx, frame1, frame2, out, B, H, W, precision, workspace, workspace_bytes, stream,
        [&] {
            const int rc = check_colour_flags(colour, bits);
            return rc ? rc : resolve_i420_stride(&out_frame_stride, H, W, "out");
        },
        [&](const T* in, T* rgb) { return yuv420_to_rgb<T>(in, 0, rgb, B, H, W, colour, bits, stream); },
        [&](const T* rgb) { return rgb_to_yuv420<T>(rgb, out, out_frame_stride, B, H, W, colour, bits, stream); });
}
}  // extern "C++"

size_t fiunet_workspace_bytes_yuv420(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    return staged_workspace(ctx, B, H, W, precision, 1).total;
}

size_t fiunet_workspace_bytes_yuv420p10(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    return staged_workspace(ctx, B, H, W, precision, 2).total;
}

int fiunet_forward_yuv420(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, uint8_t* out,
                          size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision,
                          void* workspace, size_t workspace_bytes, void* stream)
{
    return forward_yuv420<uint8_t>("fiunet_forward_yuv420", 8, ctx, frame1, frame2, out, out_frame_stride, B, H, W, colour,
                                   precision, workspace, workspace_bytes, stream);
}

int fiunet_forward_yuv420p10(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, uint16_t* out,
                             size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    return forward_yuv420<uint16_t>("fiunet_forward_yuv420p10", 10, ctx, frame1, frame2, out, out_frame_stride, B, H, W,
                                    colour, precision, workspace, workspace_bytes, stream);
}

// ---- NV12 / P010 decoder surfaces: the colour conversions on semi-planar, pitched frames ----
// The caller's layout -> the resolved one (plane_check.h: resolve_surface, the chroma plane ceil(H/2) rows high), refused
// before any launch.  Every quantity in samples.
static int resolve_nv12(const fiunet_surface_layout* l, int H, int W, ColourSurface* sf)
{
    fiunet_surface_layout r;
    if (const char* why = resolve_surface(l, H, W, ((size_t)H + 1) / 2, &r)) return fail(FIUNET_ERR_INVALID_ARG, why);
    *sf = ColourSurface{r.luma_pitch, r.chroma_offset, r.chroma_pitch, r.frame_stride};
    return FIUNET_OK;
}

extern "C++" {   // (templates over the sample type, inside this file's extern "C" part)
// one 4-sample access per luma quad and per pair of owned chroma pairs: everything a multiple of 4 samples
template <typename T>
static bool surface_vec(const ColourSurface& sf, int W, const void* a, const void* b)
{
    return W % 4 == 0 && (sf.luma_pitch | sf.chroma_offset | sf.chroma_pitch | sf.frame_stride) % 4 == 0 &&
           (((uintptr_t)a | (uintptr_t)b) & (4 * sizeof(T) - 1)) == 0;
}

template <typename T>
static int surface_to_rgb(const T* in, const fiunet_surface_layout* layout, T* out, int B, int H, int W,
                          unsigned colour, int bits, void* stream)
{
    int rc;
    if ((rc = check_colour_args(in, out, B, H, W, colour, bits))) return rc;
    ColourSurface sf;
    if ((rc = resolve_nv12(layout, H, W, &sf))) return rc;
    return launch_vec<&nv12_to_rgb_kernel<T, true>, &nv12_to_rgb_kernel<T, false>>(
        surface_vec<T>(sf, W, in, out), colour_grid(W, H, B), stream, in, sf, out, H, W, colour_coef(colour, bits));
}

template <typename T>
static int rgb_to_surface(const T* in, T* out, const fiunet_surface_layout* layout, int B, int H, int W,
                          unsigned colour, int bits, void* stream)
{
    int rc;
    if ((rc = check_colour_args(in, out, B, H, W, colour, bits))) return rc;
    ColourSurface sf;
    if ((rc = resolve_nv12(layout, H, W, &sf))) return rc;
    return launch_vec<&rgb_to_nv12_kernel<T, true>, &rgb_to_nv12_kernel<T, false>>(
        surface_vec<T>(sf, W, in, out), colour_grid(W, (H + 1) / 2, B), stream, in, out, sf, H, W,
        colour_coef(colour, bits));
}

template <typename T>
static int forward_surface(const char* name, int bits, fiunet_ctx* ctx, const T* frame1, const T* frame2,
                           const fiunet_surface_layout* in_layout, T* out, const fiunet_surface_layout* out_layout, int B,
                           int H, int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes,
                           void* stream)
{
    return forward_staged<T>(
        name, ctx, frame1, frame2, out, B, H, W, precision, workspace, workspace_bytes, stream,
        [&] {
            ColourSurface sf;
            int rc = check_colour_flags(colour, bits);
            if (!rc && !(rc = resolve_nv12(in_layout, H, W, &sf))) rc = resolve_nv12(out_layout, H, W, &sf);
            return rc;
        },
        [&](const T* in, T* rgb) { return surface_to_rgb<T>(in, in_layout, rgb, B, H, W, colour, bits, stream); },
        [&](const T* rgb) { return rgb_to_surface<T>(rgb, out, out_layout, B, H, W, colour, bits, stream); });
}
}  // extern "C++"

int fiunet_nv12_to_rgb_u8(const uint8_t* in, const fiunet_surface_layout* in_layout, uint8_t* out, int B, int H, int W,
                          unsigned colour, void* stream)
{
    return surface_to_rgb<uint8_t>(in, in_layout, out, B, H, W, colour, 8, stream);
}

int fiunet_rgb_to_nv12_u8(const uint8_t* in, uint8_t* out, const fiunet_surface_layout* out_layout, int B, int H, int W,
                          unsigned colour, void* stream)
{
    return rgb_to_surface<uint8_t>(in, out, out_layout, B, H, W, colour, 8, stream);
}

int fiunet_p010_to_rgb_p10(const uint16_t* in, const fiunet_surface_layout* in_layout, uint16_t* out, int B, int H,
                           int W, unsigned colour, void* stream)
{
    return surface_to_rgb<uint16_t>(in, in_layout, out, B, H, W, colour, 10, stream);
}

int fiunet_rgb_p10_to_p010(const uint16_t* in, uint16_t* out, const fiunet_surface_layout* out_layout, int B, int H,
                           int W, unsigned colour, void* stream)
{
    return rgb_to_surface<uint16_t>(in, out, out_layout, B, H, W, colour, 10, stream);
}

size_t fiunet_workspace_bytes_nv12(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    return staged_workspace(ctx, B, H, W, precision, 1).total;
}

size_t fiunet_workspace_bytes_p010(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    return staged_workspace(ctx, B, H, W, precision, 2).total;
}

int fiunet_forward_nv12(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2,
                        const fiunet_surface_layout* in_layout, uint8_t* out, const fiunet_surface_layout* out_layout,
                        int B, int H, int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes,
                        void* stream)
{
    return forward_surface<uint8_t>("fiunet_forward_nv12", 8, ctx, frame1, frame2, in_layout, out, out_layout, B, H, W,
                                    colour, precision, workspace, workspace_bytes, stream);
}

int fiunet_forward_p010(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2,
                        const fiunet_surface_layout* in_layout, uint16_t* out, const fiunet_surface_layout* out_layout,
                        int B, int H, int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes,
                        void* stream)
{
    return forward_surface<uint16_t>("fiunet_forward_p010", 10, ctx, frame1, frame2, in_layout, out, out_layout, B, H, W,
                                     colour, precision, workspace, workspace_bytes, stream);
}

// ---- YUV 4:2:2 / 4:4:4 frames (csrc/yuv4xx.hip.h): planar and one-plane packed, <-> planar RGB ----
// samples of one tight frame of `format` (bytes at 8 bits); 0: not a fiunet_yuv_format
static size_t yuv_frame_samples(int format, int H, int W)
{
    switch (format) {
    case FIUNET_YUV_422P: return (size_t)H * W + 2 * (size_t)H * ((W + 1) / 2);
    case FIUNET_YUV_444P: return 3 * (size_t)H * W;
    case FIUNET_YUV_UYVY422:
    case FIUNET_YUV_YUYV422: return 2 * (size_t)H * W;
    default: return 0;
    }
}

// The caller's pitch and stride (0 = tight) -> the resolved layout, with every refusal that needs no pointer: before
// any launch.  bits: the entry point's sample depth.
static int resolve_yuv(int format, int bits, size_t row_pitch, size_t frame_stride, int B, int H, int W, unsigned colour,
                       YuvLayout* lay)
{
    if (int rc = check_colour_flags(colour, bits)) return rc;
    if (const char* why = check_frame_shape(B, H, W)) return fail(FIUNET_ERR_BAD_SHAPE, why);
    const size_t tight = yuv_frame_samples(format, H, W);
    if (!tight) return fail(FIUNET_ERR_INVALID_ARG, "format: not a fiunet_yuv_format");
    if (row_pitch > kLayoutMax || frame_stride > kLayoutMax) return fail(FIUNET_ERR_INVALID_ARG, "yuv layout: a value above 2^40");
    if (yuv_is_packed(format)) {
        if (bits != 8) return fail(FIUNET_ERR_INVALID_ARG, "format: uyvy422 / yuyv422 are 8-bit formats");
        if (W & 1) return fail(FIUNET_ERR_INVALID_ARG, "uyvy422 / yuyv422 need an even width");
        const fiunet_packed_layout l = {row_pitch, frame_stride};   // (one plane of rows of 2 * W bytes)
        fiunet_packed_layout r;
        if (const char* why = resolve_rows(&l, H, 2 * (size_t)W, &r)) return fail(FIUNET_ERR_INVALID_ARG, why);
        *lay = YuvLayout{r.row_pitch, r.frame_stride};
        return FIUNET_OK;
    }
    if (row_pitch) return fail(FIUNET_ERR_INVALID_ARG, "yuv layout: planar frames are tight (row_pitch must be 0)");
    lay->row_pitch = 0;
    lay->frame_stride = frame_stride ? frame_stride : tight;
    if (lay->frame_stride < tight) return fail(FIUNET_ERR_INVALID_ARG, "yuv layout: frame_stride smaller than one frame");
    return FIUNET_OK;
}

extern "C++" {   // (templates over the sample type, inside this file's extern "C" part)
// vector accesses: W and every pitch and stride a multiple of 4 samples, bases aligned to 4 samples
template <typename T>
static bool yuv_vec(const YuvLayout& lay, int W, const void* a, const void* b)
{
    return W % 4 == 0 && (lay.row_pitch | lay.frame_stride) % 4 == 0 &&
           (((uintptr_t)a | (uintptr_t)b) & (4 * sizeof(T) - 1)) == 0;
}

template <int F>
using YuvFormat = std::integral_constant<int, F>;

// go(YuvFormat<F>{}) for the resolved `format` (the one-plane formats exist at 8 bits only: resolve_yuv has refused them
// at 10, and their uint16 kernels are never instantiated)
template <typename T, typename Go>
static int for_yuv_format(int format, Go go)
{
    if (format == FIUNET_YUV_422P) return go(YuvFormat<FIUNET_YUV_422P>{});
    if (format == FIUNET_YUV_444P) return go(YuvFormat<FIUNET_YUV_444P>{});
    if constexpr (sizeof(T) == 1)
        return format == FIUNET_YUV_UYVY422 ? go(YuvFormat<FIUNET_YUV_UYVY422>{}) : go(YuvFormat<FIUNET_YUV_YUYV422>{});
    return FIUNET_OK;
}

template <typename T>
static int yuv_to_rgb(const T* in, int format, size_t row_pitch, size_t frame_stride, T* out, int B, int H, int W,
                      unsigned colour, int bits, void* stream)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    YuvLayout lay;
    if (int rc = resolve_yuv(format, bits, row_pitch, frame_stride, B, H, W, colour, &lay)) return rc;
    return for_yuv_format<T>(format, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return launch_vec<&yuv_to_rgb_kernel<T, F, true>, &yuv_to_rgb_kernel<T, F, false>>(
            yuv_vec<T>(lay, W, in, out), colour_grid(W, H, B), stream, in, lay, out, H, W, colour_coef(colour, bits));
    });
}

template <typename T>
static int rgb_to_yuv(const T* in, T* out, int format, size_t row_pitch, size_t frame_stride, int B, int H, int W,
                      unsigned colour, int bits, void* stream)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    YuvLayout lay;
    if (int rc = resolve_yuv(format, bits, row_pitch, frame_stride, B, H, W, colour, &lay)) return rc;
    return for_yuv_format<T>(format, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return launch_vec<&rgb_to_yuv_kernel<T, F, true>, &rgb_to_yuv_kernel<T, F, false>>(
            yuv_vec<T>(lay, W, in, out), colour_grid(W, H, B), stream, in, out, lay, H, W, colour_coef(colour, bits));
    });
}

template <typename T>
static int forward_yuv(const char* name, int bits, fiunet_ctx* ctx, const T* frame1, const T* frame2, int format,
                       size_t in_row_pitch, size_t in_frame_stride, T* out, size_t out_row_pitch, size_t out_frame_stride,
                       int B, int H, int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes,
                       void* stream)
{
    return forward_staged<T>(
        name, ctx, frame1, frame2, out, B, H, W, precision, workspace, workspace_bytes, stream,
        [&] {
            YuvLayout lay;
            const int rc = resolve_yuv(format, bits, in_row_pitch, in_frame_stride, B, H, W, colour, &lay);
            return rc ? rc : resolve_yuv(format, bits, out_row_pitch, out_frame_stride, B, H, W, colour, &lay);
        },
        [&](const T* in, T* rgb) {
            return yuv_to_rgb<T>(in, format, in_row_pitch, in_frame_stride, rgb, B, H, W, colour, bits, stream);
        },
        [&](const T* rgb) {
            return rgb_to_yuv<T>(rgb, out, format, out_row_pitch, out_frame_stride, B, H, W, colour, bits, stream);
        });
}
}  // extern "C++"

int fiunet_yuv_to_rgb_u8(const uint8_t* in, int format, size_t row_pitch, size_t frame_stride, uint8_t* out, int B,
                         int H, int W, unsigned colour, void* stream)
{
    return yuv_to_rgb<uint8_t>(in, format, row_pitch, frame_stride, out, B, H, W, colour, 8, stream);
}

int fiunet_rgb_to_yuv_u8(const uint8_t* in, uint8_t* out, int format, size_t row_pitch, size_t frame_stride, int B,
                         int H, int W, unsigned colour, void* stream)
{
    return rgb_to_yuv<uint8_t>(in, out, format, row_pitch, frame_stride, B, H, W, colour, 8, stream);
}

int fiunet_yuv_to_rgb_p10(const uint16_t* in, int format, size_t row_pitch, size_t frame_stride, uint16_t* out, int B,
                          int H, int W, unsigned colour, void* stream)
{
    return yuv_to_rgb<uint16_t>(in, format, row_pitch, frame_stride, out, B, H, W, colour, 10, stream);
}

int fiunet_rgb_p10_to_yuv(const uint16_t* in, uint16_t* out, int format, size_t row_pitch, size_t frame_stride, int B,
                          int H, int W, unsigned colour, void* stream)
{
    return rgb_to_yuv<uint16_t>(in, out, format, row_pitch, frame_stride, B, H, W, colour, 10, stream);
}

size_t fiunet_workspace_bytes_yuv(const fiunet_ctx* ctx, int B, int H, int W, int precision, int bits)
{
    if (bits == 8 || bits == 10) return staged_workspace(ctx, B, H, W, precision, bits == 8 ? 1 : 2).total;
    last_error() = "fiunet_workspace_bytes_yuv: bits must be 8 or 10";
    return 0;
}

int fiunet_forward_yuv(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, int format, size_t in_row_pitch,
                       size_t in_frame_stride, uint8_t* out, size_t out_row_pitch, size_t out_frame_stride, int B, int H,
                       int W, unsigned colour, int precision, void* workspace, size_t workspace_bytes, void* stream)
{
    return forward_yuv<uint8_t>("fiunet_forward_yuv", 8, ctx, frame1, frame2, format, in_row_pitch, in_frame_stride, out,
                                out_row_pitch, out_frame_stride, B, H, W, colour, precision, workspace, workspace_bytes,
                                stream);
}

int fiunet_forward_yuv_p10(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, int format,
                           size_t in_row_pitch, size_t in_frame_stride, uint16_t* out, size_t out_row_pitch,
                           size_t out_frame_stride, int B, int H, int W, unsigned colour, int precision, void* workspace,
                           size_t workspace_bytes, void* stream)
{
    return forward_yuv<uint16_t>("fiunet_forward_yuv_p10", 10, ctx, frame1, frame2, format, in_row_pitch, in_frame_stride,
                                 out, out_row_pitch, out_frame_stride, B, H, W, colour, precision, workspace,
                                 workspace_bytes, stream);
}

// ---- packed RGB frames: rgb24 / bgr24 / rgba / bgra, rows a pitch apart, <-> planar RGB ----
static int packed_bpp(int format)
{
    return format == FIUNET_PACKED_RGB24 || format == FIUNET_PACKED_BGR24 ? 3
         : format == FIUNET_PACKED_RGBA || format == FIUNET_PACKED_BGRA ? 4 : 0;
}

// The caller's layout -> the resolved one (plane_check.h: resolve_rows, rows of W * bpp bytes), refused before any launch.
static int resolve_packed(const fiunet_packed_layout* l, int H, int W, int bpp, PackedLayout* pl)
{
    fiunet_packed_layout r;
    if (const char* why = resolve_rows(l, H, (size_t)W * bpp, &r)) return fail(FIUNET_ERR_INVALID_ARG, why);
    *pl = PackedLayout{r.row_pitch, r.frame_stride};
    return FIUNET_OK;
}

static int check_packed_args(const void* in, const void* out, int B, int H, int W, int format)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!packed_bpp(format)) return fail(FIUNET_ERR_INVALID_ARG, "format: not a fiunet_packed_format");
    if (const char* why = check_frame_shape(B, H, W)) return fail(FIUNET_ERR_BAD_SHAPE, why);
    return FIUNET_OK;
}

// dword and 16-byte packed accesses, uchar4 plane accesses: W and every pitch, stride and base a multiple of 4 bytes
static bool packed_vec(int W, const PackedLayout& l, uintptr_t bases)
{
    return W % 4 == 0 && (l.row_pitch | l.frame_stride) % 4 == 0 && (bases & 3) == 0;
}

extern "C++" {
template <int BPP, bool SWAP>
struct PackedFormat {
    static constexpr int bpp = BPP;
    static constexpr bool swap = SWAP;
};

// go(PackedFormat<bpp, swap>{}) for a format that packed_bpp() knows
template <typename Go>
static int for_packed_format(int format, Go go)
{
    switch (format) {
    case FIUNET_PACKED_RGB24: return go(PackedFormat<3, false>{});
    case FIUNET_PACKED_BGR24: return go(PackedFormat<3, true>{});
    case FIUNET_PACKED_RGBA: return go(PackedFormat<4, false>{});
    default: return go(PackedFormat<4, true>{});
    }
}
}  // extern "C++"

int fiunet_packed_to_rgb_u8(const uint8_t* in, const fiunet_packed_layout* in_layout, uint8_t* out_rgb,
                            uint8_t* alpha_out, int B, int H, int W, int format, void* stream)
{
    int rc;
    if ((rc = check_packed_args(in, out_rgb, B, H, W, format))) return rc;
    const int bpp = packed_bpp(format);
    if (alpha_out && bpp != 4) return fail(FIUNET_ERR_INVALID_ARG, "alpha_out: the format has no alpha byte");
    PackedLayout li;
    if ((rc = resolve_packed(in_layout, H, W, bpp, &li))) return rc;
    const bool vec = packed_vec(W, li, (uintptr_t)in | (uintptr_t)out_rgb | (uintptr_t)alpha_out);
    return for_packed_format(format, [&](auto f) {
        using F = decltype(f);
        return launch_vec<&packed_to_rgb_kernel<F::bpp, F::swap, true>, &packed_to_rgb_kernel<F::bpp, F::swap, false>>(
            vec, colour_grid(W, H, B), stream, in, li, out_rgb, alpha_out, H, W);
    });
}

int fiunet_rgb_to_packed_u8(const uint8_t* in_rgb, uint8_t* out, const fiunet_packed_layout* out_layout,
                            const uint8_t* alpha1, const uint8_t* alpha2, const fiunet_packed_layout* alpha_layout,
                            int B, int H, int W, int format, void* stream)
{
    int rc;
    if ((rc = check_packed_args(in_rgb, out, B, H, W, format))) return rc;
    const int bpp = packed_bpp(format);
    if ((alpha1 || alpha2) && bpp != 4) return fail(FIUNET_ERR_INVALID_ARG, "alpha source: the format has no alpha byte");
    if (alpha2 && !alpha1) return fail(FIUNET_ERR_INVALID_ARG, "alpha2 without alpha1");
    PackedLayout lo, la;
    if ((rc = resolve_packed(out_layout, H, W, bpp, &lo))) return rc;
    if ((rc = resolve_packed(alpha_layout, H, W, bpp, &la))) return rc;
    const bool vec = packed_vec(W, lo, (uintptr_t)in_rgb | (uintptr_t)out | (uintptr_t)alpha1 | (uintptr_t)alpha2) &&
                     (!alpha1 || packed_vec(W, la, 0));
    return for_packed_format(format, [&](auto f) {
        using F = decltype(f);
        return launch_vec<&rgb_to_packed_kernel<F::bpp, F::swap, true>, &rgb_to_packed_kernel<F::bpp, F::swap, false>>(
            vec, colour_grid(W, H, B), stream, in_rgb, out, lo, alpha1, alpha2, la, H, W);
    });
}

size_t fiunet_workspace_bytes_rgb_packed(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    return staged_workspace(ctx, B, H, W, precision, 1).total;
}

int fiunet_forward_rgb_packed(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2,
                              const fiunet_packed_layout* in_layout, uint8_t* out, const fiunet_packed_layout* out_layout,
                              int B, int H, int W, int format, int precision, void* workspace, size_t workspace_bytes,
                              void* stream)
{
    const int bpp = packed_bpp(format);
    const bool alpha = bpp == 4;   // the inserted frame's alpha: the rounded average of its neighbours'
    return forward_staged<uint8_t>(
        "fiunet_forward_rgb_packed", ctx, frame1, frame2, out, B, H, W, precision, workspace, workspace_bytes, stream,
        [&] {
            if (!bpp) return fail(FIUNET_ERR_INVALID_ARG, "format: not a fiunet_packed_format");
            PackedLayout pl;
            const int rc = resolve_packed(in_layout, H, W, bpp, &pl);
            return rc ? rc : resolve_packed(out_layout, H, W, bpp, &pl);
        },
        [&](const uint8_t* in, uint8_t* rgb) { return fiunet_packed_to_rgb_u8(in, in_layout, rgb, NULL, B, H, W, format, stream); },
        [&](const uint8_t* rgb) {
            return fiunet_rgb_to_packed_u8(rgb, out, out_layout, alpha ? frame1 : NULL, alpha ? frame2 : NULL, in_layout, B,
                                           H, W, format, stream);
        });
}

// ---- 10-bit 4:2:2 wire packings (csrc/wire10.hip.h): v210 / y210le / p210le <-> yuv422p10le ----
// bytes of one tight row of a one-plane packing
static size_t wire10_row_bytes(int packing, int W)
{
    return packing == FIUNET_PACK10_V210 ? 128 * (size_t)((W + 47) / 48) : 4 * (size_t)W;
}

// The caller's layouts (NULL or zero fields = tight) and the working frames' stride (0 = tight) -> the resolved ones and
// whether the vector path applies, with every refusal: before any launch.  wire / work: the two base pointers.
static int resolve_wire10(const void* wire, int packing, const fiunet_packed_layout* pl, const fiunet_surface_layout* sl,
                          const void* work, size_t* work_stride, int B, int H, int W, Wire10Layout* lay, bool* vec)
{
    if (!wire || !work) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (packing != FIUNET_PACK10_V210 && packing != FIUNET_PACK10_Y210 && packing != FIUNET_PACK10_P210)
        return fail(FIUNET_ERR_INVALID_ARG, "packing: not a fiunet_packing10");
    if (const char* why = check_frame_shape(B, H, W)) return fail(FIUNET_ERR_BAD_SHAPE, why);
    if (((uintptr_t)wire | (uintptr_t)work) & 1) return fail(FIUNET_ERR_INVALID_ARG, "wire10: a pointer is not 2-byte aligned");
    const size_t Wc = (size_t)(W + 1) / 2, tight = (size_t)H * W + 2 * (size_t)H * Wc;
    if (*work_stride == 0) *work_stride = tight;
    if (*work_stride > kLayoutMax) return fail(FIUNET_ERR_INVALID_ARG, "wire10: a value above 2^40");
    if (*work_stride < tight) return fail(FIUNET_ERR_INVALID_ARG, "wire10: the planar frame stride is smaller than one frame");
    bool aligned = W % 8 == 0 && *work_stride % 8 == 0 && (((uintptr_t)wire | (uintptr_t)work) & 15) == 0;
    if (packing == FIUNET_PACK10_P210) {
        if (pl) return fail(FIUNET_ERR_INVALID_ARG, "p210le takes a fiunet_surface_layout, not a fiunet_packed_layout");
        fiunet_surface_layout r;
        if (const char* why = resolve_surface(sl, H, W, (size_t)H, &r)) return fail(FIUNET_ERR_INVALID_ARG, why);
        *lay = Wire10Layout{r.luma_pitch, r.chroma_offset, r.chroma_pitch, r.frame_stride};
        *vec = aligned && (lay->pitch | lay->chroma_offset | lay->chroma_pitch | lay->frame_stride) % 8 == 0;
        return FIUNET_OK;
    }
    if (sl) return fail(FIUNET_ERR_INVALID_ARG, "v210 / y210le take a fiunet_packed_layout, not a fiunet_surface_layout");
    if (W & 1) return fail(FIUNET_ERR_INVALID_ARG, "v210 / y210le need an even width");
    fiunet_packed_layout r;
    if (const char* why = resolve_rows(pl, H, wire10_row_bytes(packing, W), &r)) return fail(FIUNET_ERR_INVALID_ARG, why);
    *lay = Wire10Layout{r.row_pitch, 0, 0, r.frame_stride};
    if ((lay->pitch | lay->frame_stride) & 1)
        return fail(FIUNET_ERR_INVALID_ARG, "packed layout: row_pitch and frame_stride must be even (16-bit words)");
    *vec = aligned && (lay->pitch | lay->frame_stride) % 16 == 0;
    return FIUNET_OK;
}

extern "C++" {
template <int P>
using Packing10 = std::integral_constant<int, P>;

// go(Packing10<P>{}) for a packing that resolve_wire10 has accepted
template <typename Go>
static int for_packing10(int packing, Go go)
{
    switch (packing) {
    case FIUNET_PACK10_V210: return go(Packing10<FIUNET_PACK10_V210>{});
    case FIUNET_PACK10_Y210: return go(Packing10<FIUNET_PACK10_Y210>{});
    default: return go(Packing10<FIUNET_PACK10_P210>{});
    }
}
}  // extern "C++"

static dim3 wire10_grid(int packing, bool vec, int W, int H, int B)
{
    return dim3((unsigned)wire10_blocks(packing, vec, W), (unsigned)H, (unsigned)B);
}

int fiunet_unpack_422p10(const void* in, int packing, const fiunet_packed_layout* in_packed,
                         const fiunet_surface_layout* in_surface, uint16_t* out, size_t out_frame_stride, int B, int H,
                         int W, void* stream)
{
    Wire10Layout lay;
    bool vec;
    if (int rc = resolve_wire10(in, packing, in_packed, in_surface, out, &out_frame_stride, B, H, W, &lay, &vec)) return rc;
    return for_packing10(packing, [&](auto p) {
        constexpr int P = decltype(p)::value;
        return launch_vec<&unpack_422p10_kernel<P, true>, &unpack_422p10_kernel<P, false>>(
            vec, wire10_grid(packing, vec, W, H, B), stream, (const uint16_t*)in, lay, out, out_frame_stride, H, W);
    });
}

int fiunet_pack_422p10(const uint16_t* in, size_t in_frame_stride, void* out, int packing,
                       const fiunet_packed_layout* out_packed, const fiunet_surface_layout* out_surface, int B, int H,
                       int W, void* stream)
{
    Wire10Layout lay;
    bool vec;
    if (int rc = resolve_wire10(out, packing, out_packed, out_surface, in, &in_frame_stride, B, H, W, &lay, &vec)) return rc;
    return for_packing10(packing, [&](auto p) {
        constexpr int P = decltype(p)::value;
        return launch_vec<&pack_422p10_kernel<P, true>, &pack_422p10_kernel<P, false>>(
            vec, wire10_grid(packing, vec, W, H, B), stream, in, in_frame_stride, (uint16_t*)out, lay, H, W);
    });
}

}  // extern "C"
