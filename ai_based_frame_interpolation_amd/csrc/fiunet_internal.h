// fiunet_internal.h -- what the translation units of libfiunet_hip.so share (not installed; the C ABI is
// include/fiunet.h).  The units: fiunet.hip (context, weights, plan, forward, debug entry points), conv_f32.hip /
// conv_f16.hip / conv_bf16.hip / conv_bf16x2.hip (the conv kernels, nothing else), formats.hip, metrics.hip, video.hip
// and flow.hip (one topic each).  Every __global__ kernel is compiled into exactly one of them: a kernel another unit
// needs is reached through a host function declared here (zero_fill_async, launch_conv).  State has one definition, in
// fiunet.hip.
#pragma once
#include "../../include/fiunet.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#pragma GCC visibility push(hidden)   // (shared between the units, not exported from the library)

namespace fiunet {

struct ConvArgs;   // conv_common.hip.h

// The message fiunet_last_error_string() returns on this thread, whichever unit raised it.  The thread-local string has
// its one definition in fiunet.hip and the other units reach it through these two: a thread_local variable named from
// another unit is read through a weak "TLS init" symbol, and a hidden weak symbol that stays undefined (a variable that
// needs no dynamic initialisation) cannot be tested for null inside a shared object - the test compares load address + 0.
std::string& last_error();
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(FIUNET_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr int NCONV = 18;
// output channels of the 18 convs: bilinear=True (factor 2, Up's DoubleConv has mid = in / 2; the only variant a reference
// caller constructs) and bilinear=False (the constructor's default, unet.py:66,99: factor 1, down4 -> 1024, Up =
// ConvTranspose2d(in, in / 2, 2, 2) + DoubleConv(in, out), unet.py:42-44)
inline constexpr int kCoutBil[NCONV] = {64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 256, 256, 128, 128, 64, 64, 64};
inline constexpr int kCoutCT[NCONV] = {64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64};

struct ConvWeights {
    int cin = 0, cout = 0;
    void* w_f32 = nullptr;   // packed [cin/16][kx][ky][cout][16] fp32   (conv 0: [9][cin][64])
    void* w_bf16 = nullptr;  // packed [cin/32][kx][ky][cout][32] bf16
    void* w_x2 = nullptr;    // FIUNET_BF16X2 (fiunet_prepare_precision): two pieces [wh | wl], each packed like w_bf16
    void* w_f16 = nullptr;   // FIUNET_FP16 (fiunet_prepare_precision): packed like w_bf16, IEEE half values
    float* scale = nullptr;
    float* shift = nullptr;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline bool valid_precision(int p) { return p == FIUNET_FP32 || p == FIUNET_BF16 || p == FIUNET_BF16X2 || p == FIUNET_FP16; }

template <typename T> constexpr const char* elem_name()
{
    return std::is_same_v<T, _Float16> ? "f16" : sizeof(T) == 2 ? "bf16" : "f32";
}

inline unsigned grid_for(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 256 * 32); }

// `bytes` (a multiple of 4) of zeros from the 16-byte-aligned `p`, as a kernel on `s` (pointwise.hip.h, zero_fill_kernel:
// why it is not hipMemsetAsync)
int zero_fill_async(void* p, size_t bytes, hipStream_t s);

inline long long padded_area(int H, int W, int TH, int TW)
{
    return (long long)((H + TH - 1) / TH) * TH * ((W + TW - 1) / TW) * TW;
}

// The 32-pixel-wide tiles are the tuned ones (whole 128-B lines per tile row, no register spills in
// any variant); the narrow tiles only win when they save real padding work: more than 1/32 of it
// (135x240 at 8x32 pads to 136x256 = +0.7 % over 16x16 and still runs 10 % faster per FLOP).
inline bool prefer_wide(int H, int W, int THw, int TWw, int THn, int TWn)
{
    const long long wide = padded_area(H, W, THw, TWw), narrow = padded_area(H, W, THn, TWn);
    return wide * 32 <= narrow * 33;
}

// the launch configuration of one conv stage (fiunet.hip: choose_conv_cfg, plan_stages)
struct ConvCfg { bool small; int ksplit; bool kwave = false; };   // kwave: the K loop cut over the four waves of a workgroup (conv3x3_kwave.hip.h)

// where the next conv launch on this thread reports its kernel (fiunet_profile_read), nullptr: nowhere; the thread-local
// pointer is fiunet.hip's (g_name_out)
std::string* name_out();

// One conv stage (conv_launch.hip.h).  mode: SRC_DIRECT | SRC_CONCAT_UP | SRC_DIRECT_X2 | SRC_STEM | SRC_STEM_X2; epi:
// EPI_PLAIN | EPI_HEAD | EPI_HEAD3 | EPI_POOL (direct sources only); cfg: the stage's (plan_stages).  Each instantiation,
// with every kernel it launches, is compiled in the conv unit of its element type; the two-piece modes of __bf16
// (FIUNET_BF16X2) in a unit of their own, behind launch_conv_x2.
template <typename T> int launch_conv(const ConvArgs& a, int mode, int epi, const ConvCfg& cfg, hipStream_t s);
extern template int launch_conv<float>(const ConvArgs&, int, int, const ConvCfg&, hipStream_t);
extern template int launch_conv<_Float16>(const ConvArgs&, int, int, const ConvCfg&, hipStream_t);
extern template int launch_conv<__bf16>(const ConvArgs&, int, int, const ConvCfg&, hipStream_t);
int launch_conv_x2(const ConvArgs& a, int mode, int epi, const ConvCfg& cfg, hipStream_t s);

}  // namespace fiunet

#pragma GCC visibility pop

struct fiunet_ctx {
    int device = 0;
    int cf = 1;  // channels per frame
    bool bilinear = true;          // false: ConvTranspose2d decoder (unet.py:42-44)
    const int* cout = fiunet::kCoutBil;    // output channels per conv of this architecture
    struct { int cin = 0, cout = 0; void* w_f32 = nullptr; void* w_bf16 = nullptr; void* w_x2 = nullptr; void* w_f16 = nullptr; float* bias = nullptr; } convt[4];
    bool x2_ready = false;         // the two-piece weight copies exist (fiunet_prepare_precision(FIUNET_BF16X2))
    bool f16_ready = false;        // the fp16 weight copies exist (fiunet_prepare_precision(FIUNET_FP16))
    unsigned flags = 0;
    bool loaded = false;
    fiunet::ConvWeights conv[fiunet::NCONV];
    float* head_w = nullptr;  // [cf][64]
    float* head_b = nullptr;  // [cf]
    void* stem_w_split = nullptr;  // gray stem weights x BatchNorm scale as bf16 hi/lo pairs [2][64][32] (fused stem)
    unsigned long long* stamps = nullptr;  // per-wave cycle records (diagnostic -DFIUNET_STAMP builds)
    int stamp_layer = -1;
    int force_tile[fiunet::NCONV] = {0};     // diagnostic overrides of choose_conv_cfg per conv (fiunet_debug_force_cfg; tools/cfg_sweep.py)
    int force_ksplit[fiunet::NCONV] = {0};
    std::vector<void*> owned;
    hipEvent_t load_done = nullptr;  // recorded behind the kernels of fiunet_load_weights_device (fiunet_prepare_precision waits for it)
    // per-layer HIP-event profiling (fiunet_profile_*): NCONV+1 events per recorded forward
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::string layer_name[fiunet::NCONV];
    double layer_flops[fiunet::NCONV] = {0};
};
