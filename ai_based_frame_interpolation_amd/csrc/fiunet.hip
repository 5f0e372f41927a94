// fiunet.hip -- C ABI (include/fiunet.h) + host orchestration of the MI355X UNet forward.
//
// Replaces, for the hot path only, the Python surface of the reference:
//   FrameInterpolationUNet.__init__/forward   /root/reference/model/unet.py:97-112
//   UNet.__init__/forward (wiring)            /root/reference/model/unet.py:65-95
//   load_state_dict + .to(device) + .eval()   /root/reference/model/inference.py:83-97
//   pre/post-processing arithmetic            /root/reference/model/inference.py:31-35, :54-61
// Device code: conv3x3_mfma.hip.h (MFMA implicit-GEMM conv) and pointwise.hip.h.
// gfx950 only; no CPU fallback: every entry point either launches HIP kernels or returns an error.
#include "../../include/fiunet.h"
#include "pointwise.hip.h"
#include "conv3x3_kwave.hip.h"
#include "metrics.hip.h"
#include "colour.hip.h"
#include "packed.hip.h"
#include "yuv4xx.hip.h"
#include "scene.hip.h"
#include "retime.hip.h"
#include "resize.hip.h"
#include "weights.hip.h"
#include "flow.hip.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace fiunet;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(FIUNET_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr int NCONV = 18;
constexpr size_t kSlabBytes = 64u << 20;  // split-K slab: ksplit * B*H*W*Cout * 4 <= ~50 MB by construction
[[maybe_unused]] constexpr size_t kStampWaves = 4 * 40000;  // diagnostic stamp records (128 B each); launches with more waves leave the rest unrecorded
[[maybe_unused]] constexpr size_t kStampRec = 16;              // u64 slots per record
// conv index = 2*block + {0,1}; blocks: inc, down1..4, up1..4 (state-dict order)
const char* const kBlockPrefix[9] = {
    "unet.inc", "unet.down1.maxpool_conv.1", "unet.down2.maxpool_conv.1",
    "unet.down3.maxpool_conv.1", "unet.down4.maxpool_conv.1", "unet.up1.conv", "unet.up2.conv",
    "unet.up3.conv", "unet.up4.conv"};
// output channels of the 18 convs: bilinear=True (factor 2, Up's DoubleConv has mid = in / 2; the only variant a reference
// caller constructs) and bilinear=False (the constructor's default, unet.py:66,99: factor 1, down4 -> 1024, Up =
// ConvTranspose2d(in, in / 2, 2, 2) + DoubleConv(in, out), unet.py:42-44)
const int kCoutBil[NCONV] = {64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 256, 256, 128, 128, 64, 64, 64};
const int kCoutCT[NCONV] = {64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64};
const int kLevel[NCONV] = {0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0};
// gather mode and sources (activation indices) of each conv; conv 0 is the fp32 stem kernel
// SRC_POOL here means "reads MaxPool2d(2) of its source": the pooled tensor is written by the
// producer conv's epilogue (EPI_POOL) -- or by maxpool2_kernel on the ablation path -- and the
// consumer then gathers it like any other NHWC tensor.
const int kMode[NCONV] = {-1, SRC_DIRECT, SRC_POOL, SRC_DIRECT, SRC_POOL, SRC_DIRECT, SRC_POOL,
                          SRC_DIRECT, SRC_POOL, SRC_DIRECT, SRC_CONCAT_UP, SRC_DIRECT,
                          SRC_CONCAT_UP, SRC_DIRECT, SRC_CONCAT_UP, SRC_DIRECT, SRC_CONCAT_UP,
                          SRC_DIRECT};
// producer conv i -> index of the pooled copy it also emits (convs 1,3,5,7 = x1..x4), else -1
const int kPoolOut[NCONV] = {-1, 0, -1, 1, -1, 2, -1, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
const int kSrc0[NCONV] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 7, 10, 5, 12, 3, 14, 1, 16};
const int kSrc1[NCONV] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 9, -1, 11, -1, 13, -1, 15, -1};

struct ConvWeights {
    int cin = 0, cout = 0;
    void* w_f32 = nullptr;   // packed [cin/16][kx][ky][cout][16] fp32   (conv 0: [9][cin][64])
    void* w_bf16 = nullptr;  // packed [cin/32][kx][ky][cout][32] bf16
    void* w_x2 = nullptr;    // FIUNET_BF16X2 (fiunet_prepare_precision): two pieces [wh | wl], each packed like w_bf16
    void* w_f16 = nullptr;   // FIUNET_FP16 (fiunet_prepare_precision): packed like w_bf16, IEEE half values
    float* scale = nullptr;
    float* shift = nullptr;
};

// (bf16_row_to_cout, f32_to_bf16_rne, f32_to_bf16_feedback: weights.hip.h - one definition for the host loop of
// fiunet_load_weights and the kernels of fiunet_load_weights_device)

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline bool valid_precision(int p) { return p == FIUNET_FP32 || p == FIUNET_BF16 || p == FIUNET_BF16X2 || p == FIUNET_FP16; }
// bf16 and fp16: one 2-byte element per activation and weight (32 channels per 64-B plane, the same MFMA shape), so both
// take every branch of the launch rule and the same workspace layout; fp32 and bf16x2 (two bf16 pieces) have 4 bytes
inline bool two_byte_elems(int p) { return p != FIUNET_FP32 && p != FIUNET_BF16X2; }
template <typename T> constexpr const char* elem_name()
{
    return std::is_same_v<T, _Float16> ? "f16" : sizeof(T) == 2 ? "bf16" : "f32";
}

}  // namespace

struct fiunet_ctx {
    int device = 0;
    int cf = 1;  // channels per frame
    bool bilinear = true;          // false: ConvTranspose2d decoder (unet.py:42-44)
    const int* cout = kCoutBil;    // output channels per conv of this architecture
    struct { int cin = 0, cout = 0; void* w_f32 = nullptr; void* w_bf16 = nullptr; void* w_x2 = nullptr; void* w_f16 = nullptr; float* bias = nullptr; } convt[4];
    bool x2_ready = false;         // the two-piece weight copies exist (fiunet_prepare_precision(FIUNET_BF16X2))
    bool f16_ready = false;        // the fp16 weight copies exist (fiunet_prepare_precision(FIUNET_FP16))
    unsigned flags = 0;
    bool loaded = false;
    ConvWeights conv[NCONV];
    float* head_w = nullptr;  // [cf][64]
    float* head_b = nullptr;  // [cf]
    void* stem_w_split = nullptr;  // gray stem weights x BatchNorm scale as bf16 hi/lo pairs [2][64][32] (fused stem)
    unsigned long long* stamps = nullptr;  // per-wave cycle records (diagnostic -DFIUNET_STAMP builds)
    int stamp_layer = -1;
    int force_tile[NCONV] = {0};     // diagnostic overrides of choose_conv_cfg per conv (fiunet_debug_force_cfg; tools/cfg_sweep.py)
    int force_ksplit[NCONV] = {0};
    std::vector<void*> owned;
    hipEvent_t load_done = nullptr;  // recorded behind the kernels of fiunet_load_weights_device (fiunet_prepare_precision waits for it)
    // per-layer HIP-event profiling (fiunet_profile_*): NCONV+1 events per recorded forward
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::string layer_name[NCONV];
    double layer_flops[NCONV] = {0};
};

namespace {


int dev_upload(fiunet_ctx* ctx, const void* host, size_t bytes, void** out)
{
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    ctx->owned.push_back(d);
    HIP_TRY(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    *out = d;
    return FIUNET_OK;
}

void free_weights(fiunet_ctx* ctx)
{
    for (void* p : ctx->owned) (void)hipFree(p);
    ctx->owned.clear();
    ctx->loaded = false;
    ctx->x2_ready = false;
    ctx->f16_ready = false;
    // (fiunet_prepare_precision and fiunet_load_weights_device reuse a non-null buffer: none may outlive its memory)
    for (auto& c : ctx->conv) { c.w_f32 = c.w_bf16 = c.w_x2 = c.w_f16 = nullptr; c.scale = c.shift = nullptr; }
    for (auto& c : ctx->convt) { c.w_f32 = c.w_bf16 = c.w_x2 = c.w_f16 = nullptr; c.bias = nullptr; }
    ctx->head_w = ctx->head_b = nullptr;
    ctx->stem_w_split = nullptr;
    ctx->stamps = nullptr;
}

thread_local std::string* g_name_out = nullptr;  // where the next conv launch reports its kernel

// One conv kernel on `nblk` workgroups of 256 threads with `lds` bytes of dynamic LDS: more than 64 KiB needs the opt-in
// attribute, set once per kernel and device (a duplicate hipFuncSetAttribute is harmless); `name` is what the profiler
// reports for the stage (fiunet_profile_read).
template <auto Kernel>
int launch_lds(const char* name, long long nblk, int lds, const ConvArgs& a, hipStream_t s)
{
    if (g_name_out) *g_name_out = name;
    if (nblk <= 0 || nblk > 0x7fffffffLL) return fail(FIUNET_ERR_INVALID_ARG, "conv grid too large");
    static std::atomic<bool> lds_attr_set[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && !lds_attr_set[dev].load(std::memory_order_acquire)) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        lds_attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)nblk), dim3(256), lds, s, a);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

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

template <typename T, int BN, int TH, int TW, int MODE, int EPI>
int launch_conv_cfg(ConvArgs a, hipStream_t s)
{
    char name[128] = "";
    if (g_name_out)
        std::snprintf(name, sizeof name, "conv3x3_mfma_kernel<%s,%d,%d,%d,%d,%d>", elem_name<T>(), BN, TH, TW,
                      MODE, EPI);
    a.tilesX = (a.W + TW - 1) / TW;
    a.tilesY = (a.H + TH - 1) / TH;
    a.nct = a.Cout / BN;
    const long long nblk = (long long)a.B * a.tilesX * a.tilesY * a.nct * (epi_is_splitk(EPI) ? a.ksplit : 1);
    return launch_lds<&conv3x3_mfma_kernel<T, BN, TH, TW, MODE, EPI>>(name, nblk, ConvTile<BN, TH, TW, MODE>::LDS_BYTES, a, s);
}

inline unsigned grid_for(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 256 * 32); }

// `bytes` (a multiple of 4) of zeros from the 16-byte-aligned `p`, as a kernel on `s` (pointwise.hip.h, zero_fill_kernel:
// why it is not hipMemsetAsync)
int zero_fill_async(void* p, size_t bytes, hipStream_t s)
{
    if (((uintptr_t)p & 15) || (bytes & 3)) return fail(FIUNET_ERR_INVALID_ARG, "internal: zero-fill of an unaligned range");
    if (!bytes) return FIUNET_OK;
    const size_t n16 = bytes / 16;
    hipLaunchKernelGGL(zero_fill_kernel, dim3(grid_for(std::max<size_t>(n16, 1))), dim3(256), 0, s, (uint4*)p, n16,
                       (unsigned)((bytes % 16) / 4));
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

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

// ---- tile shape and K split of one conv launch ---------------------------------------------------------------------
// Two tile families.  BIG (rounds 1-5, tuned on the 1080p workload): 64 couts x 16x32 / 32x16 pixels or 128 couts x 8x32 /
// 16x16 pixels, every wave a 64 x 128 tile (128 accumulator registers), two workgroups per CU.  SMALL (round 6): 64 couts x
// 8x32 pixels, every wave a 64 x 64 tile, three workgroups per CU - twice (Cout = 64) or four times (Cout >= 128, where two
// cout tiles replace one) the workgroups of the big tile, each with half the MFMAs per step.  On a problem that fills the
// chip the big tile wins (fewer fragment reads per MFMA, half the halo and weight re-reads: measured in rounds 1-3); on a
// problem with fewer big-tile workgroups than the chip has CUs - every layer of the ONE 256x256 pair that is the reference's
// only operating point (/root/reference/model/inference.py:29,101-122) - half the SIMDs have no wave at all and the small
// tile halves the time (fp32: MFMA-bound; bf16: the serial chain of a workgroup's steps).  The K loop (planes) can be cut
// over `ksplit` workgroups as well (raw fp32 partial sums to a slab + splitk_finalize_tile_kernel): worth it only where a
// workgroup's serial K loop is longer than the extra launch (~5 us) - the deep levels.
//
// Neither choice changes a bit of the result as long as ksplit stays the same: the summation order of an output element
// is (plane, kx, ky) in every tile shape, the fused head reduces in the same association, and a K cut only moves where the
// partial sums meet (fp32, in slice order).  The cut itself does change the fp32 summation order, so it must not depend on
// the batch size for frames whose batches are compared bit for bit (a video's ragged last chunk, B=1 vs B=8 at 1080p):
// layers with >= 64 big-tile workgroups PER IMAGE are cut only below 128 workgroups in total, which such a layer never has
// for B >= 2 (a SINGLE pair with 64..127 workgroups per image, e.g. the deepest level of a 720p frame, is); small frames,
// where a single pair is cut anyway, below 256.  fiunet_min_unsplit_batch answers from the stage plan (plan_stages).
struct TileShape { int BN, TH, TW; };
struct ConvCfg { bool small; int ksplit; bool kwave = false; };   // kwave: the K loop cut over the four waves of a workgroup (conv3x3_kwave.hip.h)

inline TileShape big_tile(int H, int W, int Cout)
{
    if (Cout == 64) return prefer_wide(H, W, 16, 32, 32, 16) ? TileShape{64, 16, 32} : TileShape{64, 32, 16};
    return prefer_wide(H, W, 8, 32, 16, 16) ? TileShape{128, 8, 32} : TileShape{128, 16, 16};
}
constexpr TileShape kSmallTile = {64, 8, 32};

inline long long tile_blocks(const TileShape& t, int B, int H, int W, int Cout)
{
    return (long long)B * ((W + t.TW - 1) / t.TW) * ((H + t.TH - 1) / t.TH) * (Cout / t.BN);
}

// K cut of a small problem (tools/cfg_sweep.py on MI355X, ONE 256x256 pair and B = 16 / 1080p B = 1 as cross-checks:
// profiles/r06_cfg_sweep_*.txt).  What the sweep shows:
//  * the small tile beats the big one on every layer of a problem the big tile cannot fill the chip with (12-35 %);
//  * bf16: a lone workgroup's step (48 MFMAs, a barrier, the waits) takes ~0.6 us whatever is done about the weight
//    stream (a 4-deep ring changed nothing and was taken out), a dependent dispatch ~4.5 us, and the slab of a cut costs its bytes twice
//    (k slices of the padded fp32 output written, then read back through the Infinity Cache at ~2.5-4.5 TB/s): cutting
//    pays from 8 planes (24 serial steps) on, best at 2-4 planes per slice - k = 4 for 8 planes, 8 beyond;
//  * fp32: a step is MFMA time (~3 us per 64 x 64 wave tile), so what counts is one workgroup on every CU: k = 256 /
//    workgroups (a second workgroup per CU shares the same MFMA pipes: no gain, twice the slab) - except the concat convs,
//    whose gather interpolates its upsampled half (address arithmetic and blend per tap, latency- not MFMA-bound): two
//    workgroups per CU hide it, k = 512 / workgroups (ONE 256x256 pair, up1.0 / up2.0 / up3.0: 98 -> 92-95 us; four pairs,
//    up1.0: 335 -> 304 us; profiles/r06_cfg_sweep_b{1,4}_256_fp32.txt);
//  * never more workgroups than 512 (bf16) / 256 (fp32) in total, never a slab beyond kSlabBytes.
inline int pow2_floor(long long v) { int k = 1; while (2LL * k <= v) k *= 2; return k; }

inline int small_ksplit(bool fp32, long long nblk, int nplanes, int fp32_slots = 256)
{
    int k;
    if (nblk >= (fp32 ? fp32_slots : 256)) return 1;   // the chip is covered already: a cut only adds the slab (B = 16 256x256, level 4: 39.3 -> 42.9 us)
    if (fp32) k = pow2_floor(std::max<long long>(1, fp32_slots / std::max<long long>(nblk, 1)));
    else {
        k = nplanes < 8 ? 1 : (nplanes < 16 ? 4 : 8);
        k = std::min(k, pow2_floor(std::max<long long>(1, 512 / std::max<long long>(nblk, 1))));
    }
    k = std::min(k, pow2_floor(nplanes));
    while (k > 1 && (size_t)k * nblk * kSmallTile.BN * kSmallTile.TH * kSmallTile.TW * 4 > kSlabBytes) k /= 2;
    return k;
}

// `splittable`: plain / pooled epilogue with a slab to write to (never the fused stem or the fused head).
// force_small: -1 = choose, 0 / 1 = debug override; force_ksplit: 0 = choose, k >= 1 = debug override (powers of two).
// Would a bf16 direct conv of this shape take conv3x3_kwave_kernel?  >= 4 planes of K (one per wave), at most one
// workgroup per CU (136 KiB of LDS each), a problem the tuned tile cannot fill the chip with, and the batch-invariance gate
// of every K cut (it IS one: the fp32 summation order changes).
inline bool kwave_applies(int B, int H, int W, int Cin, int Cout)
{
    const TileShape big = big_tile(H, W, Cout);
    const long long nblk_big = tile_blocks(big, B, H, W, Cout);
    if (nblk_big >= 256 || !(nblk_big < (nblk_big / B < 64 ? 256 : 128))) return false;
    const long long nwg = (long long)B * ((H + 1) / 2) * ((W + 31) / 32) * (Cout / 64);
    return Cin / 32 >= 4 && Cout % 64 == 0 && nwg <= 256;
}

// kwave_ok: the launch has the form conv3x3_kwave_kernel covers (direct sources, plain / pooled epilogue; fp32: see below).
// force_small == 2: that kernel where it applies (diagnostic).
// Between one and a few ROUNDS of tuned-tile workgroups (512 resident slots) the last, partial round decides: 544
// workgroups take 1.6 rounds' time (the 32 left over run alone), 480 take one.  The small tile - three workgroups per CU, 768
// slots, twice the workgroups of half the size - quantises finer and wins exactly where the tuned tile's remainder is
// small: one to four 1080p pairs, levels 3-4: -4 .. -18 % per stage; 480 or 920 workgroups: +4 .. +16 % (the tuned tile
// fits its rounds).  Times in units of a full tuned round; a partial round with `l` of `occ` workgroups per CU takes
// 0.2 + 0.8 l / occ of a full one; a small-tile round does 1.5x the work of a tuned one at ~8 % less efficiency, times the
// padded-area ratio of the two tilings.  Fitted to tools/cfg_sweep.py at eight shapes (profiles/r06_tail_rule_sweeps.txt);
// bf16 direct convs and the >= 256-cout concat convs only (the 64 / 128-cout concat gathers and the fused stem measured
// slower on the small tile at every size: they interpolate / evaluate their halo twice); bf16x2's direct convs follow the
// same rule (A/B: B = 4 1080p 183.2 -> 185.3 frames/s, B = 1 169 -> 178), and so does fp32 (B = 4 53.2 -> 53.9, B = 1 47.5 -> 50.3).
inline bool small_tile_wins_on_the_tail(long long nblk_big, long long nblk_small, double area_ratio)
{
    auto rounds = [](long long n, int slots, int occ) {
        const long long full = n / slots, rem = n % slots;
        return (double)full + (rem ? 0.2 + 0.8 * (double)((rem + 255) / 256) / occ : 0.0);
    };
    return rounds(nblk_small, 768, 3) * 0.81 * area_ratio < rounds(nblk_big, 512, 2);
}

inline ConvCfg choose_conv_cfg(bool fp32, bool x2, int B, int H, int W, int Cin, int Cout, bool splittable,
                               int force_small = -1, int force_ksplit = 0, bool kwave_ok = false, bool tail_rule_ok = false,
                               bool concat_conv = false)
{
    const int PL = fp32 ? 16 : 32;
    const int nplanes = Cin / PL * (x2 ? 3 : 1);
    const TileShape big = big_tile(H, W, Cout);
    const long long nblk_big = tile_blocks(big, B, H, W, Cout), nblk_small = tile_blocks(kSmallTile, B, H, W, Cout);
    // the chip is full with the tuned tile: whole K loop; the tile by the partial-round rule up to a few rounds, tuned beyond
    if (nblk_big >= 256 && force_small < 0 && force_ksplit <= 0) {
        const bool small = tail_rule_ok && nblk_big <= 2304 &&
                           small_tile_wins_on_the_tail(nblk_big, nblk_small,
                                                       (double)padded_area(H, W, kSmallTile.TH, kSmallTile.TW) /
                                                           (double)padded_area(H, W, big.TH, big.TW));
        return ConvCfg{small, 1};
    }
    const bool may_split = splittable && nblk_big < (nblk_big / B < 64 ? 256 : 128);
    // bf16, direct sources, >= 4 planes of K, at most one workgroup per CU: the K loop cut over the WAVES of a workgroup
    // (conv3x3_kwave.hip.h) - a quarter of the serial step chain with no slab and no reduction dispatch (kwave_applies).
    // (bf16x2 runs nine steps per real plane: from 16 planes on its per-wave chain is longer than what a cross-workgroup cut
    // of 8 leaves - ONE 256x256 pair, down4: 34 us against 26 - so there the slab form stays; profiles/r06_cfg_sweep_b1_256_bf16x2.txt)
    if (kwave_ok && fp32 && splittable && Cin / 16 >= 4 && force_small == 2) return ConvCfg{true, 1, true};
    if (kwave_ok && !fp32 && splittable && Cin / 32 >= 4 && (force_small == 2 || (force_small < 0 && force_ksplit <= 0))) {
        if (force_small == 2 || (kwave_applies(B, H, W, Cin, Cout) && !(x2 && Cin / 32 > 8))) return ConvCfg{true, 1, true};
    }
    if (force_small == 2) force_small = 1;
    auto big_ksplit = [&]() {   // the rule of rounds 1-5 for the tuned tiles (powers of two)
        int k = (int)std::min<long long>(std::min(nplanes / 2, 16), (256 + nblk_big - 1) / nblk_big);
        k = k > 1 ? pow2_floor(k) : 1;
        while (k > 1 && (size_t)k * nblk_big * big.BN * big.TH * big.TW * 4 > kSlabBytes) k /= 2;
        return k;
    };
    bool small = force_small >= 0 ? force_small != 0 : true;
    if (force_small < 0 && fp32) {
        // fp32 is MFMA-bound per SIMD: where the 8x32 tile pads a narrow level (16 columns: half of every tile is
        // padding) AND the batch already fills the chip, the tuned 16x16 tile with its K cut does half the MFMAs
        // (B = 16 256x256, level 4: 64 tuned workgroups x 4 slices x 24 steps against 256 small ones x 96 steps)
        const int slots = concat_conv ? 512 : 256;
        auto mfma_ns = [&](long long nblk, int k, double step_ns) {
            const long long nwg = nblk * k;
            return (double)((nwg + slots - 1) / slots) * ((nplanes + k - 1) / k * 3) * step_ns + (k > 1 ? 8000.0 : 0.0);
        };
        const int ks = may_split ? small_ksplit(true, nblk_small, nplanes, slots) : 1, kb = may_split ? big_ksplit() : 1;
        small = mfma_ns(nblk_small, ks, 2950.0) <= mfma_ns(nblk_big, kb, 5900.0);
        // fp32 and the in-workgroup cut (conv3x3_kwave_kernel<.., float>): the same MFMA time per SIMD as a cut over
        // workgroups when its workgroups x 4 waves cover the chip, without the slab and the reduce dispatch (~8 us).
        // One workgroup per CU (136 KiB of LDS), up to two rounds of them.  ONE 256x256 pair: down1.0 35.0 -> 31.7 us,
        // down1.1 56.3 -> 50.9, down2.0 34 -> 28.0, down2.1 57 -> 47.1, up3.1 35 -> 27.3; where the cut over workgroups
        // reaches one workgroup per CU with fewer steps it stays (down3.0: 35.4 against 43.0) - profiles/r06_cfg_sweep_b{1,4}_256_fp32.txt
        if (kwave_ok && splittable && may_split && nplanes >= 4 && Cout % 64 == 0) {
            const long long nwg = (long long)B * ((H + 1) / 2) * ((W + 31) / 32) * (Cout / 64);
            const double kw = (double)((nwg + 255) / 256) * ((nplanes + 3) / 4 * 3) * 2950.0;
            if (nwg <= 512 && kw < (small ? mfma_ns(nblk_small, ks, 2950.0) : mfma_ns(nblk_big, kb, 5900.0))) return ConvCfg{true, 1, true};
        }
    }
    const TileShape& t = small ? kSmallTile : big;
    const long long nblk = small ? nblk_small : nblk_big;
    int k = 1;
    if (force_ksplit > 0) {
        k = splittable ? std::min(pow2_floor(force_ksplit), pow2_floor(nplanes)) : 1;
        while (k > 1 && (size_t)k * nblk * t.BN * t.TH * t.TW * 4 > kSlabBytes) k /= 2;
    } else if (may_split) {
        k = small ? small_ksplit(fp32, nblk, nplanes, concat_conv ? 512 : 256) : big_ksplit();
    }
    return ConvCfg{small, k};
}

// An fp32 concat conv whose direct two-source form would take the in-workgroup K cut: its upsampled half is materialised
// (upsample_kernel, one more dispatch) and the conv launched in that form - on the ablation path too (upcat_kernel's single
// source has the same planes in the same order), so the two paths keep the same summation order.
inline bool fp32_concat_takes_kwave(int B, int H, int W, int Cin, int Cout)
{
    return choose_conv_cfg(true, false, B, H, W, Cin, Cout, true, -1, 0, true, false, false).kwave;
}

// ---- the stage plan: how every stage of one forward launches -------------------------------------------------------
// plan_stages is the one place that decides, per stage, the source form, the epilogue, the split-K slab and the launch
// configuration (choose_conv_cfg, overrides included).  The forward walks the plan; make_plan lays the workspace out from
// it; fiunet_min_unsplit_batch and fiunet_debug_stage_cfg read it.
enum StemForm {          // stage 0: which kernel computes the stem (unet.py:72, first conv of inc)
    STEM_FUSED = 0,      //   none: conv 1 evaluates it inside its gather (FORM_STEM)
    STEM_FIRST = 1,      //   conv3x3_first_kernel
    STEM_RGB_SPLIT = 2,  //   stem_rgb_split_kernel (RGB, bf16 / bf16x2)
};
enum SrcForm {               // stages 1..17: what the conv gathers
    FORM_DIRECT = 0,         //   an activation
    FORM_POOL = 1,           //   MaxPool2d(2) of one (the producer's EPI_POOL, or maxpool2_kernel on the ablation path)
    FORM_CONCAT_GATHER = 2,  //   skip + the bilinear 2x upsample of the low-res tensor, interpolated in the gather (SRC_CONCAT_UP)
    FORM_CONCAT_UP = 3,      //   skip + that upsample materialised first (upsample_kernel / x2_upsample_kernel)
    FORM_CONCAT_CONVT = 4,   //   skip + ConvTranspose2d of the low-res tensor (convt2x2_kernel; bilinear=False)
    FORM_CONCAT_UPCAT = 5,   //   the ablation path: the whole concat tensor written by upcat_kernel
    FORM_STEM = 6,           //   the gray stem evaluated in the gather (SRC_STEM / SRC_STEM_X2)
};
struct StageLaunch {
    int form = FORM_DIRECT;   // stage 0: StemForm
    int epi = EPI_PLAIN;      // EPI_PLAIN | EPI_POOL | EPI_HEAD | EPI_HEAD3
    bool slab = false;        // gets the split-K slab
    bool stored = true;       // its output is a tensor in the workspace
    ConvCfg cfg{false, 1, false};
};

// What the plan depends on besides precision and shape.
struct NetDesc {
    int cf = 1;                        // channels per frame
    bool bilinear = true;              // false: ConvTranspose2d decoder (unet.py:42-44)
    const int* cout = kCoutBil;        // output channels per conv of this architecture
    unsigned flags = 0;                // FIUNET_OPT_*
    bool stem_w = false;               // the fused-stem weight copy exists (gray)
    const int* force_tile = nullptr;   // diagnostic overrides per conv (fiunet_debug_force_cfg), nullptr = none
    const int* force_ksplit = nullptr;
};

// input channels of conv i >= 1
inline int conv_cin(const int* cout, bool bilinear, int i)
{
    if (kMode[i] != SRC_CONCAT_UP) return cout[kSrc0[i]];
    return cout[kSrc0[i]] + (bilinear ? cout[kSrc1[i]] : cout[kSrc1[i]] / 2);
}

// A bf16 / fp32 bilinear concat conv: is its upsampled half written to HBM first?  One whose output spans several 128-cout
// tiles would bilinearly interpolate every input tile once per cout tile (4x at up1, 2x at up2): there the upsampled half is
// written once (upsample_kernel) and gathered by plain LDS-DMA like the skip half.  bf16 only: on the fp32 matrix cores the
// interpolation is small beside the 16x slower MFMAs, and the tensor twice as big.  Small problems (launch-bound, K-split)
// keep the fused gather - unless the conv then qualifies for the in-workgroup K cut (conv3x3_kwave.hip.h, direct sources
// only): a quarter of the serial step chain is worth the extra upsample dispatch (ONE 256x256 pair: up1.0 34 -> 23 us, up2.0
// 30 -> 18 us).  B, H, W: the stage's level.
inline bool materialise_up(int precision, int B, int H, int W, int Cin, int Cout)
{
    if (precision == FIUNET_FP32) return fp32_concat_takes_kwave(B, H, W, Cin, Cout);
    if (Cout >= 256 && (long long)B * H * W >= 65536) return true;
    return kwave_applies(B, H, W, Cin, Cout);
}

void plan_stages(const NetDesc& n, int precision, int B, int H, int W, StageLaunch L[NCONV])
{
    const bool fp32 = precision == FIUNET_FP32, x2 = precision == FIUNET_BF16X2;
    const bool keep_all = n.flags & FIUNET_OPT_KEEP_ALL;
    // bf16x2 has no ablation path and no in-gather upsample
    const bool unfused = !x2 && (n.flags & FIUNET_OPT_UNFUSED), gather_up = !x2 && (n.flags & FIUNET_OPT_GATHER_UPSAMPLE);
    int hs[5] = {H}, ws[5] = {W};
    for (int k = 1; k < 5; ++k) { hs[k] = hs[k - 1] / 2; ws[k] = ws[k - 1] / 2; }
    // gray bf16 / bf16x2: the stem is evaluated inside conv 1's gather (16x32 tiles only), unless the ablation path needs its
    // output in HBM.  The debug read-back (KEEP_ALL) runs the stem kernel for tap 0 as well: in bf16 conv 1 still evaluates the
    // stem in its gather (the fused numerics are what the read-back must show downstream), in bf16x2 it reads tap 0.
    const bool fuse_stem = !fp32 && n.cf == 1 && n.stem_w && !unfused && !(x2 && keep_all) && prefer_wide(H, W, 16, 32, 32, 16);
    L[0] = StageLaunch{};
    L[0].form = fuse_stem && !keep_all ? STEM_FUSED : n.cf == 3 && !fp32 ? STEM_RGB_SPLIT : STEM_FIRST;
    L[0].stored = L[0].form != STEM_FUSED;
    for (int i = 1; i < NCONV; ++i) {
        StageLaunch& st = L[i];
        st = StageLaunch{};
        const int h = hs[kLevel[i]], w = ws[kLevel[i]], cin = conv_cin(n.cout, n.bilinear, i), cout = n.cout[i];
        if (i == 1 && fuse_stem) st.form = FORM_STEM;
        else if (kMode[i] == SRC_POOL) st.form = FORM_POOL;
        else if (kMode[i] == SRC_CONCAT_UP) {
            if (!n.bilinear) st.form = FORM_CONCAT_CONVT;
            else if (x2) st.form = FORM_CONCAT_UP;
            else if (unfused) st.form = FORM_CONCAT_UPCAT;
            else st.form = !gather_up && materialise_up(precision, B, h, w, cin, cout) ? FORM_CONCAT_UP : FORM_CONCAT_GATHER;
        }
        if (kPoolOut[i] >= 0 && !unfused) st.epi = EPI_POOL;                            // also MaxPool2d(2) of the output (unet.py:28)
        if (i == NCONV - 1 && !unfused) st.epi = n.cf == 1 ? EPI_HEAD : EPI_HEAD3;      // OutConv (unet.py:60) in the last epilogue
        // the last conv is never K-split: its fused-head form cannot be, and the ablation path must accumulate in the same
        // order to stay bit-identical with it
        st.slab = i != NCONV - 1;
        st.stored = !(i == NCONV - 1 && st.epi != EPI_PLAIN && !keep_all);
        const bool stem = st.form == FORM_STEM, gather = st.form == FORM_CONCAT_GATHER, direct = !stem && !gather;
        const bool plain_or_pool = st.epi == EPI_PLAIN || st.epi == EPI_POOL;
        // an fp32 concat conv on the ablation path whose fused counterpart keeps the in-gather form takes that form's
        // configuration (same K cut, never conv3x3_kwave_kernel), so that the two paths stay bit-identical per stage
        const bool as_gather = st.form == FORM_CONCAT_UPCAT && fp32 && !fp32_concat_takes_kwave(B, h, w, cin, cout);
        st.cfg = choose_conv_cfg(fp32, x2, B, h, w, cin, cout, !stem && plain_or_pool && st.slab,
                                 (n.force_tile ? n.force_tile[i] : 0) - 1, stem || !n.force_ksplit ? 0 : n.force_ksplit[i],
                                 direct && plain_or_pool && !as_gather, direct || (gather && cout >= 256), gather || as_gather);
    }
}

struct Plan {
    StageLaunch st[NCONV];
    int hs[5], ws[5];
    size_t act_off[NCONV];
    size_t pool_off[4];  // MaxPool2d(2) of x1..x4: kCout[2k+1] channels at level k+1
    size_t scratch_off;
    size_t up_off[NCONV];  // upsampled half of a concat input, where it is materialised (else unused)
    size_t slab_off;   // split-K partial sums (small problems), kSlabBytes
    size_t total;
};

// One buffer of the workspace plan: what it holds, how many bytes, the live interval [first, last] in stages, and where its
// offset goes in the Plan (fiunet_debug_plan reads the placed list back).
enum BufKind { BUF_ACT = 0, BUF_POOL = 1, BUF_UP = 2, BUF_SCRATCH = 3, BUF_SLAB = 4 };
struct PlanBuf { int kind, index; size_t bytes; int first, last; size_t* off; };

// The stage plan and the workspace plan of one forward.  The reference, under no_grad, frees every non-skip tensor as soon
// as its consumer has run (model/unet.py:84-95 keeps only x1..x4 alive); here the same liveness is turned into a static
// layout: every buffer gets the interval [stage that writes it, last stage that reads it] (stage i = conv i of the 18) and
// buffers whose intervals do not overlap share bytes (first-fit over the buffers in order of their first stage).  B=8 1080p
// bf16 needs 6.2 GB this way instead of the 12.7 GB of one private buffer per tensor (tests/test_workspace_plan.py holds
// both figures).  FIUNET_OPT_KEEP_ALL (the debug read-back) pins every activation to the end (17.0 GB there); the ablation
// path adds its concat scratch; the fused stem / fused head leave activations 0 / 17 out altogether.
// `placed` (diagnostic): receives the buffers in placement order, their `off` pointing into `p`.
// g_plan_refusal: why the last make_plan on this thread answered false.
thread_local const char* g_plan_refusal = "";
bool make_plan(const NetDesc& n, int B, int H, int W, int precision, Plan& p, std::vector<PlanBuf>* placed = nullptr)
{
    g_plan_refusal = "B must be >= 1, H and W >= 16 (four 2x2 max-pools)";
    if (B < 1 || H < 16 || W < 16) return false;
    g_plan_refusal = "H*W must be below 2^26 pixels per call: cut taller frames into bands (fiunet_forward_strip)";
    // the kernels address a pixel record inside one image plane with 32 bits: H*W*64 B < 4 GiB.
    // Larger frames go through fiunet_forward_strip band by band.
    if ((long long)H * W >= (1LL << 26)) return false;
    plan_stages(n, precision, B, H, W, p.st);
    const bool keep_all = n.flags & FIUNET_OPT_KEEP_ALL;
    const size_t es = two_byte_elems(precision) ? 2 : 4;   // bytes per activation element (bf16x2: two pieces)
    p.hs[0] = H; p.ws[0] = W;
    for (int k = 1; k < 5; ++k) { p.hs[k] = p.hs[k - 1] / 2; p.ws[k] = p.ws[k - 1] / 2; }
    // a materialised upsampled half is written by a grid of (row chunks, H / UPS_ROWS, B * planes): a shape whose grid.y or
    // grid.z would pass the 65535 of the launch is refused here, before any stage of a forward runs
    for (int i = 1; i < NCONV; ++i)
        if (p.st[i].form == FORM_CONCAT_UP &&
            ((p.hs[kLevel[i]] + UPS_ROWS - 1) / UPS_ROWS > 65535 ||
             (long long)B * (n.cout[kSrc1[i]] / (precision == FIUNET_FP32 ? 16 : 32)) > 65535)) {
            g_plan_refusal = "upsample grid too large: cut the frame into shorter bands (fiunet_forward_strip) or the batch "
                             "into smaller ones";
            return false;
        }
    using Buf = PlanBuf;
    std::vector<Buf> bufs;
    const int END = NCONV;  // "still live after the last conv" (the unfused head, the debug read-back)
    for (int i = 0; i < NCONV; ++i) {
        p.act_off[i] = 0;
        if (!p.st[i].stored) continue;
        int last = i;  // conv j reads act i as its direct / skip source (kSrc0) or low-res source (kSrc1)
        for (int j = i + 1; j < NCONV; ++j)
            if (kSrc0[j] == i || kSrc1[j] == i) last = j;
        if (i == NCONV - 1 || keep_all) last = END;
        bufs.push_back({BUF_ACT, i, align256((size_t)B * p.hs[kLevel[i]] * p.ws[kLevel[i]] * n.cout[i] * es), i, last,
                        &p.act_off[i]});
    }
    for (int k = 0; k < 4; ++k) {  // MaxPool2d(2) of x1..x4: written by conv 2k+1, read by conv 2k+2
        bufs.push_back({BUF_POOL, k, align256((size_t)B * p.hs[k + 1] * p.ws[k + 1] * n.cout[2 * k + 1] * es), 2 * k + 1,
                        keep_all ? END : 2 * k + 2, &p.pool_off[k]});
    }
    bool upcat = false;
    for (int i = 0; i < NCONV; ++i) {
        p.up_off[i] = 0;
        const int form = i ? p.st[i].form : -1;
        upcat |= form == FORM_CONCAT_UPCAT;
        if (form == FORM_CONCAT_UP || form == FORM_CONCAT_CONVT)
            bufs.push_back({BUF_UP, i, align256((size_t)B * p.hs[kLevel[i]] * p.ws[kLevel[i]] *
                                             (form == FORM_CONCAT_CONVT ? n.cout[kSrc1[i]] / 2 : n.cout[kSrc1[i]]) * es), i,
                            keep_all ? END : i, &p.up_off[i]});
    }
    p.scratch_off = 0;
    if (upcat)  // ablation path: concat tensor (<= 128 ch at level 0), rewritten by every Up block
        bufs.push_back({BUF_SCRATCH, 0, align256((size_t)B * H * W * 128 * es), 0, END, &p.scratch_off});
    bufs.push_back({BUF_SLAB, 0, kSlabBytes, 0, END, &p.slab_off});  // split-K partial sums (small problems)
    std::stable_sort(bufs.begin(), bufs.end(), [](const Buf& a, const Buf& b) { return a.first < b.first; });
    struct Live { size_t off, bytes; int last; };
    std::vector<Live> live;
    size_t total = 0;
    for (const Buf& b : bufs) {
        // buffers whose last reader ran before this one's writer are dead (a conv never reads and
        // writes the same bytes: its sources are live through its own stage)
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live& l) { return l.last < b.first; }),
                   live.end());
        std::sort(live.begin(), live.end(), [](const Live& a, const Live& c) { return a.off < c.off; });
        size_t off = 0;
        for (const Live& l : live) {
            if (off + b.bytes <= l.off) break;
            off = std::max(off, l.off + l.bytes);
        }
        *b.off = off;
        live.push_back({off, b.bytes, b.last});
        total = std::max(total, off + b.bytes);
    }
    p.total = total;
    if (placed) *placed = bufs;
    return true;
}

// The K loop cut over the four waves of a workgroup (small problems, direct sources, every precision): conv3x3_kwave.hip.h.
template <typename T, int EPI, bool X2> int launch_kwave(ConvArgs a, hipStream_t s)
{
    using Tile = KWaveTile;
    char name[96] = "";
    if (g_name_out)
        std::snprintf(name, sizeof name, "conv3x3_kwave_kernel<%s%s,64,2,32,%d>+kwave4", elem_name<T>(), X2 ? "x2" : "", EPI);
    a.tilesX = (a.W + Tile::TW - 1) / Tile::TW;
    a.tilesY = (a.H + Tile::TH - 1) / Tile::TH;
    a.nct = a.Cout / Tile::BN;
    return launch_lds<&conv3x3_kwave_kernel<EPI, X2, T>>(name, (long long)a.B * a.tilesX * a.tilesY * a.nct, Tile::LDS_BYTES, a, s);
}

// One conv launch in a given tile shape; ksplit > 1: the K loop (planes) cut over `ksplit` workgroups that store raw
// fp32 partial sums, then splitk_finalize_tile_kernel adds them in slice order (deterministic) and runs the epilogue.
template <typename T, int BN, int TH, int TW, int MODE, int EPI>
int launch_conv_maybe_split(ConvArgs a, hipStream_t s, int ksplit)
{
    if constexpr (!src_is_stem(MODE) && (EPI == EPI_PLAIN || EPI == EPI_POOL)) {
        if (ksplit > 1 && a.kslab && a.dst) {
            ConvArgs k = a;
            k.ksplit = ksplit;
            int rc = launch_conv_cfg<T, BN, TH, TW, MODE, EPI_SPLITK>(k, s);
            if (rc) return rc;
            k.tilesX = (a.W + TW - 1) / TW;
            k.tilesY = (a.H + TH - 1) / TH;
            k.nct = a.Cout / BN;
            const long long ntile = (long long)a.B * k.tilesX * k.tilesY * k.nct;
            hipLaunchKernelGGL((splitk_finalize_tile_kernel<T, BN, TH, TW, EPI, src_is_x2(MODE)>), dim3((unsigned)(4 * ntile)), dim3(64), 0, s, k);
            HIP_TRY(hipGetLastError());
            if (g_name_out) *g_name_out += "+splitk" + std::to_string(ksplit);
            return FIUNET_OK;
        }
    }
    return launch_conv_cfg<T, BN, TH, TW, MODE, EPI>(a, s);
}

template <typename T, int MODE, int EPI> int launch_conv_shape(const ConvArgs& a, const ConvCfg& cfg, hipStream_t s)
{
    if (a.Cout != 64 && a.Cout % 128 != 0) return fail(FIUNET_ERR_INVALID_ARG, "Cout must be 64 or k*128");
    if ((EPI == EPI_HEAD || EPI == EPI_HEAD3) && a.Cout != 64) return fail(FIUNET_ERR_INVALID_ARG, "fused head needs Cout == 64");
    if constexpr ((MODE == SRC_DIRECT || MODE == SRC_DIRECT_X2) && (EPI == EPI_PLAIN || EPI == EPI_POOL)) {
        if (cfg.kwave) return launch_kwave<T, EPI, MODE == SRC_DIRECT_X2>(a, s);
    }
    if (cfg.small) return launch_conv_maybe_split<T, 64, 8, 32, MODE, EPI>(a, s, cfg.ksplit);
    if (a.Cout == 64) {
        const bool wide = prefer_wide(a.H, a.W, 16, 32, 32, 16);
        return wide ? launch_conv_maybe_split<T, 64, 16, 32, MODE, EPI>(a, s, cfg.ksplit)
                    : launch_conv_maybe_split<T, 64, 32, 16, MODE, EPI>(a, s, cfg.ksplit);
    }
    if constexpr (EPI != EPI_HEAD && EPI != EPI_HEAD3) {
        const bool wide = prefer_wide(a.H, a.W, 8, 32, 16, 16);
        return wide ? launch_conv_maybe_split<T, 128, 8, 32, MODE, EPI>(a, s, cfg.ksplit)
                    : launch_conv_maybe_split<T, 128, 16, 16, MODE, EPI>(a, s, cfg.ksplit);
    }
    return fail(FIUNET_ERR_INVALID_ARG, "fused head needs Cout == 64");
}

// mode: SRC_DIRECT | SRC_CONCAT_UP | SRC_DIRECT_X2 | SRC_STEM | SRC_STEM_X2; epi: EPI_PLAIN | EPI_HEAD | EPI_HEAD3 | EPI_POOL
// (direct sources only); cfg: the stage's (plan_stages)
template <typename T> int launch_conv(const ConvArgs& a, int mode, int epi, const ConvCfg& cfg, hipStream_t s)
{
    constexpr int PL = Elem<T>::PL;
    if (a.C0 % PL || a.C1 % PL) return fail(FIUNET_ERR_INVALID_ARG, "channels not a plane multiple");
    if (mode == SRC_CONCAT_UP && epi == EPI_PLAIN) return launch_conv_shape<T, SRC_CONCAT_UP, EPI_PLAIN>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_PLAIN) return launch_conv_shape<T, SRC_DIRECT, EPI_PLAIN>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_HEAD) return launch_conv_shape<T, SRC_DIRECT, EPI_HEAD>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_HEAD3) return launch_conv_shape<T, SRC_DIRECT, EPI_HEAD3>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_POOL) return launch_conv_shape<T, SRC_DIRECT, EPI_POOL>(a, cfg, s);
    if constexpr (std::is_same_v<T, __bf16>) {   // FIUNET_BF16X2: two-piece operands
        if (mode == SRC_DIRECT_X2 && epi == EPI_PLAIN) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_PLAIN>(a, cfg, s);
        if (mode == SRC_DIRECT_X2 && epi == EPI_POOL) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_POOL>(a, cfg, s);
        if (mode == SRC_DIRECT_X2 && epi == EPI_HEAD) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_HEAD>(a, cfg, s);
        if (mode == SRC_DIRECT_X2 && epi == EPI_HEAD3) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_HEAD3>(a, cfg, s);
        if (mode == SRC_STEM_X2 && epi == EPI_POOL && a.Cout == 64)
            return cfg.small ? launch_conv_cfg<T, 64, 8, 32, SRC_STEM_X2, EPI_POOL>(a, s)
                             : launch_conv_cfg<T, 64, 16, 32, SRC_STEM_X2, EPI_POOL>(a, s);
    }
    if constexpr (sizeof(T) == 2) {   // the fused gray stem (bf16, fp16): 32-wide tiles only (the patch layout)
        if (mode == SRC_STEM && epi == EPI_POOL && a.Cout == 64)
            return cfg.small ? launch_conv_cfg<T, 64, 8, 32, SRC_STEM, EPI_POOL>(a, s)
                             : launch_conv_cfg<T, 64, 16, 32, SRC_STEM, EPI_POOL>(a, s);
    }
    return fail(FIUNET_ERR_INVALID_ARG, "unsupported gather/epilogue combination");
}

// The band [y_origin, y_origin + H) of an image of Hg rows (un-tiled: y_origin = 0, Hg = H), launched as the plan `p.st`
// says.  T = float (FIUNET_FP32), __bf16 (FIUNET_BF16, FIUNET_BF16X2) or _Float16 (FIUNET_FP16).
// FIUNET_FP16: the bf16 launch plan with IEEE half activations and weights (fiunet_prepare_precision builds the weight
// copies): the same kernels instantiated for _Float16 (v_mfma_f32_16x16x32_f16), every rounding to fp16 RNE and saturated,
// no stem dither; the stems keep the bf16 path's arithmetic (split-bf16 MFMAs / the exact fp32 kernel) and round to fp16.
// FIUNET_BF16X2: the fp32 contract on the bf16 pipe (include/fiunet.h).  Activations are two-piece bf16 tensors
// [hi planes | lo planes] (4 B per element), weights [wh | wl]; every conv is the bf16 direct kernel in mode
// SRC_DIRECT_X2 (three virtual planes per real plane: (xh, wh), (xh, wl) on the same in-tile, (xl, wh)), the stem is the
// exact-fp32 kernel with a splitting epilogue (no dither), the upsampled halves are always materialised
// (x2_upsample_kernel: fp32 interpolation of hi + lo; bilinear=False: convt2x2_kernel<bf16, X2>), the head is the usual
// fused fp32 reduction; no ablation path.
// u1/u2 (uint8 frames) replace f1/f2 only where the stem reads the frames itself (fused stem, RGB split stem); out_u8
// replaces out only where the head is fused into the last conv's epilogue (fiunet_forward_u8 decides)
template <typename T>
int forward_impl(fiunet_ctx* ctx, int precision, const float* f1, const float* f2, float* out, int B, int H, int W,
                 char* ws, const Plan& p, hipStream_t s, int y_origin, int Hg, const uint8_t* u1 = nullptr,
                 const uint8_t* u2 = nullptr, uint8_t* out_u8 = nullptr,
                 size_t out_img_stride = 0 /* elements between images of out / out_u8; 0 = contiguous */)
{
    const bool x2 = precision == FIUNET_BF16X2, bf16 = precision == FIUNET_BF16, f16 = precision == FIUNET_FP16;
    if (x2 && !ctx->x2_ready)
        return fail(FIUNET_ERR_NOT_LOADED, "precision bf16x2: call fiunet_prepare_precision(ctx, FIUNET_BF16X2) after "
                                           "fiunet_load_weights (it builds the two-piece weight copies)");
    if (f16 && !ctx->f16_ready)
        return fail(FIUNET_ERR_NOT_LOADED, "precision fp16: call fiunet_prepare_precision(ctx, FIUNET_FP16) after "
                                           "fiunet_load_weights (it builds the fp16 weight copies)");
    const StageLaunch* L = p.st;
    const size_t es = x2 ? 4 : sizeof(T);   // bytes per activation element
    int hg[5];  // rows of the whole image at each pyramid level (floor halving, unet.py:28)
    hg[0] = Hg;
    for (int l = 1; l < 5; ++l) hg[l] = hg[l - 1] / 2;
    auto act = [&](int i) { return ws + p.act_off[i]; };

    // optional per-layer timing: event e[0] before the stem, e[i+1] after stage i
    hipEvent_t* ev = nullptr;
    if (ctx->profiling) {
        if (ctx->ev_used + NCONV + 1 > ctx->ev_pool.size()) {
            const size_t old = ctx->ev_pool.size();
            ctx->ev_pool.resize(old + 64 * (NCONV + 1));
            for (size_t k = old; k < ctx->ev_pool.size(); ++k) HIP_TRY(hipEventCreate(&ctx->ev_pool[k]));
        }
        ev = ctx->ev_pool.data() + ctx->ev_used;
        ctx->ev_used += NCONV + 1;
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    // bf16 only: ordered input dither of the stem (conv3x3_mfma.hip.h, stem_dither); 2^-8 = a quarter of
    // an 8-bit input step peak to peak
    const float dither = bf16 && !(ctx->flags & FIUNET_OPT_NO_DITHER) ? 0.00390625f : 0.f;
    const ConvWeights& c0 = ctx->conv[0];
    const double stem_flops = 2.0 * B * H * W * 9.0 * c0.cin * c0.cout;
    if (L[0].form == STEM_RGB_SPLIT) {
        // RGB: split-bf16 MFMA stem (pointwise.hip.h), also on the ablation path (all 18 stage outputs of the RGB bf16
        // network stay bit-identical fused vs unfused); bf16x2 with a two-piece epilogue (the exact-fp32 MFMA stem needs 56
        // fp32 MFMAs per 16 pixels: it was the longest stage of the RGB network); it reads the uint8 frames itself on the
        // video path.  Persistent workgroups, one tile after the other: exactly as many as are resident at once
        // (FIUNET_RGB_STEM_OCC = 2 per CU, the kernel's __launch_bounds__: 176 registers); with more than that the surplus
        // ran a second round on a fraction of the chip
        const long long ntiles = (long long)B * ((H + 15) / 16) * ((W + 31) / 32);
        const dim3 g2((unsigned)std::min<long long>(ntiles, 256 * FIUNET_RGB_STEM_OCC));
        if (x2)
            hipLaunchKernelGGL(stem_rgb_split_kernel<true>, g2, dim3(256), 0, s, f1, f2, (const float*)c0.w_f32, c0.scale,
                               c0.shift, (__bf16*)act(0), B, H, W, dither, u1, u2);
        else if (f16)
            hipLaunchKernelGGL((stem_rgb_split_kernel<false, _Float16>), g2, dim3(256), 0, s, f1, f2, (const float*)c0.w_f32, c0.scale,
                               c0.shift, (_Float16*)act(0), B, H, W, 0.f, u1, u2);
        else
            hipLaunchKernelGGL(stem_rgb_split_kernel<false>, g2, dim3(256), 0, s, f1, f2, (const float*)c0.w_f32, c0.scale,
                               c0.shift, (__bf16*)act(0), B, H, W, dither, u1, u2);
        HIP_TRY(hipGetLastError());
    } else if (L[0].form == STEM_FIRST) {   // the exact fp32 stem kernel (bf16x2: its epilogue splits into the two pieces)
        const long long nruns = (long long)B * H * (((W + 15) / 16 + 7) / 8);  // 8-tile row runs
        const dim3 grid((unsigned)std::min<long long>((nruns + 3) / 4, 256 * 64));
        if (x2)
            hipLaunchKernelGGL((conv3x3_first_kernel<__bf16, 1, true>), grid, dim3(256), 0, s, f1, f2, (const float*)c0.w_f32,
                               c0.scale, c0.shift, (__bf16*)act(0), B, H, W, dither);
        else if (ctx->cf == 1)
            hipLaunchKernelGGL((conv3x3_first_kernel<T, 1>), grid, dim3(256), 0, s, f1, f2, (const float*)c0.w_f32, c0.scale,
                               c0.shift, (T*)act(0), B, H, W, dither);
        else if constexpr (sizeof(T) == 4)   // (RGB bf16 runs the split stem)
            hipLaunchKernelGGL((conv3x3_first_kernel<T, 3>), grid, dim3(256), 0, s, f1, f2, (const float*)c0.w_f32, c0.scale,
                               c0.shift, (T*)act(0), B, H, W, dither);
        HIP_TRY(hipGetLastError());
    }
    if (ev) {
        HIP_TRY(hipEventRecord(ev[1], s));
        if (L[0].form == STEM_FUSED) ctx->layer_name[0] = "(stem fused into next stage)";
        else if (x2) ctx->layer_name[0] = L[0].form == STEM_FIRST ? "conv3x3_first_kernel<f32 arithmetic, two-piece output>"
                                                                  : "stem_rgb_split_kernel<two-piece output>";
        else ctx->layer_name[0] = L[0].form == STEM_FIRST ? std::string("conv3x3_first_kernel<") + elem_name<T>() + "," +
                                                                std::to_string(ctx->cf) + ">"
                                                          : std::string(f16 ? "stem_rgb_split_kernel<fp16 output>" : "stem_rgb_split_kernel");
        ctx->layer_flops[0] = L[0].form == STEM_FUSED ? 0.0 : stem_flops;
    }
    for (int i = 1; i < NCONV; ++i) {
        const StageLaunch& st = L[i];
        const ConvWeights& cw = ctx->conv[i];
        const int lv = kLevel[i];
        ConvArgs a;
        std::memset(&a, 0, sizeof(a));
        a.B = B; a.H = p.hs[lv]; a.W = p.ws[lv];
        a.Cout = cw.cout;
        a.wgt = x2 ? cw.w_x2 : bf16 ? cw.w_bf16 : f16 ? cw.w_f16 : cw.w_f32;
        a.scale = cw.scale; a.shift = cw.shift;
        a.relu = 1;
        a.ksplit = 1;
        a.kslab = st.slab ? (float*)(ws + p.slab_off) : nullptr;
        a.stamp = (ctx->stamps && i == ctx->stamp_layer) ? ctx->stamps : nullptr;
        a.stamp_cap = (unsigned)kStampWaves;
        a.dst = st.stored ? act(i) : nullptr;
        a.src0 = act(kSrc0[i]);
        a.C0 = ctx->cout[kSrc0[i]];   // (bf16x2: REAL channels: the kernel knows both pieces of a tensor)
        int mode = x2 ? SRC_DIRECT_X2 : SRC_DIRECT;
        if (st.form == FORM_POOL) {
            // MaxPool2d(2) of the source (unet.py:28): already materialised by the producer's
            // epilogue (EPI_POOL), or by maxpool2_kernel right here on the ablation path
            char* pooled = ws + p.pool_off[lv - 1];
            if (L[i - 1].epi != EPI_POOL) {
                const size_t n = (size_t)B * a.H * a.W * (a.C0 * sizeof(T) / 16);
                hipLaunchKernelGGL((maxpool2_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s,
                                   (const T*)a.src0, (T*)pooled, B, p.hs[lv - 1], p.ws[lv - 1], a.C0);
                HIP_TRY(hipGetLastError());
            }
            a.src0 = pooled;
        } else if (kMode[i] == SRC_CONCAT_UP) {
            a.src1 = act(kSrc1[i]);
            a.C1 = ctx->cout[kSrc1[i]];
            a.lowH = p.hs[lv + 1]; a.lowW = p.ws[lv + 1];
            // vertical mapping in whole-image coordinates (a band starts at a multiple of 16 rows,
            // so its level-l tensors start at global row y_origin >> l)
            a.lowHg = hg[lv + 1];
            a.upOffY = y_origin >> lv;
            a.lowOffY = y_origin >> (lv + 1);
            const int dy = hg[lv] - 2 * a.lowHg, dx = a.W - 2 * a.lowW;  // unet.py:49-53
            a.padT = dy / 2; a.padL = dx / 2;
            // aten area_pixel_compute_scale, align_corners=True: (in - 1) / (out - 1) in fp32
            a.sy = 2 * a.lowHg > 1 ? (float)(a.lowHg - 1) / (float)(2 * a.lowHg - 1) : 0.f;
            a.sx = 2 * a.lowW > 1 ? (float)(a.lowW - 1) / (float)(2 * a.lowW - 1) : 0.f;
            char* up = ws + p.up_off[i];
            if (st.form == FORM_CONCAT_CONVT) {
                // bilinear=False (unet.py:42-44): ConvTranspose2d(C, C / 2, 2, 2) of the low-res tensor + F.pad, written once
                // as a full-resolution tensor; the conv then gathers two full-resolution sources (skip planes, then these)
                const auto& ct = ctx->convt[(i - 10) / 2];
                ConvTArgs c;
                std::memset(&c, 0, sizeof(c));
                c.low = a.src1; c.wgt = x2 ? ct.w_x2 : bf16 ? ct.w_bf16 : f16 ? ct.w_f16 : ct.w_f32; c.bias = ct.bias; c.dst = up;
                c.B = B; c.H = a.H; c.W = a.W; c.lowH = a.lowH; c.lowW = a.lowW; c.Cin = ct.cin; c.Cout = ct.cout;
                c.padT = a.padT; c.padL = a.padL; c.upOffY = a.upOffY; c.lowOffY = a.lowOffY; c.lowHg = a.lowHg;
                if (a.C1 != ct.cin) return fail(FIUNET_ERR_INVALID_ARG, "internal: transposed-conv channel plan mismatch");
                if (y_origin != 0 || Hg != H || a.H != 2 * a.lowH || a.W != 2 * a.lowW)   // F.pad rows / columns (and a band's edges)
                    if (int rc = zero_fill_async(up, (size_t)B * a.H * a.W * ct.cout * es, s)) return rc;
                const long long units = (long long)B * a.lowH * ((a.lowW + 31) / 32) * (ct.cout / 64);   // 32 pixels per wave
                const dim3 grid((unsigned)std::min<long long>((units + 3) / 4, 256 * 16));
                if (x2) {
                    if constexpr (std::is_same_v<T, __bf16>) hipLaunchKernelGGL((convt2x2_kernel<T, true>), grid, dim3(256), 0, s, c);
                } else
                    hipLaunchKernelGGL((convt2x2_kernel<T>), grid, dim3(256), 0, s, c);
                HIP_TRY(hipGetLastError());
                a.src1 = up; a.C1 = ct.cout;
            } else if (st.form == FORM_CONCAT_UPCAT) {
                T* scratch = (T*)(ws + p.scratch_off);
                const size_t n = (size_t)B * a.H * a.W * ((a.C0 + a.C1) * sizeof(T) / 16);
                hipLaunchKernelGGL((upcat_kernel<T>), dim3(grid_for(n)), dim3(256), 0, s, a, scratch);
                HIP_TRY(hipGetLastError());
                a.src0 = scratch; a.C0 = a.C0 + a.C1; a.C1 = 0; a.src1 = nullptr;
            } else if (st.form == FORM_CONCAT_UP) {   // two full-resolution sources: skip planes, then these
                const dim3 grid((unsigned)((a.W * 4 + 255) / 256), (unsigned)((a.H + UPS_ROWS - 1) / UPS_ROWS),
                                (unsigned)(B * (a.C1 / Elem<T>::PL)));
                // (grid.y, grid.z <= 65535: make_plan refuses a shape that would pass it)
                if (x2)
                    hipLaunchKernelGGL(x2_upsample_kernel, grid, dim3(256), 0, s, a, up);
                else
                    hipLaunchKernelGGL((upsample_kernel<T>), grid, dim3(256), 0, s, a, (T*)up);
                HIP_TRY(hipGetLastError());
                a.src1 = up;
            } else
                mode = SRC_CONCAT_UP;
        } else if (st.form == FORM_STEM) {   // the stem's output exists only as this conv's LDS tiles
            mode = x2 ? SRC_STEM_X2 : SRC_STEM;
            a.f1 = f1; a.f2 = f2;
            a.u1 = u1; a.u2 = u2;
            a.stem_w = ctx->stem_w_split;
            a.dither = dither;
        }
        if (a.C0 + a.C1 != cw.cin) return fail(FIUNET_ERR_INVALID_ARG, "internal: channel plan mismatch");
        if (st.epi == EPI_POOL) a.pool_dst = ws + p.pool_off[kPoolOut[i]];
        if (st.epi == EPI_HEAD || st.epi == EPI_HEAD3) {
            a.head_w = ctx->head_w; a.head_b = ctx->head_b; a.head_out = out; a.head_out_u8 = out_u8; a.head_nc = ctx->cf;
            a.head_img_stride = out_img_stride ? out_img_stride : (size_t)ctx->cf * H * W;
        }
        g_name_out = ev ? &ctx->layer_name[i] : nullptr;
        const int rc = launch_conv<T>(a, mode, st.epi, st.cfg, s);
        g_name_out = nullptr;
        if (rc != FIUNET_OK) return rc;
        if (ev) {
            ctx->layer_flops[i] = 2.0 * B * a.H * a.W * 9.0 * cw.cin * cw.cout;   // algorithmic (bf16x2 executes 3x)
            if (st.form == FORM_STEM && L[0].form == STEM_FUSED) ctx->layer_flops[i] += stem_flops;   // the fused stage does the stem's too
            if (i < NCONV - 1) HIP_TRY(hipEventRecord(ev[i + 1], s));
        }
    }
    if (L[NCONV - 1].epi == EPI_PLAIN) {   // the ablation path's OutConv
        const size_t n = (size_t)B * H * W;
        hipLaunchKernelGGL((head1x1_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                           (const T*)act(NCONV - 1), ctx->head_w, ctx->head_b, out, B, H, W, ctx->cf);
        HIP_TRY(hipGetLastError());
    }
    if (ev) HIP_TRY(hipEventRecord(ev[NCONV], s));
    return FIUNET_OK;
}

// the forward instantiation of a (valid) precision
auto forward_of(int precision)
{
    return precision == FIUNET_FP32 ? forward_impl<float> : precision == FIUNET_FP16 ? forward_impl<_Float16> : forward_impl<__bf16>;
}

NetDesc net_of(const fiunet_ctx* c)
{
    return NetDesc{c->cf, c->bilinear, c->cout, c->flags, c->stem_w_split != nullptr, c->force_tile, c->force_ksplit};
}

}  // namespace

extern "C" {

int fiunet_abi_version(void) { return FIUNET_ABI_VERSION; }

const char* fiunet_last_error_string(void) { return g_err.c_str(); }

int fiunet_create(fiunet_ctx** out_ctx, int device_id, int frame_channels, int bilinear)
{
    if (!out_ctx) return fail(FIUNET_ERR_INVALID_ARG, "out_ctx is NULL");
    *out_ctx = nullptr;
    if (frame_channels != 1 && frame_channels != 3)
        return fail(FIUNET_ERR_INVALID_ARG, "frame_channels must be 1 (gray) or 3 (RGB)");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(FIUNET_ERR_INVALID_ARG, "bad device_id");
    fiunet_ctx* c = new (std::nothrow) fiunet_ctx();
    if (!c) return fail(FIUNET_ERR_INVALID_ARG, "out of host memory");
    c->device = device_id;
    c->cf = frame_channels;
    c->bilinear = bilinear != 0;
    c->cout = c->bilinear ? kCoutBil : kCoutCT;
    *out_ctx = c;
    return FIUNET_OK;
}

int fiunet_destroy(fiunet_ctx* ctx)
{
    if (!ctx) return FIUNET_OK;
    (void)hipSetDevice(ctx->device);
    free_weights(ctx);
    if (ctx->load_done) (void)hipEventDestroy(ctx->load_done);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    delete ctx;
    return FIUNET_OK;
}

int fiunet_set_options(fiunet_ctx* ctx, unsigned flags)
{
    if (!ctx) return fail(FIUNET_ERR_INVALID_ARG, "ctx is NULL");
    ctx->flags = flags;
    return FIUNET_OK;
}

int fiunet_load_weights(fiunet_ctx* ctx, int n, const char* const* names,
                        const float* const* host_ptrs, const int64_t* numels)
{
    if (!ctx || n < 0 || !names || !host_ptrs || !numels)
        return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    std::map<std::string, std::pair<const float*, int64_t>> tab;
    for (int i = 0; i < n; ++i)
        if (names[i] && host_ptrs[i]) tab[names[i]] = {host_ptrs[i], numels[i]};
    auto get = [&](const std::string& k, int64_t want, const float** out) -> int {
        auto it = tab.find(k);
        if (it == tab.end()) return fail(FIUNET_ERR_MISSING_WEIGHT, "missing state-dict key " + k);
        if (it->second.second != want)
            return fail(FIUNET_ERR_MISSING_WEIGHT, "size mismatch for " + k + ": got " +
                            std::to_string(it->second.second) + ", want " + std::to_string(want));
        *out = it->second.first;
        return FIUNET_OK;
    };
    free_weights(ctx);
    const int cin0 = 2 * ctx->cf;
    const bool rne_weights = ctx->flags & FIUNET_OPT_RNE_WEIGHTS;  // read at LOAD time
    for (int i = 0; i < NCONV; ++i) {
        const int blk = i / 2, second = i % 2;
        const std::string pre = std::string(kBlockPrefix[blk]) + ".double_conv.";
        const std::string wk = pre + (second ? "3" : "0") + ".weight";
        const std::string bn = pre + (second ? "4" : "1");
        const int* kCout = ctx->cout;
        const int cout = kCout[i];
        const int cin = i == 0 ? cin0 : conv_cin(kCout, ctx->bilinear, i);
        const float *w, *g, *be, *mu, *var;
        int rc;
        if ((rc = get(wk, (int64_t)cout * cin * 9, &w))) return rc;
        if ((rc = get(bn + ".weight", cout, &g))) return rc;
        if ((rc = get(bn + ".bias", cout, &be))) return rc;
        if ((rc = get(bn + ".running_mean", cout, &mu))) return rc;
        if ((rc = get(bn + ".running_var", cout, &var))) return rc;
        ConvWeights& cw = ctx->conv[i];
        cw.cin = cin; cw.cout = cout;
        // eval-mode BatchNorm2d (eps = 1e-5, unet.py:13,16) folded to y = x*scale + shift
        std::vector<float> sc(cout), sh(cout);
        for (int c = 0; c < cout; ++c) {
            const float inv = 1.0f / std::sqrt(var[c] + 1e-5f);
            sc[c] = g[c] * inv;
            sh[c] = be[c] - mu[c] * sc[c];
        }
        if ((rc = dev_upload(ctx, sc.data(), cout * 4, (void**)&cw.scale))) return rc;
        if ((rc = dev_upload(ctx, sh.data(), cout * 4, (void**)&cw.shift))) return rc;
        if (i == 0) {  // stem: [tap][cin][64] fp32
            std::vector<float> pk((size_t)9 * cin * 64);
            for (int co = 0; co < 64; ++co)
                for (int ci = 0; ci < cin; ++ci)
                    for (int t = 0; t < 9; ++t)
                        pk[((size_t)t * cin + ci) * 64 + co] = w[((size_t)co * cin + ci) * 9 + t];
            if ((rc = dev_upload(ctx, pk.data(), pk.size() * 4, &cw.w_f32))) return rc;
            if (cin == 2) {  // fused-stem copy: w = hi + lo in bf16, [hi|lo][packed row][k]
                // packed row P = plane*32 + tile*16 + r holds cout bf16_row_to_cout(P), so that a lane of the
                // stem MFMAs ends up with 8 consecutive channels (one 16-B chunk of the in-tile record);
                // k = lane group*8 + dx*2 + frame with lane groups 0, 1, 2 <-> dy = 0, 2, 1 (LDS banks of the
                // patch reads, conv3x3_mfma.hip.h) and k = 24 = the BatchNorm shift (operand 1.0)
                std::vector<uint16_t> sp((size_t)2 * 64 * 32, 0);
                static const int kLaneGroupOfDy[3] = {0, 2, 1};
                for (int P = 0; P < 64; ++P) {
                    const int co = bf16_row_to_cout(P);
                    auto put = [&](int k, float v) {
                        const uint16_t hi = f32_to_bf16_rne(v);
                        uint32_t hb = (uint32_t)hi << 16;
                        float hf;
                        std::memcpy(&hf, &hb, 4);
                        sp[(size_t)P * 32 + k] = hi;
                        sp[(size_t)64 * 32 + P * 32 + k] = f32_to_bf16_rne(v - hf);
                    };
                    for (int dy = 0; dy < 3; ++dy)
                        for (int dx = 0; dx < 3; ++dx)
                            for (int f = 0; f < 2; ++f)  // BatchNorm scale folded in
                                put(kLaneGroupOfDy[dy] * 8 + dx * 2 + f, w[((size_t)co * 2 + f) * 9 + dy * 3 + dx] * sc[co]);
                    put(24, sh[co]);
                }
                if ((rc = dev_upload(ctx, sp.data(), sp.size() * 2, &ctx->stem_w_split))) return rc;
            }
            continue;
        }
        const size_t nel = (size_t)cout * cin * 9;
        std::vector<float> p32(nel);
        std::vector<uint16_t> p16(nel);
        for (int R = 0; R < cout; ++R) {  // R = packed row; fp32 rows are in natural cout order
            const int co16 = bf16_row_to_cout(R);
            double carry = 0.0;  // running sum of (exact - rounded) over this filter's bf16 weights
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < 9; ++t) {
                    // OIHW tap t = ky*3 + kx goes to packed slot kx*3 + ky: a kernel step is one
                    // (plane, kx) with its three ky taps contiguous (conv3x3_mfma.hip.h)
                    const int slot = (t % 3) * 3 + t / 3;
                    // BatchNorm's scale goes into the weights (one fp32 product, then the bf16
                    // rounding for the bf16 copy), its shift into the accumulators' initial value
                    p32[(((size_t)(ci / 16) * 9 + slot) * cout + R) * 16 + (ci % 16)] =
                        w[((size_t)R * cin + ci) * 9 + t] * sc[R];
                    const float wv = w[((size_t)co16 * cin + ci) * 9 + t] * sc[co16];
                    p16[(((size_t)(ci / 32) * 9 + slot) * cout + R) * 32 + (ci % 32)] =
                        rne_weights ? f32_to_bf16_rne(wv) : f32_to_bf16_feedback(wv, carry);
                }
        }
        if ((rc = dev_upload(ctx, p32.data(), nel * 4, &cw.w_f32))) return rc;
        if ((rc = dev_upload(ctx, p16.data(), nel * 2, &cw.w_bf16))) return rc;
    }
    if (!ctx->bilinear) {
        // ConvTranspose2d weights [Cin][Cout = Cin / 2][2][2] + bias (unet.py:43): packed per tap t = dy*2 + dx as
        // [t][Cin/PL][Cout][PL], the conv kernels' weight layout with 4 taps (rows in natural cout order; the bf16 copy
        // rounded to nearest - or with the per-filter error feedback, one filter = one (cout, tap))
        for (int k = 0; k < 4; ++k) {
            const int cin = ctx->cout[kSrc1[10 + 2 * k]], cout = cin / 2;
            const std::string pre = "unet.up" + std::to_string(k + 1) + ".up.";
            const float *w, *bi;
            int rc;
            if ((rc = get(pre + "weight", (int64_t)cin * cout * 4, &w))) return rc;
            if ((rc = get(pre + "bias", cout, &bi))) return rc;
            auto& ct = ctx->convt[k];
            ct.cin = cin; ct.cout = cout;
            const size_t nel = (size_t)4 * cin * cout;
            std::vector<float> p32(nel);
            std::vector<uint16_t> p16(nel);
            for (int t = 0; t < 4; ++t)
                for (int co = 0; co < cout; ++co) {
                    double carry = 0.0;
                    for (int ci = 0; ci < cin; ++ci) {
                        const float wv = w[((size_t)ci * cout + co) * 4 + t];
                        p32[(((size_t)t * (cin / 16) + ci / 16) * cout + co) * 16 + ci % 16] = wv;
                        p16[(((size_t)t * (cin / 32) + ci / 32) * cout + co) * 32 + ci % 32] =
                            rne_weights ? f32_to_bf16_rne(wv) : f32_to_bf16_feedback(wv, carry);
                    }
                }
            if ((rc = dev_upload(ctx, p32.data(), nel * 4, &ct.w_f32))) return rc;
            if ((rc = dev_upload(ctx, p16.data(), nel * 2, &ct.w_bf16))) return rc;
            if ((rc = dev_upload(ctx, bi, (size_t)cout * 4, (void**)&ct.bias))) return rc;
        }
    }
    {
        const float *w, *bi;
        int rc;
        if ((rc = get("unet.outc.conv.weight", (int64_t)ctx->cf * 64, &w))) return rc;
        if ((rc = get("unet.outc.conv.bias", ctx->cf, &bi))) return rc;
        if ((rc = dev_upload(ctx, w, (size_t)ctx->cf * 64 * 4, (void**)&ctx->head_w))) return rc;
        if ((rc = dev_upload(ctx, bi, (size_t)ctx->cf * 4, (void**)&ctx->head_b))) return rc;
#if defined(FIUNET_STAMP) || defined(FIUNET_CLOCK)
        {   // one 128-B record per wave of the largest launch (B=8 1080p: 32 640 workgroups); the kernels bound their index
            void* d = nullptr;
            HIP_TRY(hipMalloc(&d, kStampWaves * kStampRec * 8));
            ctx->owned.push_back(d);
            HIP_TRY(hipMemset(d, 0, kStampWaves * kStampRec * 8));
            ctx->stamps = (unsigned long long*)d;
        }
#endif
    }
    ctx->loaded = true;
    return FIUNET_OK;
}

int fiunet_load_weights_device(fiunet_ctx* ctx, int n, const char* const* names,
                               const float* const* device_ptrs, const int64_t* numels, void* stream)
{
    if (!ctx || n < 0 || !names || !device_ptrs || !numels)
        return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    std::map<std::string, std::pair<const float*, int64_t>> tab;
    for (int i = 0; i < n; ++i)
        if (names[i] && device_ptrs[i]) tab[names[i]] = {device_ptrs[i], numels[i]};
    auto get = [&](const std::string& k, int64_t want, const float** out) -> int {
        auto it = tab.find(k);
        if (it == tab.end()) return fail(FIUNET_ERR_MISSING_WEIGHT, "missing state-dict key " + k);
        if (it->second.second != want)
            return fail(FIUNET_ERR_MISSING_WEIGHT, "size mismatch for " + k + ": got " +
                            std::to_string(it->second.second) + ", want " + std::to_string(want));
        *out = it->second.first;
        return FIUNET_OK;
    };
    // 1. every key, in the host entry's order (the same first complaint), before anything on the context or the device
    //    changes: a failed call leaves the weights of the load before it in place
    WpTable t;
    std::memset(&t, 0, sizeof(t));
    const int* kCout = ctx->cout;
    int rc;
    for (int i = 0; i < NCONV; ++i) {
        const int blk = i / 2, second = i % 2;
        const std::string pre = std::string(kBlockPrefix[blk]) + ".double_conv.";
        const std::string wk = pre + (second ? "3" : "0") + ".weight";
        const std::string bn = pre + (second ? "4" : "1");
        WpConv& L = t.conv[i];
        L.cout = kCout[i];
        L.cin = i == 0 ? 2 * ctx->cf : conv_cin(kCout, ctx->bilinear, i);
        if ((rc = get(wk, (int64_t)L.cout * L.cin * 9, &L.w))) return rc;
        if ((rc = get(bn + ".weight", L.cout, &L.gamma))) return rc;
        if ((rc = get(bn + ".bias", L.cout, &L.beta))) return rc;
        if ((rc = get(bn + ".running_mean", L.cout, &L.mean))) return rc;
        if ((rc = get(bn + ".running_var", L.cout, &L.var))) return rc;
    }
    const float* ct_bias[4] = {nullptr, nullptr, nullptr, nullptr};
    t.nconvt = ctx->bilinear ? 0 : 4;
    for (int k = 0; k < t.nconvt; ++k) {
        WpConvT& L = t.convt[k];
        L.cin = kCout[kSrc1[10 + 2 * k]];
        L.cout = L.cin / 2;
        const std::string pre = "unet.up" + std::to_string(k + 1) + ".up.";
        if ((rc = get(pre + "weight", (int64_t)L.cin * L.cout * 4, &L.w))) return rc;
        if ((rc = get(pre + "bias", L.cout, &ct_bias[k]))) return rc;
    }
    const float *head_w, *head_b;
    if ((rc = get("unet.outc.conv.weight", (int64_t)ctx->cf * 64, &head_w))) return rc;
    if ((rc = get("unet.outc.conv.bias", ctx->cf, &head_b))) return rc;

    // 2. the prepared buffers: the ones a load before this one left (their sizes depend on the architecture alone, which a
    //    context keeps for life) - then nothing below allocates, frees or waits for the device - or new ones
    HIP_TRY(hipSetDevice(ctx->device));
    auto buf = [&](auto** p, size_t bytes) -> int {
        if (*p) return FIUNET_OK;
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, bytes));
        ctx->owned.push_back(d);
        *p = static_cast<std::remove_reference_t<decltype(*p)>>(d);
        return FIUNET_OK;
    };
    if (!ctx->load_done) HIP_TRY(hipEventCreateWithFlags(&ctx->load_done, hipEventDisableTiming));
    for (int i = 0; i < NCONV; ++i) {
        ConvWeights& cw = ctx->conv[i];
        WpConv& L = t.conv[i];
        const size_t nel = (size_t)9 * L.cin * L.cout;
        if ((rc = buf(&cw.scale, (size_t)L.cout * 4))) return rc;
        if ((rc = buf(&cw.shift, (size_t)L.cout * 4))) return rc;
        if ((rc = buf(&cw.w_f32, nel * 4))) return rc;
        if (i > 0 && (rc = buf(&cw.w_bf16, nel * 2))) return rc;
        L.scale = cw.scale; L.shift = cw.shift; L.w_f32 = (float*)cw.w_f32; L.w_bf16 = (uint16_t*)cw.w_bf16;
    }
    if (ctx->cf == 1) {
        if ((rc = buf(&ctx->stem_w_split, (size_t)2 * 64 * 32 * 2))) return rc;
        t.stem_split = (uint16_t*)ctx->stem_w_split;
    }
    for (int k = 0; k < t.nconvt; ++k) {
        auto& ct = ctx->convt[k];
        WpConvT& L = t.convt[k];
        const size_t nel = (size_t)4 * L.cin * L.cout;
        if ((rc = buf(&ct.w_f32, nel * 4))) return rc;
        if ((rc = buf(&ct.w_bf16, nel * 2))) return rc;
        if ((rc = buf(&ct.bias, (size_t)L.cout * 4))) return rc;
        L.w_f32 = (float*)ct.w_f32; L.w_bf16 = (uint16_t*)ct.w_bf16;
    }
    if ((rc = buf(&ctx->head_w, (size_t)ctx->cf * 64 * 4))) return rc;
    if ((rc = buf(&ctx->head_b, (size_t)ctx->cf * 4))) return rc;
#if defined(FIUNET_STAMP) || defined(FIUNET_CLOCK)
    if (!ctx->stamps) {
        if ((rc = buf(&ctx->stamps, kStampWaves * kStampRec * 8))) return rc;
        HIP_TRY(hipMemset(ctx->stamps, 0, kStampWaves * kStampRec * 8));
    }
#endif

    // 3. the kernels (weights.hip.h), asynchronous on `stream`.  From here on the buffers change: the copies a precision
    //    derives from them are stale exactly as after a host load (kept allocated: fiunet_prepare_precision packs into them)
    hipStream_t s = (hipStream_t)stream;
    ctx->loaded = false;
    ctx->x2_ready = false;
    ctx->f16_ready = false;
    for (int i = 0; i < NCONV; ++i) { ctx->conv[i].cin = t.conv[i].cin; ctx->conv[i].cout = t.conv[i].cout; }
    for (int k = 0; k < t.nconvt; ++k) { ctx->convt[k].cin = t.convt[k].cin; ctx->convt[k].cout = t.convt[k].cout; }
    const unsigned gy = (unsigned)(NCONV - 1 + t.nconvt);
    hipLaunchKernelGGL(wp_fold_bn_kernel, dim3(4, NCONV), dim3(256), 0, s, t);   // (cout <= 1024 = 4 x 256)
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(wp_pack_f32_kernel, dim3(512, gy + 1), dim3(256), 0, s, t);
    HIP_TRY(hipGetLastError());
    if (ctx->flags & FIUNET_OPT_RNE_WEIGHTS)  // read at LOAD time
        hipLaunchKernelGGL(wp_pack_bf16_rne_kernel, dim3(512, gy), dim3(256), 0, s, t);
    else   // (at most 1024 conv filters, 4 x 512 ConvTranspose2d filters in a layer = 32 x 64)
        hipLaunchKernelGGL(wp_pack_bf16_feedback_kernel, dim3(32, gy), dim3(64), 0, s, t);
    HIP_TRY(hipGetLastError());
    if (t.stem_split) {
        hipLaunchKernelGGL(wp_stem_split_kernel, dim3(1), dim3(64), 0, s, t);
        HIP_TRY(hipGetLastError());
    }
    for (int k = 0; k < t.nconvt; ++k)
        HIP_TRY(hipMemcpyAsync(ctx->convt[k].bias, ct_bias[k], (size_t)t.convt[k].cout * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->head_w, head_w, (size_t)ctx->cf * 64 * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctx->head_b, head_b, (size_t)ctx->cf * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipEventRecord(ctx->load_done, s));
    ctx->loaded = true;
    return FIUNET_OK;
}

int fiunet_prepare_precision(fiunet_ctx* ctx, int precision)
{
    if (!ctx) return fail(FIUNET_ERR_INVALID_ARG, "ctx is NULL");
    if (!valid_precision(precision)) return fail(FIUNET_ERR_INVALID_ARG, "bad precision");
    if (!ctx->loaded) return fail(FIUNET_ERR_NOT_LOADED, "fiunet_prepare_precision before fiunet_load_weights");
    if (precision == FIUNET_FP16) {
        if (ctx->f16_ready) return FIUNET_OK;
        HIP_TRY(hipSetDevice(ctx->device));
        // the packs below run on this device's null stream: behind a device-side load's kernels, whichever stream those are on
        if (ctx->load_done) HIP_TRY(hipStreamWaitEvent(nullptr, ctx->load_done, 0));
        // fp16 weights, packed on the device from the fp32 copy (BatchNorm scale folded in) like the bf16 copy: ~35 MB more
        auto pack16 = [&](const void* w32, int cin, int cout, int convt, void** out) -> int {
            const size_t n = (size_t)cin * (convt ? 4 : 9) * cout;
            void* d = *out;
            if (!d) {
                HIP_TRY(hipMalloc(&d, n * 2));
                ctx->owned.push_back(d);
                *out = d;
            }
            hipLaunchKernelGGL(f16_pack_weights_kernel, dim3(grid_for(n / 2)), dim3(256), 0, 0, (const float*)w32,
                               (unsigned*)d, cin, cout, convt);
            HIP_TRY(hipGetLastError());
            return FIUNET_OK;
        };
        int rc;
        for (int i = 1; i < NCONV; ++i)
            if ((rc = pack16(ctx->conv[i].w_f32, ctx->conv[i].cin, ctx->conv[i].cout, 0, &ctx->conv[i].w_f16))) return rc;
        if (!ctx->bilinear)
            for (int k = 0; k < 4; ++k)
                if ((rc = pack16(ctx->convt[k].w_f32, ctx->convt[k].cin, ctx->convt[k].cout, 1, &ctx->convt[k].w_f16))) return rc;
        HIP_TRY(hipDeviceSynchronize());
        ctx->f16_ready = true;
        return FIUNET_OK;
    }
    if (precision != FIUNET_BF16X2 || ctx->x2_ready) return FIUNET_OK;   // fp32 / bf16 copies are made by the load
    HIP_TRY(hipSetDevice(ctx->device));
    // the packs below run on this device's null stream: behind a device-side load's kernels, whichever stream those are on
    if (ctx->load_done) HIP_TRY(hipStreamWaitEvent(nullptr, ctx->load_done, 0));
    // two-piece weights [wh | wl], packed on the device from the fp32 copy (BatchNorm scale folded in): ~69 MB more
    // (a copy that a failed earlier attempt already allocated is packed again in place: a retry allocates nothing twice)
    auto pack = [&](const void* w32, int cin, int cout, int convt, void** out) -> int {
        const size_t n = (size_t)2 * cin * (convt ? 4 : 9) * cout;
        void* d = *out;
        if (!d) {
            HIP_TRY(hipMalloc(&d, n * 2));
            ctx->owned.push_back(d);
            *out = d;
        }
        hipLaunchKernelGGL(x2_pack_weights_kernel, dim3(grid_for(n)), dim3(256), 0, 0, (const float*)w32,
                           (unsigned short*)d, cin, cout, convt);
        HIP_TRY(hipGetLastError());
        return FIUNET_OK;
    };
    int rc;
    for (int i = 1; i < NCONV; ++i)
        if ((rc = pack(ctx->conv[i].w_f32, ctx->conv[i].cin, ctx->conv[i].cout, 0, &ctx->conv[i].w_x2))) return rc;
    if (!ctx->bilinear)
        for (int k = 0; k < 4; ++k)
            if ((rc = pack(ctx->convt[k].w_f32, ctx->convt[k].cin, ctx->convt[k].cout, 1, &ctx->convt[k].w_x2))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    ctx->x2_ready = true;
    return FIUNET_OK;
}

int fiunet_min_unsplit_batch(const fiunet_ctx* ctx, int H, int W, int precision)
{
    if (!ctx || H < 16 || W < 16 || !valid_precision(precision)) {
        g_err = "fiunet_min_unsplit_batch: bad arguments";
        return 0;
    }
    if (!ctx->loaded) {   // the plan depends on the loaded weights (the fused-stem copy)
        g_err = "fiunet_min_unsplit_batch before fiunet_load_weights";
        return 0;
    }
    // the stage plan the forwards launch: no stage cuts its K loop (the stem stages and conv 17 never do)
    StageLaunch L[NCONV];
    for (int B = 1; B <= 64; ++B) {
        plan_stages(net_of(ctx), precision, B, H, W, L);
        if (std::none_of(L + 1, L + NCONV, [](const StageLaunch& st) { return st.cfg.ksplit > 1 || st.cfg.kwave; })) return B;
    }
    return 65;
}

static bool ctx_plan(const fiunet_ctx* ctx, int B, int H, int W, int precision, Plan& p)
{
    return ctx && valid_precision(precision) && make_plan(net_of(ctx), B, H, W, precision, p);
}

size_t fiunet_workspace_bytes(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    Plan p;
    if (!ctx_plan(ctx, B, H, W, precision, p)) {
        g_err = "fiunet_workspace_bytes: bad arguments";
        if (ctx && valid_precision(precision)) g_err += std::string(" (") + g_plan_refusal + ")";
        return 0;
    }
    return p.total;
}

int fiunet_forward(fiunet_ctx* ctx, const float* frame1, const float* frame2, float* out, int B,
                   int H, int W, int precision, void* workspace, size_t workspace_bytes,
                   void* stream)
{
    return fiunet_forward_strip(ctx, frame1, frame2, out, B, H, W, 0, H, precision, workspace,
                                workspace_bytes, stream);
}

int fiunet_forward_strip(fiunet_ctx* ctx, const float* frame1, const float* frame2, float* out, int B,
                         int H, int W, int y_origin, int H_image, int precision, void* workspace,
                         size_t workspace_bytes, void* stream)
{
    if (!ctx || !frame1 || !frame2 || !out || !workspace)
        return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (y_origin < 0 || y_origin % 16 != 0 || H_image < H || y_origin > H_image - H)
        return fail(FIUNET_ERR_BAD_SHAPE, "strip: y_origin must be a multiple of 16 inside the image");
    if (y_origin + H != H_image && H % 16 != 0)
        return fail(FIUNET_ERR_BAD_SHAPE, "strip: rows must be a multiple of 16 unless it ends the image");
    if (!ctx->loaded) return fail(FIUNET_ERR_NOT_LOADED, "fiunet_forward before fiunet_load_weights");
    if (!valid_precision(precision)) return fail(FIUNET_ERR_INVALID_ARG, "bad precision");
    if (B < 1) return fail(FIUNET_ERR_INVALID_ARG, "B < 1");
    if (H < 16 || W < 16)
        return fail(FIUNET_ERR_BAD_SHAPE, "H and W must be >= 16 (four 2x2 max-pools)");
    Plan p;
    if (!make_plan(net_of(ctx), B, H, W, precision, p))
        return fail(FIUNET_ERR_BAD_SHAPE, g_plan_refusal);
    if (workspace_bytes < p.total) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    auto fwd = forward_of(precision);
    return fwd(ctx, precision, frame1, frame2, out, B, H, W, (char*)workspace, p, (hipStream_t)stream, y_origin, H_image,
               nullptr, nullptr, nullptr, 0);
}

// fiunet_forward_u8: which of the three fp32 frame buffers (frame1, frame2, output logits) a forward still needs - the
// frames only where the stem kernel is the exact one that reads fp32 (the fused stem and the RGB split stem read the uint8
// frames themselves), the logits only where the last activation is a tensor (the ablation path's separate head, the debug
// read-back): everywhere else the fused head writes uint8 itself.
static size_t u8_extra_bytes(const fiunet_ctx* ctx, const Plan& p, int B, int H, int W, bool* in_f32, bool* out_f32)
{
    *in_f32 = p.st[0].form == STEM_FIRST;
    *out_f32 = p.st[NCONV - 1].stored;
    return ((*in_f32 ? 2 : 0) + (*out_f32 ? 1 : 0)) * align256((size_t)B * ctx->cf * H * W * 4);
}

size_t fiunet_workspace_bytes_u8(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    Plan p;
    if (!ctx_plan(ctx, B, H, W, precision, p)) {
        g_err = "fiunet_workspace_bytes: bad arguments";
        return 0;
    }
    bool in_f32, out_f32;
    return p.total + u8_extra_bytes(ctx, p, B, H, W, &in_f32, &out_f32);
}

int fiunet_forward_u8(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, uint8_t* out,
                      int B, int H, int W, int precision, void* workspace, size_t workspace_bytes,
                      void* stream)
{
    return fiunet_forward_u8_strided(ctx, frame1, frame2, out, 0, B, H, W, precision, workspace, workspace_bytes, stream);
}

int fiunet_forward_u8_strided(fiunet_ctx* ctx, const uint8_t* frame1, const uint8_t* frame2, uint8_t* out,
                              size_t out_image_stride, int B, int H, int W, int precision, void* workspace,
                              size_t workspace_bytes, void* stream)
{
    if (!ctx || !frame1 || !frame2 || !out || !workspace)
        return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->loaded) return fail(FIUNET_ERR_NOT_LOADED, "fiunet_forward before fiunet_load_weights");
    Plan p;
    if (!ctx_plan(ctx, B, H, W, precision, p))
        return fail(H < 16 || W < 16 ? FIUNET_ERR_BAD_SHAPE : FIUNET_ERR_INVALID_ARG, "bad shape");
    const size_t base = p.total;
    bool in_f32, out_f32;
    const size_t extra_bytes = u8_extra_bytes(ctx, p, B, H, W, &in_f32, &out_f32);
    const size_t img = (size_t)ctx->cf * H * W;
    if (out_image_stride == 0) out_image_stride = img;
    if (out_image_stride < img) return fail(FIUNET_ERR_INVALID_ARG, "out_image_stride smaller than one image");
    const size_t n = (size_t)B * img, fb = align256(n * 4);
    if (workspace_bytes < base + extra_bytes) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    char* ws = (char*)workspace;
    char* extra = ws + base;
    float *a = nullptr, *b = nullptr, *o = nullptr;
    int rc;
    if (in_f32) {
        a = (float*)extra; b = (float*)(extra + fb); extra += 2 * fb;
        if ((rc = fiunet_preprocess_u8(frame1, a, n, stream))) return rc;
        if ((rc = fiunet_preprocess_u8(frame2, b, n, stream))) return rc;
    }
    if (out_f32) o = (float*)extra;
    HIP_TRY(hipSetDevice(ctx->device));
    // the fused head writes the (possibly strided) uint8 destination itself; the fp32 staging buffer is contiguous
    auto fwd = forward_of(precision);
    if ((rc = fwd(ctx, precision, a, b, o, B, H, W, ws, p, (hipStream_t)stream, 0, H, in_f32 ? nullptr : frame1,
                  in_f32 ? nullptr : frame2, out_f32 ? nullptr : out, out_f32 ? 0 : out_image_stride)))
        return rc;
    if (!out_f32) return FIUNET_OK;
    if (out_image_stride == img) return fiunet_postprocess_u8(o, out, n, stream);
    for (int i = 0; i < B; ++i)   // (ablation / read-back configurations only: one elementwise launch per image)
        if ((rc = fiunet_postprocess_u8(o + (size_t)i * img, out + (size_t)i * out_image_stride, img, stream))) return rc;
    return FIUNET_OK;
}

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
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > 65535) return fail(FIUNET_ERR_BAD_SHAPE, "bad frame shape");
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

// ---- 10-bit frames (ABI v7): uint16 samples, pre10 / post10 around the fp32 forward.  Strides are
//      counted in samples.
size_t fiunet_workspace_bytes_p10(const fiunet_ctx* ctx, int B, int H, int W, int precision)
{
    const size_t base = fiunet_workspace_bytes(ctx, B, H, W, precision);
    if (base == 0) return 0;
    return align256(base) + 3 * align256((size_t)B * ctx->cf * H * W * 4);
}

int fiunet_forward_p10(fiunet_ctx* ctx, const uint16_t* frame1, const uint16_t* frame2, uint16_t* out,
                       size_t out_image_stride, int B, int H, int W, int precision, void* workspace,
                       size_t workspace_bytes, void* stream)
{
    if (!frame1 || !frame2 || !out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (B < 1) return fail(FIUNET_ERR_INVALID_ARG, "B < 1");
    if (H < 16 || W < 16) return fail(FIUNET_ERR_BAD_SHAPE, "H and W must be >= 16 (four 2x2 max-pools)");
    if (!ctx) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->loaded) return fail(FIUNET_ERR_NOT_LOADED, "fiunet_forward before fiunet_load_weights");
    const size_t need = fiunet_workspace_bytes_p10(ctx, B, H, W, precision);
    if (need == 0) return fail(FIUNET_ERR_INVALID_ARG, "bad precision or shape");
    const size_t img = (size_t)ctx->cf * H * W, n = (size_t)B * img;
    if (out_image_stride == 0) out_image_stride = img;
    if (out_image_stride < img) return fail(FIUNET_ERR_INVALID_ARG, "out_image_stride smaller than one image");
    if (workspace_bytes < need) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    // [fiunet_forward's workspace | frame1 fp32 | frame2 fp32 | output logits fp32]
    const size_t base = align256(fiunet_workspace_bytes(ctx, B, H, W, precision)), fb = align256(n * 4);
    float* a = (float*)((char*)workspace + base);
    float* b = (float*)((char*)a + fb);
    float* o = (float*)((char*)b + fb);
    int rc;
    if ((rc = fiunet_preprocess_p10(frame1, a, n, stream))) return rc;
    if ((rc = fiunet_preprocess_p10(frame2, b, n, stream))) return rc;
    if ((rc = fiunet_forward(ctx, a, b, o, B, H, W, precision, workspace, base, stream))) return rc;
    if (out_image_stride == img) return fiunet_postprocess_p10(o, out, n, stream);
    for (int i = 0; i < B; ++i)   // images apart (the video loop's interleaved result): one elementwise launch each
        if ((rc = fiunet_postprocess_p10(o + (size_t)i * img, out + (size_t)i * out_image_stride, img, stream))) return rc;
    return FIUNET_OK;
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
// The caller's layout (NULL or zero fields = tight) -> the resolved one, refused before any launch where it cannot
// hold an H x W frame.  Every quantity in samples.
static int resolve_surface(const fiunet_surface_layout* l, int H, int W, ColourSurface* sf)
{
    const size_t Hc = (size_t)(H + 1) / 2, Wc = (size_t)(W + 1) / 2;
    sf->luma_pitch = l && l->luma_pitch ? l->luma_pitch : (size_t)W;
    sf->chroma_offset = l && l->chroma_offset ? l->chroma_offset : (size_t)H * W;
    sf->chroma_pitch = l && l->chroma_pitch ? l->chroma_pitch : 2 * Wc;
    sf->frame_stride = l && l->frame_stride ? l->frame_stride : i420_frame_bytes(H, W);
    const size_t big = (size_t)1 << 40;   // (keeps every product below in range)
    if (sf->luma_pitch > big || sf->chroma_pitch > big || sf->chroma_offset > big || sf->frame_stride > big)
        return fail(FIUNET_ERR_INVALID_ARG, "surface layout: a value above 2^40 samples");
    if (sf->luma_pitch < (size_t)W) return fail(FIUNET_ERR_INVALID_ARG, "surface layout: luma_pitch < W");
    if (sf->chroma_pitch < 2 * Wc) return fail(FIUNET_ERR_INVALID_ARG, "surface layout: chroma_pitch < 2*ceil(W/2)");
    if (sf->chroma_offset < (size_t)(H - 1) * sf->luma_pitch + W)
        return fail(FIUNET_ERR_INVALID_ARG, "surface layout: chroma_offset inside the luma plane");
    if (sf->frame_stride < sf->chroma_offset + (Hc - 1) * sf->chroma_pitch + 2 * Wc)
        return fail(FIUNET_ERR_INVALID_ARG, "surface layout: frame_stride does not cover the chroma plane");
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
    if ((rc = resolve_surface(layout, H, W, &sf))) return rc;
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
    if ((rc = resolve_surface(layout, H, W, &sf))) return rc;
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
            if (!rc && !(rc = resolve_surface(in_layout, H, W, &sf))) rc = resolve_surface(out_layout, H, W, &sf);
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
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > 65535) return fail(FIUNET_ERR_BAD_SHAPE, "bad frame shape");
    const size_t tight = yuv_frame_samples(format, H, W);
    if (!tight) return fail(FIUNET_ERR_INVALID_ARG, "format: not a fiunet_yuv_format");
    const size_t big = (size_t)1 << 40;   // (keeps every product below in range)
    if (row_pitch > big || frame_stride > big) return fail(FIUNET_ERR_INVALID_ARG, "yuv layout: a value above 2^40");
    if (yuv_is_packed(format)) {
        if (bits != 8) return fail(FIUNET_ERR_INVALID_ARG, "format: uyvy422 / yuyv422 are 8-bit formats");
        if (W & 1) return fail(FIUNET_ERR_INVALID_ARG, "uyvy422 / yuyv422 need an even width");
        const size_t row = 2 * (size_t)W;
        lay->row_pitch = row_pitch ? row_pitch : row;
        if (lay->row_pitch < row) return fail(FIUNET_ERR_INVALID_ARG, "yuv layout: row_pitch < 2*W");
        lay->frame_stride = frame_stride ? frame_stride : (size_t)H * lay->row_pitch;
        if (lay->frame_stride < (size_t)(H - 1) * lay->row_pitch + row)
            return fail(FIUNET_ERR_INVALID_ARG, "yuv layout: frame_stride does not cover the last row");
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
    g_err = "fiunet_workspace_bytes_yuv: bits must be 8 or 10";
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

// The caller's layout (NULL or zero fields = tight) -> the resolved one, refused before any launch where it cannot hold
// an H x W frame of bpp bytes per pixel.  Every quantity in bytes.
static int resolve_packed(const fiunet_packed_layout* l, int H, int W, int bpp, PackedLayout* pl)
{
    const size_t row = (size_t)W * bpp, big = (size_t)1 << 40;   // (keeps every product below in range)
    pl->row_pitch = l && l->row_pitch ? l->row_pitch : row;
    if (pl->row_pitch > big) return fail(FIUNET_ERR_INVALID_ARG, "packed layout: a value above 2^40 bytes");
    pl->frame_stride = l && l->frame_stride ? l->frame_stride : (size_t)H * pl->row_pitch;
    if (pl->frame_stride > big) return fail(FIUNET_ERR_INVALID_ARG, "packed layout: a value above 2^40 bytes");
    if (pl->row_pitch < row) return fail(FIUNET_ERR_INVALID_ARG, "packed layout: row_pitch < W*bpp");
    if (pl->frame_stride < (size_t)(H - 1) * pl->row_pitch + row)
        return fail(FIUNET_ERR_INVALID_ARG, "packed layout: frame_stride does not cover the last row");
    return FIUNET_OK;
}

static int check_packed_args(const void* in, const void* out, int B, int H, int W, int format)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!packed_bpp(format)) return fail(FIUNET_ERR_INVALID_ARG, "format: not a fiunet_packed_format");
    if (B < 1 || H < 1 || W < 1 || B > 65535 || H > 65535) return fail(FIUNET_ERR_BAD_SHAPE, "bad frame shape");
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
        g_err = "fiunet_metrics_workspace_bytes: bad arguments";
        return 0;
    }
    const size_t tiles = (H >= SSIM_WIN && W >= SSIM_WIN) ? (size_t)ssim_tiles(H, W, nullptr) : 0;
    return align256((size_t)images * 8) + align256((size_t)images * tiles * 8);
}

int fiunet_psnr_u8(const uint8_t* pred, const uint8_t* target, int images, int H, int W, double* out,
                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (!pred || !target || !out || !workspace) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (images < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_BAD_SHAPE, "bad image shape");
    if (images > 65535) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 planes per call");
    if (workspace_bytes < align256((size_t)images * 8)) return fail(FIUNET_ERR_WORKSPACE, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* sums = (unsigned long long*)workspace;
    const size_t n = (size_t)H * W;
    if (int rc = zero_fill_async(sums, (size_t)images * 8, s)) return rc;
    // ~4 x 16 B per thread and at most 128 workgroups (= atomics) per image
    const unsigned bx = (unsigned)std::min<size_t>((n / 64 + 255) / 256 + 1, 128);
    hipLaunchKernelGGL(sqdiff_u8_kernel, dim3(bx, (unsigned)images), dim3(256), 0, s, pred, target, n, sums);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(psnr_finalize_kernel, dim3((images + 63) / 64), dim3(64), 0, s, sums, n, out, images);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
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
    hipStream_t s = (hipStream_t)stream;
    int tx = 0;
    const int tiles = ssim_tiles(H, W, &tx);
    double* partial = (double*)((char*)workspace + align256((size_t)images * 8));
    hipLaunchKernelGGL(ssim_u8_kernel, dim3((unsigned)tiles, (unsigned)images), dim3(256), 0, s, pred, target,
                       H, W, tx, partial);
    HIP_TRY(hipGetLastError());
    const double count = (double)(H - 2 * SSIM_PAD) * (double)(W - 2 * SSIM_PAD);
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3((unsigned)images), dim3(256), 0, s, partial, tiles, count, out);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

size_t fiunet_plane_metrics_workspace_bytes(int images, int H, int W)
{
    if (images < 1 || H < 1 || W < 1) {
        g_err = "fiunet_plane_metrics_workspace_bytes: bad arguments";
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
    if (bits != 8 && bits != 10) return fail(FIUNET_ERR_INVALID_ARG, "bits must be 8 or 10");
    if (images < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_INVALID_ARG, "bad plane shape");
    if (images > 65535) return fail(FIUNET_ERR_INVALID_ARG, "more than 65535 planes per call");
    if (!pred_row) pred_row = (size_t)W;
    if (!target_row) target_row = (size_t)W;
    if (pred_row_pitch < pred_row || target_row_pitch < target_row)
        return fail(FIUNET_ERR_INVALID_ARG, "plane layout: row_pitch < W");
    const size_t limit = (size_t)1 << 40;
    if (pred_row_pitch > limit || target_row_pitch > limit || pred_image_stride > limit || target_image_stride > limit)
        return fail(FIUNET_ERR_INVALID_ARG, "plane layout: a value above 2^40 samples");
    if (images > 1 && (pred_image_stride < (size_t)(H - 1) * pred_row_pitch + pred_row ||
                       target_image_stride < (size_t)(H - 1) * target_row_pitch + target_row))
        return fail(FIUNET_ERR_INVALID_ARG, "plane layout: image_stride smaller than one plane");
    const size_t align = bits == 10 ? 1 : 0;
    if ((((uintptr_t)pred | (uintptr_t)target) & align) != 0)
        return fail(FIUNET_ERR_INVALID_ARG, "10-bit planes are 16-bit words: odd address");
    if (workspace_bytes < need) return fail(FIUNET_ERR_INVALID_ARG, "workspace too small");
    if ((uintptr_t)workspace & 255) return fail(FIUNET_ERR_INVALID_ARG, "workspace not 256-B aligned");
    return FIUNET_OK;
}

extern "C++" {   // (a template over the sample type, inside this file's extern "C" part)
template <typename T>
static int launch_plane_psnr(const void* pred, size_t ps, size_t pp, const void* target, size_t ts, size_t tp,
                             int images, int H, int W, unsigned long long* sums, hipStream_t s)
{
    // a plane whose rows follow each other on both sides is one run of H*W samples, cut into PLANE_SEG pieces
    // (a multiple of 16 bytes, so every piece of an aligned plane keeps the 16-byte path)
    const size_t n = (size_t)H * W;
    const bool flat = pp == (size_t)W && tp == (size_t)W;
    if (flat && (n + PLANE_SEG - 1) / PLANE_SEG > 0xffffffffull) return fail(FIUNET_ERR_INVALID_ARG, "plane too large");
    const unsigned rows = flat ? (unsigned)((n + PLANE_SEG - 1) / PLANE_SEG) : (unsigned)H;
    const unsigned w = flat ? (unsigned)PLANE_SEG : (unsigned)W;
    const unsigned w_last = flat ? (unsigned)(n - (size_t)(rows - 1) * PLANE_SEG) : (unsigned)W;
    const size_t pa = flat ? (size_t)PLANE_SEG : pp, pb = flat ? (size_t)PLANE_SEG : tp;
    // one wave per row and step, at most 128 workgroups (= atomics) per image
    const unsigned bx = std::min<unsigned>((rows + 3) / 4, 128u);
    hipLaunchKernelGGL(plane_sqdiff_kernel<T>, dim3(bx, (unsigned)images), dim3(256), 0, s, (const T*)pred, ps, pa,
                       (const T*)target, ts, pb, rows, w, w_last, sums);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_plane_psnr(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, const void* target,
                      size_t target_image_stride, size_t target_row_pitch, int bits, int images, int H, int W,
                      double* out_psnr, unsigned long long* out_sse, void* workspace, size_t workspace_bytes,
                      void* stream)
{
    const size_t need = images > 0 ? align256((size_t)images * 8) : 0;
    if (int rc = check_planes(pred, pred_image_stride, pred_row_pitch, target, target_image_stride, target_row_pitch,
                              bits, images, H, W, out_psnr, workspace, workspace_bytes, need))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* sums = (unsigned long long*)workspace;
    if (int rc = zero_fill_async(sums, (size_t)images * 8, s)) return rc;
    if (int rc = bits == 10 ? launch_plane_psnr<uint16_t>(pred, pred_image_stride, pred_row_pitch, target,
                                                          target_image_stride, target_row_pitch, images, H, W, sums, s)
                            : launch_plane_psnr<uint8_t>(pred, pred_image_stride, pred_row_pitch, target,
                                                         target_image_stride, target_row_pitch, images, H, W, sums, s))
        return rc;
    hipLaunchKernelGGL(plane_psnr_finalize_kernel, dim3((images + 63) / 64), dim3(64), 0, s, sums, (size_t)H * W,
                       bits == 10 ? 1023.0 : 255.0, out_psnr, out_sse, images);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
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
    hipStream_t s = (hipStream_t)stream;
    int tx = 0;
    const int tiles = ssim_tiles(H, W, &tx);
    double* partial = (double*)((char*)workspace + align256((size_t)images * 8));
    const dim3 grid((unsigned)tiles, (unsigned)images);
    if (bits == 10)
        hipLaunchKernelGGL(plane_ssim_kernel<uint16_t>, grid, dim3(256), 0, s, (const uint16_t*)pred, pred_image_stride,
                           pred_row_pitch, (unsigned)pred_step, (const uint16_t*)target, target_image_stride,
                           target_row_pitch, (unsigned)target_step, H, W, tx, partial);
    else
        hipLaunchKernelGGL(plane_ssim_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)pred, pred_image_stride,
                           pred_row_pitch, (unsigned)pred_step, (const uint8_t*)target, target_image_stride,
                           target_row_pitch, (unsigned)target_step, H, W, tx, partial);
    HIP_TRY(hipGetLastError());
    const double count = (double)(H - 2 * SSIM_PAD) * (double)(W - 2 * SSIM_PAD);
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3((unsigned)images), dim3(256), 0, s, partial, tiles, count, out_ssim);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_plane_ssim(const void* pred, size_t pred_image_stride, size_t pred_row_pitch, const void* target,
                      size_t target_image_stride, size_t target_row_pitch, int bits, int images, int H, int W,
                      double* out_ssim, void* workspace, size_t workspace_bytes, void* stream)
{
    return fiunet_stepped_ssim(pred, pred_image_stride, pred_row_pitch, 1, target, target_image_stride,
                                     target_row_pitch, 1, bits, images, H, W, out_ssim, workspace, workspace_bytes,
                                     stream);
}

extern "C++" {
template <typename T, int S>
static int launch_interleaved_sqdiff(const void* pred, size_t ps, size_t pp, const void* target, size_t ts, size_t tp,
                                     int images, int H, int W, unsigned long long* sums, hipStream_t s)
{
    // rows that follow each other on both sides are one run of H*W*S samples, cut into interleaved_seg(S) pieces (a
    // multiple of S and of 16 bytes: a piece starts at component 0 and an aligned run keeps the 16-byte path)
    constexpr size_t SEG = interleaved_seg(S);
    const size_t row = (size_t)W * S, n = (size_t)H * row;
    const bool flat = pp == row && tp == row;
    if (flat && (n + SEG - 1) / SEG > 0xffffffffull) return fail(FIUNET_ERR_INVALID_ARG, "plane too large");
    const unsigned rows = flat ? (unsigned)((n + SEG - 1) / SEG) : (unsigned)H;
    const unsigned len = flat ? (unsigned)SEG : (unsigned)row;
    const unsigned l_last = flat ? (unsigned)(n - (size_t)(rows - 1) * SEG) : (unsigned)row;
    const size_t pa = flat ? SEG : pp, pb = flat ? SEG : tp;
    const unsigned bx = std::min<unsigned>((rows + 3) / 4, 128u);
    hipLaunchKernelGGL((interleaved_sqdiff_kernel<T, S>), dim3(bx, (unsigned)images), dim3(256), 0, s, (const T*)pred, ps,
                       pa, (const T*)target, ts, pb, rows, len, l_last, sums);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

template <typename T>
static int launch_interleaved_psnr(int S, const void* pred, size_t ps, size_t pp, const void* target, size_t ts,
                                   size_t tp, int images, int H, int W, unsigned long long* sums, hipStream_t s)
{
    if (S == 2) return launch_interleaved_sqdiff<T, 2>(pred, ps, pp, target, ts, tp, images, H, W, sums, s);
    if (S == 3) return launch_interleaved_sqdiff<T, 3>(pred, ps, pp, target, ts, tp, images, H, W, sums, s);
    return launch_interleaved_sqdiff<T, 4>(pred, ps, pp, target, ts, tp, images, H, W, sums, s);
}
}  // extern "C++"

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
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* sums = (unsigned long long*)workspace;
    const int planes = images * components;
    if (int rc = zero_fill_async(sums, (size_t)planes * 8, s)) return rc;
    if (int rc = bits == 10 ? launch_interleaved_psnr<uint16_t>(components, pred, pred_image_stride, pred_row_pitch,
                                                                target, target_image_stride, target_row_pitch, images,
                                                                H, W, sums, s)
                            : launch_interleaved_psnr<uint8_t>(components, pred, pred_image_stride, pred_row_pitch,
                                                               target, target_image_stride, target_row_pitch, images, H,
                                                               W, sums, s))
        return rc;
    hipLaunchKernelGGL(plane_psnr_finalize_kernel, dim3((planes + 63) / 64), dim3(64), 0, s, sums, (size_t)H * W,
                       bits == 10 ? 1023.0 : 255.0, out_psnr, out_sse, planes);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
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
        g_err = "fiunet_ssim_gauss_workspace_bytes: bad arguments";
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

int fiunet_preprocess_u8(const uint8_t* in, float* out, size_t n, void* stream)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!n) return FIUNET_OK;
    hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_postprocess_u8(const float* in, uint8_t* out, size_t n, void* stream)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!n) return FIUNET_OK;
    hipLaunchKernelGGL(postprocess_u8_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_preprocess_p10(const uint16_t* in, float* out, size_t n, void* stream)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!n) return FIUNET_OK;
    hipLaunchKernelGGL(preprocess_p10_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_postprocess_p10(const float* in, uint16_t* out, size_t n, void* stream)
{
    if (!in || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (!n) return FIUNET_OK;
    hipLaunchKernelGGL(postprocess_p10_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, n);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

// ---- scene cuts (csrc/scene.hip.h) -------------------------------------------------------------
constexpr int kMaxGridY = 65535;   // pairs / intervals per launch (grid.y)

extern "C++" {   // (a template inside the extern "C" block)
template <typename T>
static int pair_sad(const T* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream)
{
    if (!frames || !sums) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (n_frames < 2 || frame_samples == 0) return FIUNET_OK;
    // ~4 x 16 B per thread and at most 128 workgroups (= atomics) per pair, as fiunet_psnr_u8
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int p0 = 0; p0 < n_frames - 1; p0 += kMaxGridY) {
        const int np = std::min(n_frames - 1 - p0, kMaxGridY);
        hipLaunchKernelGGL(pair_sad_kernel<T>, dim3(bx, (unsigned)np), dim3(kSceneBlock), 0, (hipStream_t)stream,
                           frames + (size_t)p0 * frame_samples, frame_samples,
                           reinterpret_cast<unsigned long long*>(sums + p0));
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_pair_sad_u8(const uint8_t* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream)
{
    return pair_sad(frames, n_frames, frame_samples, sums, stream);
}

int fiunet_pair_sad_p10(const uint16_t* frames, int n_frames, size_t frame_samples, int64_t* sums, void* stream)
{
    return pair_sad(frames, n_frames, frame_samples, sums, stream);
}

// repeated frames: the calling conventions of pair_sad
extern "C++" {
template <typename T>
static int pair_peak(const T* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream)
{
    if (!frames || !peaks) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (n_frames < 2 || frame_samples == 0) return FIUNET_OK;
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int p0 = 0; p0 < n_frames - 1; p0 += kMaxGridY) {
        const int np = std::min(n_frames - 1 - p0, kMaxGridY);
        hipLaunchKernelGGL(pair_peak_kernel<T>, dim3(bx, (unsigned)np), dim3(kSceneBlock), 0, (hipStream_t)stream,
                           frames + (size_t)p0 * frame_samples, frame_samples, peaks + p0);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_pair_peak_u8(const uint8_t* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream)
{
    return pair_peak(frames, n_frames, frame_samples, peaks, stream);
}

int fiunet_pair_peak_p10(const uint16_t* frames, int n_frames, size_t frame_samples, uint32_t* peaks, void* stream)
{
    return pair_peak(frames, n_frames, frame_samples, peaks, stream);
}

int fiunet_scene_cuts(const int64_t* sums, int n_frames, size_t count, int bits, double threshold, double* scores,
                      uint8_t* flags, void* stream)
{
    if (!sums || !scores || !flags) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (bits != 8 && bits != 10) return fail(FIUNET_ERR_INVALID_ARG, "bits must be 8 or 10");
    if (!(threshold > 0.0 && threshold <= 100.0)) return fail(FIUNET_ERR_INVALID_ARG, "threshold outside (0, 100]");
    if (count == 0) return fail(FIUNET_ERR_INVALID_ARG, "count == 0");
    if (n_frames < 2) return FIUNET_OK;
    const int intervals = n_frames - 1;
    hipLaunchKernelGGL(scene_cuts_kernel, dim3((unsigned)((intervals + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const long long*>(sums), intervals, (double)count,
                       (double)(1 << bits), threshold, scores, flags);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

int fiunet_hold_cut_frames(uint8_t* video, int n_frames, size_t frame_bytes, int factor, const uint8_t* flags,
                           void* stream)
{
    if (!video || !flags) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    if (factor < 2 || (factor & (factor - 1)) || factor > (1 << 20))
        return fail(FIUNET_ERR_INVALID_ARG, "factor must be a power of two in [2, 2^20]");
    if (n_frames < 2 || frame_bytes == 0) return FIUNET_OK;
    const unsigned gx = (unsigned)kHoldBlocks * (unsigned)(factor - 1);
    for (int i0 = 0; i0 < n_frames - 1; i0 += kMaxGridY) {
        const int ni = std::min(n_frames - 1 - i0, kMaxGridY);
        hipLaunchKernelGGL(hold_cut_frames_kernel, dim3(gx, (unsigned)ni), dim3(kSceneBlock), 0, (hipStream_t)stream,
                           video + (size_t)i0 * factor * frame_bytes, frame_bytes, factor, flags + i0);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}

// ---- frame-rate conversion (csrc/retime.hip.h) ---------------------------------------------------
extern "C++" {
template <typename T>
static int retime(const T* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval, uint64_t j0,
                  int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, T* out, void* stream)
{
    if (!grid || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_intervals < 0 || n_out < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (depth < 1 || depth > 4) return fail(FIUNET_ERR_INVALID_ARG, "depth outside 1..4");
    if (p == 0 || p >= q) return fail(FIUNET_ERR_INVALID_ARG, "need 0 < p < q");
    if (q > kRetimeMaxQ) return fail(FIUNET_ERR_INVALID_ARG, "q above 2^20");
    if (mode != 0 && mode != 1) return fail(FIUNET_ERR_INVALID_ARG, "mode must be 0 (blend) or 1 (nearest)");
    if (n_out == 0) return FIUNET_OK;
    // the first and the last requested frame lie in the grid (the times in between do, being monotonic); in 128 bits,
    // so that the kernel's 64-bit j * p cannot wrap
    const unsigned __int128 t0 = (unsigned __int128)j0 * p, t1 = ((unsigned __int128)j0 + (unsigned)(n_out - 1)) * p;
    if (t1 >> 64) return fail(FIUNET_ERR_INVALID_ARG, "frame index too large");
    const unsigned __int128 end = (unsigned __int128)first_interval + (unsigned)n_intervals;
    if (t0 / q < first_interval) return fail(FIUNET_ERR_INVALID_ARG, "first frame lies before the grid");
    if (t1 / q > end || (t1 / q == end && t1 % q != 0))
        return fail(FIUNET_ERR_INVALID_ARG, "last frame lies behind the grid");
    if (frame_samples == 0) return FIUNET_OK;
    // ~4 x 16 B per thread and at most 128 workgroups per frame, as fiunet_pair_sad_u8
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int k0 = 0; k0 < n_out; k0 += kMaxGridY) {
        const int nk = std::min(n_out - k0, kMaxGridY);
        hipLaunchKernelGGL(retime_kernel<T>, dim3(bx, (unsigned)nk), dim3(kRetimeBlock), 0, (hipStream_t)stream, grid,
                           frame_samples, depth, (unsigned long long)first_interval, (unsigned long long)(j0 + k0), p, q,
                           mode, flags, out + (size_t)k0 * frame_samples);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_retime_u8(const uint8_t* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval,
                     uint64_t j0, int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, uint8_t* out,
                     void* stream)
{
    return retime(grid, n_intervals, frame_samples, depth, first_interval, j0, n_out, p, q, mode, flags, out, stream);
}

int fiunet_retime_p10(const uint16_t* grid, int n_intervals, size_t frame_samples, int depth, uint64_t first_interval,
                      uint64_t j0, int n_out, uint32_t p, uint32_t q, int mode, const uint8_t* flags, uint16_t* out,
                      void* stream)
{
    return retime(grid, n_intervals, frame_samples, depth, first_interval, j0, n_out, p, q, mode, flags, out, stream);
}

// the table-driven form: every entry is checked here, on the host, before the first launch; the entries
// travel in the kernel's arguments, kRetimeTableMax output frames per launch
static_assert(sizeof(fiunet_retime_entry) == sizeof(RetimeEntry) && sizeof(RetimeEntry) == 12, "entry layout");

extern "C++" {
template <typename T>
static int retime_table(const T* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries, int n_out,
                        T* out, void* stream)
{
    if (!grid || !out) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (n_rows < 0 || n_out < 0) return fail(FIUNET_ERR_INVALID_ARG, "negative count");
    if (n_out == 0) return FIUNET_OK;
    if (!entries) return fail(FIUNET_ERR_INVALID_ARG, "NULL entries");
    for (int k = 0; k < n_out; ++k) {
        const fiunet_retime_entry& e = entries[k];
        if (e.den < 1 || e.den > kRetimeMaxQ) return fail(FIUNET_ERR_INVALID_ARG, "entry: den outside 1..2^20");
        if (e.wn >= e.den) return fail(FIUNET_ERR_INVALID_ARG, "entry: wn >= den");
        if ((uint64_t)e.row >= (uint64_t)n_rows) return fail(FIUNET_ERR_INVALID_ARG, "entry: row outside the grid");
        if (e.wn > 0 && (uint64_t)e.row + 1 >= (uint64_t)n_rows)
            return fail(FIUNET_ERR_INVALID_ARG, "entry: the row after `row` lies outside the grid");
    }
    if (frame_samples == 0) return FIUNET_OK;
    const unsigned bx = (unsigned)std::min<size_t>((frame_samples * sizeof(T) / 64 + 255) / 256 + 1, 128);
    for (int k0 = 0; k0 < n_out; k0 += kRetimeTableMax) {
        const int nk = std::min(n_out - k0, kRetimeTableMax);
        RetimeTable table = {};
        for (int k = 0; k < nk; ++k) table.e[k] = RetimeEntry{entries[k0 + k].row, entries[k0 + k].wn, entries[k0 + k].den};
        hipLaunchKernelGGL(retime_table_kernel<T>, dim3(bx, (unsigned)nk), dim3(kRetimeBlock), 0, (hipStream_t)stream,
                           grid, frame_samples, table, out + (size_t)k0 * frame_samples);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_retime_table_u8(const uint8_t* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries,
                           int n_out, uint8_t* out, void* stream)
{
    return retime_table(grid, n_rows, frame_samples, entries, n_out, out, stream);
}

int fiunet_retime_table_p10(const uint16_t* grid, int n_rows, size_t frame_samples, const fiunet_retime_entry* entries,
                            int n_out, uint16_t* out, void* stream)
{
    return retime_table(grid, n_rows, frame_samples, entries, n_out, out, stream);
}

// ---- resizing frame planes (csrc/resize.hip.h) ------------------------------------------------------
extern "C++" {
// the byte range [lo, hi) that n frames of the planes cover, from the buffer's first sample
static void resize_extent(const fiunet_resize_plane* planes, int n_planes, int n_frames, size_t& lo, size_t& hi)
{
    lo = SIZE_MAX, hi = 0;
    for (int i = 0; i < n_planes; ++i) {
        const fiunet_resize_plane& p = planes[i];
        const size_t end = p.offset + (size_t)(n_frames - 1) * p.frame_stride + (size_t)(p.h - 1) * p.pitch +
                           (size_t)(p.w - 1) * p.step + 1;
        lo = std::min(lo, p.offset), hi = std::max(hi, end);
    }
}

static const char* resize_check_plane(const fiunet_resize_plane& p)
{
    if (p.h < 1 || p.w < 1) return "a plane's h and w must be positive";
    if (p.h > kResizeMaxSize || p.w > kResizeMaxSize) return "a plane's h and w must not exceed 2^24";
    if (p.step < 1 || p.step > 4) return "a plane's step must be 1..4";
    if (p.pitch < (size_t)(p.w - 1) * p.step + 1) return "a plane's pitch must cover a row: (w - 1) * step + 1";
    // (h, w <= 2^24, step <= 4: the row term is below 2^26; the others are checked against wrapping)
    const size_t row = (size_t)(p.w - 1) * p.step + 1;
    if (p.h > 1 && p.pitch > (SIZE_MAX - row) / (size_t)(p.h - 1)) return "a plane's pitch is too large";
    const size_t body = (size_t)(p.h - 1) * p.pitch + row;
    if (p.offset > p.frame_stride || body > p.frame_stride - p.offset) return "a plane must lie inside its frame stride";
    return nullptr;
}

template <typename T>
static int resize_planes(const T* src, const fiunet_resize_plane* sp, T* dst, const fiunet_resize_plane* dp,
                         int n_planes, int n_frames, void* stream)
{
    if (!src || !dst || !sp || !dp) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    if (((uintptr_t)src | (uintptr_t)dst) % sizeof(T)) return fail(FIUNET_ERR_INVALID_ARG, "misaligned pointer");
    if (n_planes < 1 || n_planes > kResizeMaxPlanes) return fail(FIUNET_ERR_INVALID_ARG, "n_planes must be 1..4");
    if (n_frames < 0) return fail(FIUNET_ERR_INVALID_ARG, "n_frames < 0");
    constexpr int V = ResizeSample<T>::kVec;
    ResizeArgs base = {};
    unsigned long long per_frame_max = 0;
    for (int i = 0; i < n_planes; ++i) {
        for (const fiunet_resize_plane* p : {&sp[i], &dp[i]}) {
            if (const char* why = resize_check_plane(*p)) return fail(FIUNET_ERR_INVALID_ARG, why);
            // n frames of the plane stay inside the address space
            if (n_frames > 1 && p->frame_stride > (SIZE_MAX / sizeof(T)) / (size_t)n_frames)
                return fail(FIUNET_ERR_INVALID_ARG, "a plane's frame stride is too large");
        }
        ResizePlane& P = base.p[i];
        P.src_off = sp[i].offset, P.src_pitch = sp[i].pitch, P.src_fs = sp[i].frame_stride;
        P.dst_off = dp[i].offset, P.dst_pitch = dp[i].pitch, P.dst_fs = dp[i].frame_stride;
        P.sh = sp[i].h, P.sw = sp[i].w, P.dh = dp[i].h, P.dw = dp[i].w;
        P.sstep = sp[i].step, P.dstep = dp[i].step;
        P.sx = (double)P.sw / (double)P.dw, P.sy = (double)P.sh / (double)P.dh;
        P.chunks = (unsigned)((P.dw + V - 1) / V) + (P.dstep == 1 ? 1u : 0u);
        const unsigned long long per_frame = (unsigned long long)P.dh * P.chunks;
        if (per_frame >= (1ull << 31)) return fail(FIUNET_ERR_UNSUPPORTED, "a destination plane of 2^31 or more store chunks");
        per_frame_max = std::max(per_frame_max, per_frame);
    }
    if (n_frames == 0) return FIUNET_OK;
    size_t slo, shi, dlo, dhi;
    resize_extent(sp, n_planes, n_frames, slo, shi);
    resize_extent(dp, n_planes, n_frames, dlo, dhi);
    const uintptr_t s0 = (uintptr_t)src + slo * sizeof(T), s1 = (uintptr_t)src + shi * sizeof(T);
    const uintptr_t d0 = (uintptr_t)dst + dlo * sizeof(T), d1 = (uintptr_t)dst + dhi * sizeof(T);
    if (s0 < d1 && d0 < s1) return fail(FIUNET_ERR_INVALID_ARG, "source and destination overlap");
    // frames per launch: every plane's item count stays below 2^31
    const int batch = (int)std::min<unsigned long long>(((1ull << 31) - 1) / per_frame_max, (unsigned long long)n_frames);
    for (int f0 = 0; f0 < n_frames; f0 += batch) {
        const int nf = std::min(batch, n_frames - f0);
        ResizeArgs args = base;
        unsigned items_max = 0;
        for (int i = 0; i < n_planes; ++i) {
            ResizePlane& P = args.p[i];
            P.src_off += (size_t)f0 * P.src_fs, P.dst_off += (size_t)f0 * P.dst_fs;
            P.items = (unsigned)nf * (unsigned)P.dh * P.chunks;
            items_max = std::max(items_max, P.items);
        }
        // one item per thread up to 8192 workgroups (32 per CU), a grid-stride loop beyond
        const unsigned bx = std::min((items_max + kResizeBlock - 1) / kResizeBlock, 8192u);
        hipLaunchKernelGGL(resize_planes_kernel<T>, dim3(bx, (unsigned)n_planes), dim3(kResizeBlock), 0,
                           (hipStream_t)stream, src, dst, args);
        HIP_TRY(hipGetLastError());
    }
    return FIUNET_OK;
}
}  // extern "C++"

int fiunet_resize_planes_u8(const uint8_t* src, const fiunet_resize_plane* src_planes, uint8_t* dst,
                            const fiunet_resize_plane* dst_planes, int n_planes, int n_frames, void* stream)
{
    return resize_planes(src, src_planes, dst, dst_planes, n_planes, n_frames, stream);
}

int fiunet_resize_planes_p10(const uint16_t* src, const fiunet_resize_plane* src_planes, uint16_t* dst,
                             const fiunet_resize_plane* dst_planes, int n_planes, int n_frames, void* stream)
{
    return resize_planes(src, src_planes, dst, dst_planes, n_planes, n_frames, stream);
}

// diagnostic (not part of the ABI, no declaration in include/fiunet.h): override choose_conv_cfg for one conv (1..17) of
// this context - tile: 0 = choose, 1 = big, 2 = small, 3 = the in-workgroup K cut (conv3x3_kwave_kernel) where it applies; ksplit: 0 = choose, k >= 1 = cut the K loop k ways where the launch
// can be cut.  tools/cfg_sweep.py times every candidate of every layer with it; layer < 0 clears all overrides.
int fiunet_debug_force_cfg(fiunet_ctx* ctx, int layer, int tile, int ksplit)
{
    if (!ctx || layer >= NCONV || tile < 0 || tile > 3 || ksplit < 0 || ksplit > 32)
        return fail(FIUNET_ERR_INVALID_ARG, "fiunet_debug_force_cfg: bad arguments");
    if (layer < 0) {
        for (int i = 0; i < NCONV; ++i) ctx->force_tile[i] = ctx->force_ksplit[i] = 0;
        return FIUNET_OK;
    }
    ctx->force_tile[layer] = tile;
    ctx->force_ksplit[layer] = ksplit;
    return FIUNET_OK;
}

// diagnostic (not part of the ABI, no declaration in include/fiunet.h): where one prepared weight buffer lives and how
// many bytes it has, for comparing two contexts byte for byte (tests/test_gpu_weight_prep.py).  layer 0..17 = the convs,
// 18..21 = the ConvTranspose2d of up1..up4, 22 = the 1x1 head; which: 0 scale, 1 shift, 2 w_f32 (the head: its weight),
// 3 w_bf16, 4 stem_w_split (layer 0), 5 bias (ConvTranspose2d, head).  A buffer this context does not have (or a
// combination that names none) answers NULL and 0 bytes.
int fiunet_debug_weight_buffer(const fiunet_ctx* ctx, int layer, int which, const void** ptr, size_t* bytes)
{
    if (!ctx || !ptr || !bytes || layer < 0 || layer > NCONV + 4 || which < 0 || which > 5)
        return fail(FIUNET_ERR_INVALID_ARG, "fiunet_debug_weight_buffer: bad arguments");
    if (!ctx->loaded) return fail(FIUNET_ERR_NOT_LOADED, "fiunet_debug_weight_buffer before a load");
    const void* p = nullptr;
    size_t b = 0;
    if (layer < NCONV) {
        const ConvWeights& cw = ctx->conv[layer];
        const size_t nel = (size_t)9 * cw.cin * cw.cout;
        if (which == 0) { p = cw.scale; b = (size_t)cw.cout * 4; }
        else if (which == 1) { p = cw.shift; b = (size_t)cw.cout * 4; }
        else if (which == 2) { p = cw.w_f32; b = nel * 4; }
        else if (which == 3) { p = cw.w_bf16; b = nel * 2; }
        else if (which == 4 && layer == 0) { p = ctx->stem_w_split; b = (size_t)2 * 64 * 32 * 2; }
    } else if (layer < NCONV + 4) {
        const auto& ct = ctx->convt[layer - NCONV];
        const size_t nel = (size_t)4 * ct.cin * ct.cout;
        if (which == 2) { p = ct.w_f32; b = nel * 4; }
        else if (which == 3) { p = ct.w_bf16; b = nel * 2; }
        else if (which == 5) { p = ct.bias; b = (size_t)ct.cout * 4; }
    } else {
        if (which == 2) { p = ctx->head_w; b = (size_t)ctx->cf * 64 * 4; }
        else if (which == 5) { p = ctx->head_b; b = (size_t)ctx->cf * 4; }
    }
    *ptr = p;
    *bytes = p ? b : 0;
    return FIUNET_OK;
}

// diagnostic (not part of the ABI): the rule alone - what choose_conv_cfg answers for one conv of the bilinear network
// whose inputs the caller states (tests/test_cfg_rule.py); fiunet_debug_stage_cfg below answers what a forward launches.
// Pure host arithmetic, no device call.  out[0] = 1 small tile, out[1] = K slices over workgroups, out[2] = 1 in-workgroup K
// cut (conv3x3_kwave_kernel), out[3] = would a concat conv of this shape have its upsampled half materialised (stage index
// in `concat_stage`, 0 = n/a); a concat conv has the direct form exactly there, and `kwave_ok` then stands for that.
int fiunet_debug_choose_cfg(int precision, int B, int H, int W, int Cin, int Cout, int splittable, int concat_stage,
                            int kwave_ok, int* out /* [4] */)
{
    if (!out || B < 1 || H < 1 || W < 1 || Cin < 32 || (Cout != 64 && Cout % 128 != 0) || !valid_precision(precision))
        return fail(FIUNET_ERR_INVALID_ARG, "fiunet_debug_choose_cfg: bad arguments");
    const bool concat = concat_stage >= 10;
    out[3] = concat && concat_stage < NCONV && kMode[concat_stage] == SRC_CONCAT_UP &&
             (precision == FIUNET_BF16X2 ||
              materialise_up(precision, B, H, W, conv_cin(kCoutBil, true, concat_stage), kCoutBil[concat_stage]));
    const ConvCfg c = choose_conv_cfg(precision == FIUNET_FP32, precision == FIUNET_BF16X2, B, H, W, Cin, Cout, splittable != 0,
                                      -1, 0, concat ? out[3] != 0 : kwave_ok != 0, kwave_ok != 0,
                                      concat && !(precision == FIUNET_FP32 && out[3]));
    out[0] = c.small; out[1] = c.ksplit; out[2] = c.kwave;
    return FIUNET_OK;
}

// diagnostic (not part of the ABI): how stage `stage` (0 = the stem, 1..17 = the convs) of a forward of this architecture,
// option set, precision and shape launches - plan_stages itself, pure host arithmetic with no device call, so the launch
// rule (tile family, K cut, the batch-invariance gates) is testable without a GPU (tests/test_cfg_rule.py).  A gray network
// is taken with its fused-stem weights loaded, and without diagnostic overrides.
// out[0] = 1 small tile, out[1] = K slices over workgroups, out[2] = 1 in-workgroup K cut (conv3x3_kwave_kernel),
// out[3] = 1 the upsampled half is a tensor (upsample / ConvTranspose2d), out[4] = source form (SrcForm; stage 0: StemForm),
// out[5] = epilogue (EPI_*)
int fiunet_debug_stage_cfg(int frame_channels, int bilinear, unsigned flags, int precision, int B, int H, int W, int stage,
                           int* out /* [6] */)
{
    if (!out || (frame_channels != 1 && frame_channels != 3) || B < 1 || H < 16 || W < 16 || stage < 0 || stage >= NCONV ||
        !valid_precision(precision))
        return fail(FIUNET_ERR_INVALID_ARG, "fiunet_debug_stage_cfg: bad arguments");
    NetDesc n;
    n.cf = frame_channels;
    n.bilinear = bilinear != 0;
    n.cout = n.bilinear ? kCoutBil : kCoutCT;
    n.flags = flags;
    n.stem_w = frame_channels == 1;
    StageLaunch L[NCONV];
    plan_stages(n, precision, B, H, W, L);
    const StageLaunch& st = L[stage];
    out[0] = st.cfg.small; out[1] = st.cfg.ksplit; out[2] = st.cfg.kwave;
    out[3] = stage > 0 && (st.form == FORM_CONCAT_UP || st.form == FORM_CONCAT_CONVT);
    out[4] = st.form; out[5] = st.epi;
    return FIUNET_OK;
}

// diagnostic (not part of the ABI): the workspace plan of a forward of this architecture, option set, precision and shape -
// make_plan itself on the NetDesc fiunet_debug_stage_cfg builds, pure host arithmetic with no device call, so the layout
// (sizes, live intervals, the sharing of bytes) is testable without a GPU (tests/test_workspace_plan.py).  One record of six
// values per buffer make_plan placed, in placement order: kind (0 activation `index`, 1 MaxPool2d(2) of x1..x4 `index` 0..3,
// 2 the upsampled half of stage `index`, 3 the ablation path's concat scratch, 4 the split-K slab), index, offset, bytes,
// first stage, last stage (18 = still live after the last conv).  A stage that is not stored has no record.  *n_records =
// how many there are (also when `capacity` records do not hold them: FIUNET_ERR_INVALID_ARG, nothing written), *total =
// what fiunet_workspace_bytes answers.
int fiunet_debug_plan(int frame_channels, int bilinear, unsigned flags, int precision, int B, int H, int W,
                      long long* records /* [capacity][6] */, int capacity, int* n_records, unsigned long long* total)
{
    if (!records || capacity < 0 || !n_records || !total || (frame_channels != 1 && frame_channels != 3) || B < 1 || H < 16 ||
        W < 16 || !valid_precision(precision))
        return fail(FIUNET_ERR_INVALID_ARG, "fiunet_debug_plan: bad arguments");
    NetDesc n;
    n.cf = frame_channels;
    n.bilinear = bilinear != 0;
    n.cout = n.bilinear ? kCoutBil : kCoutCT;
    n.flags = flags;
    n.stem_w = frame_channels == 1;
    Plan p;
    std::vector<PlanBuf> bufs;
    if (!make_plan(n, B, H, W, precision, p, &bufs))
        return fail(FIUNET_ERR_BAD_SHAPE, std::string("fiunet_debug_plan: bad shape: ") + g_plan_refusal);
    *n_records = (int)bufs.size();
    *total = p.total;
    if (bufs.size() > (size_t)capacity)
        return fail(FIUNET_ERR_INVALID_ARG, "fiunet_debug_plan: " + std::to_string(bufs.size()) + " records, room for " +
                                                std::to_string(capacity));
    for (size_t k = 0; k < bufs.size(); ++k) {
        const PlanBuf& b = bufs[k];
        long long* r = records + 6 * k;
        r[0] = b.kind; r[1] = b.index; r[2] = (long long)*b.off; r[3] = (long long)b.bytes; r[4] = b.first; r[5] = b.last;
    }
    return FIUNET_OK;
}

#if defined(FIUNET_STAMP) || defined(FIUNET_CLOCK)
// diagnostic builds only (not part of the ABI): stamp ONE stage per forward; read = sums over waves
int fiunet_debug_stamp_layer(fiunet_ctx* ctx, int layer)
{
    ctx->stamp_layer = layer;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(ctx->stamps, 0, kStampWaves * kStampRec * 8));
    return FIUNET_OK;
}
int fiunet_debug_stamps(fiunet_ctx* ctx, unsigned long long* out /* [16] */)
{
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> h(kStampWaves * kStampRec);
    HIP_TRY(hipMemcpy(h.data(), ctx->stamps, kStampWaves * kStampRec * 8, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < kStampRec; ++k) out[k] = 0;
    for (size_t w = 0; w < kStampWaves; ++w)
        for (size_t k = 0; k < kStampRec; ++k) out[k] += h[w * kStampRec + k];
    return FIUNET_OK;
}
// the raw per-wave records ([kStampWaves][16] u64; record[8] != 0 where a wave wrote); returns the record count
int fiunet_debug_stamp_records(fiunet_ctx* ctx, unsigned long long* out, size_t max_records)
{
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = std::min(max_records, kStampWaves);
    HIP_TRY(hipMemcpy(out, ctx->stamps, n * kStampRec * 8, hipMemcpyDeviceToHost));
    return (int)n;
}
#endif

int fiunet_profile_enable(fiunet_ctx* ctx, int enable)
{
    if (!ctx) return fail(FIUNET_ERR_INVALID_ARG, "ctx is NULL");
    ctx->profiling = enable != 0;
    ctx->ev_used = 0;
    return FIUNET_OK;
}

int fiunet_profile_read(fiunet_ctx* ctx, int* n_forwards, float* avg_ms, double* flops,
                        char* names, int name_stride)
{
    if (!ctx || !avg_ms) return fail(FIUNET_ERR_INVALID_ARG, "NULL argument");
    const size_t nf = ctx->ev_used / (NCONV + 1);
    if (n_forwards) *n_forwards = (int)nf;
    for (int i = 0; i < NCONV; ++i) avg_ms[i] = 0.f;
    for (size_t f = 0; f < nf; ++f) {
        hipEvent_t* ev = ctx->ev_pool.data() + f * (NCONV + 1);
        HIP_TRY(hipEventSynchronize(ev[NCONV]));
        for (int i = 0; i < NCONV; ++i) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            avg_ms[i] += ms;
        }
    }
    for (int i = 0; i < NCONV; ++i) {
        if (nf) avg_ms[i] /= (float)nf;
        if (flops) flops[i] = ctx->layer_flops[i];
        if (names && name_stride > 0) {
            std::strncpy(names + (size_t)i * name_stride, ctx->layer_name[i].c_str(), name_stride - 1);
            names[(size_t)i * name_stride + name_stride - 1] = 0;
        }
    }
    ctx->ev_used = 0;
    return FIUNET_OK;
}

int fiunet_debug_read_activation(fiunet_ctx* ctx, const void* workspace, int B, int H, int W,
                                 int precision, int tap, float* dst, size_t dst_capacity, int out_dims[3], void* stream)
{
    if (!ctx || tap < 0 || tap >= NCONV + 4 || (dst && !workspace))
        return fail(FIUNET_ERR_INVALID_ARG, "bad argument");
    if (!valid_precision(precision)) return fail(FIUNET_ERR_INVALID_ARG, "bad precision");
    Plan p;
    if (dst && !(ctx->flags & FIUNET_OPT_KEEP_ALL))
        return fail(FIUNET_ERR_INVALID_ARG, "read-back needs FIUNET_OPT_KEEP_ALL set for the forward: without it "
                                            "activations share workspace bytes and are overwritten");
    if (!make_plan(net_of(ctx), B, H, W, precision, p))
        return fail(FIUNET_ERR_BAD_SHAPE, "bad shape");
    // channels of THIS architecture (the ConvTranspose2d decoder is wider than the bilinear one at taps 8, 9, 11, 13, 15)
    int C, lv;
    size_t off;
    if (tap < NCONV) {
        C = ctx->cout[tap]; lv = kLevel[tap]; off = p.act_off[tap];
    } else {   // taps 18..21: `self.up(x1)` + F.pad of up1..up4 (unet.py:47-53) where it is a tensor of its own
        const int i = 10 + 2 * (tap - NCONV);
        lv = kLevel[i];
        if (p.st[i].form != FORM_CONCAT_UP && p.st[i].form != FORM_CONCAT_CONVT)
            return fail(FIUNET_ERR_UNSUPPORTED, "read-back: the upsampled half of this stage is interpolated inside the "
                                                "conv's gather in this configuration, never stored");
        C = p.st[i].form == FORM_CONCAT_CONVT ? ctx->cout[kSrc1[i]] / 2 : ctx->cout[kSrc1[i]];
        off = p.up_off[i];
    }
    const int h = p.hs[lv], w = p.ws[lv];
    if (out_dims) { out_dims[0] = C; out_dims[1] = h; out_dims[2] = w; }
    if (!dst) return FIUNET_OK;   // dims-only query
    const size_t n = (size_t)B * C * h * w;
    if (dst_capacity < n)
        return fail(FIUNET_ERR_INVALID_ARG, "read-back: dst holds " + std::to_string(dst_capacity) + " floats, tap " +
                                            std::to_string(tap) + " has " + std::to_string(n));
    const char* src = (const char*)workspace + off;
    if (precision == FIUNET_BF16X2)
        hipLaunchKernelGGL(x2_to_nchw_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream,
                           (const __bf16*)src, dst, B, C, h, w);
    else if (precision == FIUNET_BF16)
        hipLaunchKernelGGL((nhwc_to_nchw_f32_kernel<__bf16>), dim3(grid_for(n)), dim3(256), 0,
                           (hipStream_t)stream, (const __bf16*)src, dst, B, C, h, w);
    else if (precision == FIUNET_FP16)
        hipLaunchKernelGGL((nhwc_to_nchw_f32_kernel<_Float16>), dim3(grid_for(n)), dim3(256), 0,
                           (hipStream_t)stream, (const _Float16*)src, dst, B, C, h, w);
    else
        hipLaunchKernelGGL((nhwc_to_nchw_f32_kernel<float>), dim3(grid_for(n)), dim3(256), 0,
                           (hipStream_t)stream, (const float*)src, dst, B, C, h, w);
    HIP_TRY(hipGetLastError());
    return FIUNET_OK;
}

// ---------------------------------------------------------------------------------------------------
// Farneback flow and flow-compensated warps (flow.hip.h).  The level arithmetic is
// optical_flow.py's: Python's round() is round-half-to-even, which rint() is in the default rounding mode (a
// 130-wide frame has a 32-wide level 2, not 33).
extern "C++" {
namespace {
constexpr int kFlowLevels = 3, kFlowMinSize = 32, kFlowIters = 3;
constexpr size_t kFlowMaxBatch = 4096, kFlowMaxSide = 32768;

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
    if (bits != 8 && bits != 10) return fail(FIUNET_ERR_INVALID_ARG, "bits must be 8 or 10");
    if (B < 1 || H < 1 || W < 1) return fail(FIUNET_ERR_INVALID_ARG, "bad frame shape");
    if ((size_t)B > kFlowMaxBatch || (size_t)H > kFlowMaxSide || (size_t)W > kFlowMaxSide)
        return fail(FIUNET_ERR_INVALID_ARG, "flow: more than 4096 pairs per call or a side above 32768");
    if (row_pitch < (size_t)W) return fail(FIUNET_ERR_INVALID_ARG, "frame layout: row_pitch < W");
    const size_t limit = (size_t)1 << 40;
    if (row_pitch > limit || image_stride > limit) return fail(FIUNET_ERR_INVALID_ARG, "frame layout: a value above 2^40 samples");
    if (B > 1 && image_stride < (size_t)(H - 1) * row_pitch + W)
        return fail(FIUNET_ERR_INVALID_ARG, "frame layout: image_stride smaller than one frame");
    if (bits == 10 && ((((uintptr_t)a | (uintptr_t)b) & 1) != 0))
        return fail(FIUNET_ERR_INVALID_ARG, "10-bit frames are 16-bit words: odd address");
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
        g_err = "fiunet_flow_workspace_bytes: bad arguments";
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
