// fiunet.hip -- C ABI (include/fiunet.h) + host orchestration of the MI355X UNet forward.
//
// Replaces, for the hot path only, the Python surface of the reference:
//   FrameInterpolationUNet.__init__/forward   /root/reference/model/unet.py:97-112
//   UNet.__init__/forward (wiring)            /root/reference/model/unet.py:65-95
//   load_state_dict + .to(device) + .eval()   /root/reference/model/inference.py:83-97
//   pre/post-processing arithmetic            /root/reference/model/inference.py:31-35, :54-61
// Device code: conv3x3_mfma.hip.h (MFMA implicit-GEMM conv) and pointwise.hip.h.
// gfx950 only; no CPU fallback: every entry point either launches HIP kernels or returns an error.
//
// One of the library's translation units (fiunet_internal.h lists them): this one holds the context, the weight loads,
// the stage and workspace plans, the forward and its entry points, and the one definition of the state the units share.
// The conv kernels are compiled in the conv units and launched through launch_conv (conv_launch.hip.h).
#include "fiunet_internal.h"
#include "pointwise.hip.h"
#include "weights.hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

using namespace fiunet;

namespace {

thread_local std::string g_err;

thread_local std::string* g_name_out = nullptr;  // where the next conv launch reports its kernel

}  // namespace

namespace fiunet {

std::string& last_error() { return g_err; }

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

std::string* name_out() { return g_name_out; }

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

}  // namespace fiunet

namespace {

constexpr size_t kSlabBytes = 64u << 20;  // split-K slab: ksplit * B*H*W*Cout * 4 <= ~50 MB by construction
[[maybe_unused]] constexpr size_t kStampWaves = 4 * 40000;  // diagnostic stamp records (128 B each); launches with more waves leave the rest unrecorded
[[maybe_unused]] constexpr size_t kStampRec = 16;              // u64 slots per record
// conv index = 2*block + {0,1}; blocks: inc, down1..4, up1..4 (state-dict order)
const char* const kBlockPrefix[9] = {
    "unet.inc", "unet.down1.maxpool_conv.1", "unet.down2.maxpool_conv.1",
    "unet.down3.maxpool_conv.1", "unet.down4.maxpool_conv.1", "unet.up1.conv", "unet.up2.conv",
    "unet.up3.conv", "unet.up4.conv"};
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

// (bf16_row_to_cout, f32_to_bf16_rne, f32_to_bf16_feedback: weights.hip.h - one definition for the host loop of
// fiunet_load_weights and the kernels of fiunet_load_weights_device)

// bf16 and fp16: one 2-byte element per activation and weight (32 channels per 64-B plane, the same MFMA shape), so both
// take every branch of the launch rule and the same workspace layout; fp32 and bf16x2 (two bf16 pieces) have 4 bytes
inline bool two_byte_elems(int p) { return p != FIUNET_FP32 && p != FIUNET_BF16X2; }

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
struct TileShape { int BN, TH, TW; };   // (ConvCfg, what the rule answers: fiunet_internal.h)

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

}  // extern "C"
