// conv3x3_mfma.hip.h -- fused 3x3 conv (pad 1, no bias) + per-channel scale/shift (eval BatchNorm)
// + ReLU as an implicit GEMM on the CDNA4 matrix cores, for gfx950 only.
//
// Replaces the aten conv2d + batch_norm + relu triple behind DoubleConv
// (/root/reference/model/unet.py:11-18) and, fused around it, the other ops of the UNet forward:
//   * MaxPool2d(2) of Down (unet.py:28)           -> EPI_POOL: the producer also writes the pooled copy
//   * Upsample + F.pad + torch.cat of Up (:46-54) -> SRC_CONCAT_UP: interpolated inside the gather
//   * OutConv 1x1 + bias (:60)                    -> EPI_HEAD / EPI_HEAD3: reduced in the epilogue
//   * the 2->64 stem conv (:72), bf16 / fp16 gray -> SRC_STEM: evaluated inside the gather
// so none of the pooled-input re-reads, upsampled, concatenated, stem-output or last-activation
// tensors is ever materialised in HBM.  The same kernel runs precision "bf16x2" (gather mode SRC_DIRECT_X2: two bf16
// pieces per activation and weight, three MFMAs per product - the reference's fp32 tolerance on the bf16 pipe).
//
// Mapping onto the hardware (one workgroup = 4 waves = 256 threads, 2 workgroups per CU):
//   * GEMM view: D[cout][pixel] += W[cout][k] * X[k][pixel], k = (channel plane, kx, ky).
//     MFMA A operand = weights (16 couts x 8k per lane-row), B operand = pixels.  With that
//     orientation a lane of the 16x16 accumulator holds consecutive couts of one pixel, so the
//     epilogue stores 16 contiguous bytes per lane into the blocked activation layout
//     [B][C/PL][H][W][PL] (see blk_off below).
//   * A "plane" is 64 bytes of channels per pixel (32 bf16 or 16 fp32).  The input tile
//     (TH+2)x(TW+2) pixels of one plane is staged in LDS ONCE and reused by all 9 taps -- the
//     shifted windows are just different LDS addresses (base + immediate offset).
//   * A step is one (plane, kx): its three taps ky = 0..2 read in-tile rows r, r+1, r+2 of the same
//     columns, so a wave fetches each (row, 16-pixel) fragment ONCE per step and uses it for up to
//     three taps (rolling window of ROWS_W + 2 rows): 24 instead of 36 ds_read_b128 per 96 MFMAs.
//   * Weights for (plane, kx, ky=0..2) are streamed per step: 3*BN rows of 64 B, by LDS-DMA
//     (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPRs) into a 2-deep ring, one
//     step ahead of the MFMAs, so the L2 latency of the weight stream hides under the previous
//     step's 96 MFMAs per wave.  The next plane's input tile is gathered at the plane boundary
//     behind one extra barrier (LDS-DMA for stored planes; LDS-staged bilinear interpolation or
//     the split-bf16 stem conv for computed ones); the co-resident second workgroup of the CU
//     covers that gap.
//   * Both LDS images are [row][64 B] with the 16-B chunk index XOR-ed by ((row>>2)&1)<<1, which
//     makes every ds_read_b128 of 16 consecutive rows x 4 chunks conflict-free for any row
//     alignment (the 16-lane groups of ds_read_b128 are listed in MI355X_MICROARCH.md, LDS).
//     The in-tile row pitch is padded to a multiple of 8 pixels so the swizzle term of a lane
//     does not depend on the tile row.
//   * Each wave owns 64 couts x 128 pixels = 4 x 8 accumulator tiles (128 VGPRs).
//   * bf16: v_mfma_f32_16x16x32_bf16 (one per A/B chunk pair); fp16: v_mfma_f32_16x16x32_f16 (same shape and operand
//     layout: the bf16 instantiations with IEEE half values); fp32: 4 x v_mfma_f32_16x16x4_f32
//     per chunk pair (exact fp32 FMA chain) -- same kernel body, same LDS images.
#pragma once
#include "conv_common.hip.h"

namespace fiunet {

template <typename T, int BN, int TH, int TW, int MODE, int EPI>
__global__ __launch_bounds__(256, conv_occupancy(BN, TH, TW, ConvTile<BN, TH, TW, MODE>::LDS_BYTES)) void conv3x3_mfma_kernel(const ConvArgs a)
{
    using Tile = ConvTile<BN, TH, TW, MODE>;
    constexpr int PL = Elem<T>::PL;
    constexpr int TWP = Tile::TWP, THP = Tile::THP;
    constexpr int WAVES_C = BN / 64, WAVES_P = 4 / WAVES_C;
    constexpr int FR = TW / 16;       // 16-pixel fragments per tile row
    constexpr int NF = conv_wave_frags(BN, TH, TW);  // fragments per wave
    constexpr int ROWS_W = NF / FR;   // tile rows per wave
    static_assert(NF == 8 || NF == 4, "wave tile must be 64 couts x 128 or 64 pixels");
    static_assert(TH == ROWS_W * WAVES_P && ROWS_W * FR == NF, "tile does not split over the waves");
    static_assert(EPI != EPI_POOL || ROWS_W % 2 == 0, "pooled epilogue: a wave owns whole row pairs");
    static_assert(Tile::LDS_BYTES * conv_occupancy(BN, TH, TW, Tile::LDS_BYTES) <= 160 * 1024, "LDS per CU");
    constexpr int HNC = EPI == EPI_HEAD ? 1 : (EPI == EPI_HEAD3 ? 3 : 0);  // fused-head classes
    static_assert(HNC == 0 || BN == 64, "fused head needs all 64 couts in one wave");
    static_assert(MODE == SRC_DIRECT || MODE == SRC_CONCAT_UP || MODE == SRC_STEM || MODE == SRC_DIRECT_X2 ||
                  MODE == SRC_STEM_X2, "pooling is fused into the producer");
    // precision "bf16x2" (SRC_DIRECT_X2 / SRC_STEM_X2): two-piece activations and weights, three virtual planes per real plane
    constexpr bool X2 = src_is_x2(MODE);
    constexpr bool STEM = src_is_stem(MODE);
    constexpr bool DIRECT = MODE == SRC_DIRECT || MODE == SRC_DIRECT_X2;
    static_assert(!X2 || std::is_same_v<T, __bf16>, "two-piece operands are bf16");
    static_assert(!STEM || (sizeof(T) == 2 && BN == 64), "fused stem: 2-byte output (bf16 / fp16), 64 couts");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const lds_in = smem;
    char* const lds_w = smem + Tile::IN_BYTES;           // slot 0; slot 1 at + W_STRIDE
    const unsigned lds_in_addr = lds_addr_of(lds_in);
    const unsigned lds_w_addr = lds_addr_of(lds_w);

    int lid = conv_block_remap();
    const int ksplit = epi_is_splitk(EPI) ? a.ksplit : 1;
    const int split = lid % ksplit;
    lid /= ksplit;
    const ConvTileId id = conv_tile_decode(a, lid);
    const int ct = id.ct, b = id.b;
    const int y0 = id.ty * TH, x0 = id.tx * TW;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lc = lane >> 4;
    const int wc = wave % WAVES_C, wp = wave / WAVES_C;

#ifdef FIUNET_STAMP
    // diagnostic build: per-wave s_memtime sums per phase.  Slots: [0] total [1] prologue (whole) [2] MFMA phases
    // [3] end-of-step wait + barrier [4] plane-boundary gather (rest) [5] epilogue [6] upsample staging DMA + wait
    // [7] upsample interpolation [8] record count; the prologue again, split (round 6): [9] kernel entry -> accumulators
    // initialised (argument + BatchNorm-shift loads) [10] W(0) issue + LDS read offsets [11] gather walk (per-tile
    // offsets / masks, padding zeroed; CONCAT_UP: the lerp tables) [12] fused stem: weights + patch staging + barrier
    // [13] first in-tile: DMA issue (fused stem: the stem's evaluation) [14] wait for W(0) + the in-tile (vmcnt(0))
    // [15] the barrier that publishes them.  PSTAMP pins the code of a sub-phase in place (sched_barrier), so the
    // prologue of this build is not scheduled as the shipped one is: [1] / [0] of a build WITHOUT the split is the
    // share to quote, the split says where inside it the time sits.
    unsigned long long st_sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_prev = st_t0;
#ifdef FIUNET_STAMP_PROLOG
    unsigned long long st_pprev = st_t0;
#define PSTAMP(slot) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                          st_sum[slot] += t_ - st_pprev; st_pprev = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PSTAMP(slot) do {} while (0)
#endif
#define STAMP(slot) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
                         st_sum[slot] += t_ - st_prev; st_prev = t_; } while (0)
#define STAMP_UP(slot) STAMP(slot)
#else
#define STAMP(slot) do {} while (0)
#define STAMP_UP(slot) do {} while (0)
#define PSTAMP(slot) do {} while (0)
#endif
    f32x4 acc[4][NF];
    conv_acc_init<T, BN, TH, TW, EPI>(a, acc, ct, wc, lc);  // BatchNorm shift (scale is in the weights)
#ifdef FIUNET_STAMP_PROLOG
    asm volatile("" :: "v"(acc[3][NF - 1][3]), "v"(acc[0][0][0]));  // the shift loads have landed
#endif
    PSTAMP(9);

    // per-lane LDS read offsets (everything else is an immediate)
    const int a_off = (wc * 64 + l15) * 64 + ((lc ^ swz(l15)) << 4);  // within a weight ring slot
    int b_off[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
        b_off[kx] = (wp * ROWS_W * TWP + kx + l15) * 64 + ((lc ^ swz(kx + l15)) << 4);

    const int nplanes_real = (a.C0 + a.C1) / PL;
    // X2: virtual plane v = 3 * real plane + j, j = 0: (xh, wh), 1: (xh, wl) on the SAME in-tile, 2: (xl, wh)
    const int nplanes_all = X2 ? 3 * nplanes_real : nplanes_real;
    const int p0 = a.C0 / PL;
    // this workgroup's K slice: (virtual) planes [pbeg, pend)
    const int pbeg = split * nplanes_all / ksplit, pend = (split + 1) * nplanes_all / ksplit;
    const int nsteps = (pend - pbeg) * 3;
    const char* wbase = (const char*)a.wgt + (size_t)ct * BN * 64;

    // ---- weight stream: each wave moves NW 1-KiB pieces (16 LDS rows) per step by LDS-DMA.  The
    //      LDS image is lane-linear, so the XOR swizzle goes on the per-lane SOURCE chunk. --------
    constexpr int NW = Tile::W_BYTES / 1024 / 4;
    // Piece j of this wave = packed rows r0 .. r0+15 with r0 = (wave * NW + j) * 16; 16 divides BN, so a
    // piece lies inside one tap: its source offset is a wave-uniform part (added to the SGPR base) plus
    // ONE per-lane register shared by all pieces (row within the piece, swizzled 16-B chunk).
    static_assert(BN % 16 == 0, "a weight piece must not straddle two taps");
    const unsigned w_lane_off = (unsigned)((lane >> 2) * 64 + (((lane & 3) ^ swz(lane >> 2)) << 4));
    auto issue_w = [&](int step) __attribute__((always_inline)) {  // step counts from this slice's start
        const int lp = step / 3, kx = step - lp * 3;
        int pl = pbeg + lp;
        if constexpr (X2) {  // weight planes: [wh of every real plane | wl of every real plane]
            const int real = pl / 3;
            pl = pl - real * 3 == 1 ? nplanes_real + real : real;
        }
        const char* wsrc = wbase + ((size_t)(pl * 9 + kx * 3) * a.Cout) * 64;  // packed [plane][kx][ky][cout]
        const unsigned dst = __builtin_amdgcn_readfirstlane(
            lds_w_addr + (unsigned)((step & 1) * Tile::W_STRIDE + wave * NW * 1024));
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int r0 = (wave * NW + j) * 16, tap = r0 / BN;  // tap = ky within the step
            glds16s(wsrc + (size_t)(tap * (a.Cout - BN) + r0) * 64, w_lane_off, dst + j * 1024);
        }
    };
    // W(0) goes out first (slot 0; slot 1 + spare is the idle staging area for plane 0), ahead of the
    // in-tile address math below, so its round trip runs under those ~200 instructions
#ifndef FIUNET_DIAG_FREE_PROLOGUE
    issue_w(0);
#endif
#ifdef FIUNET_DIAG_NO_WSTREAM
    if (nsteps > 1) issue_w(1);   // both ring slots hold real weights (realistic operand data, hence realistic power); nothing streams afterwards
#endif
    PSTAMP(10);

    // ---- in-tile gather (a): planes stored as-is in an NHWC tensor go by LDS-DMA: piece j = 16
    //      consecutive LDS rows (pixels) x 64 B, address = plane base in SGPRs + a 32-bit per-lane
    //      offset; lanes on pixels outside the image / on the row-pitch padding are switched off
    //      (their slots were zeroed once).  No data VGPRs, one memory round trip per plane. ---------
    constexpr int NPIECE = THP * TWP / 16;
    static_assert(THP * TWP % 16 == 0, "in-tile must be a whole number of 1-KiB pieces");
    const int aH = a.H, aW = a.W;
    const char* const dma_src = (const char*)a.src0 + (size_t)b * a.H * a.W * a.C0 * sizeof(T) * (X2 ? 2 : 1);
    // SRC_DIRECT with C1 > 0: planes >= p0 come from a second full-resolution tensor (the upsampled
    // half of a concat input, materialised by upsample_kernel when several cout tiles share it)
    const char* const dma_src1 = DIRECT && a.C1 > 0
                                     ? (const char*)a.src1 + (size_t)b * a.H * a.W * a.C1 * sizeof(T) * (X2 ? 2 : 1) : nullptr;
    // The per-lane source offset of every piece is plane-invariant in the blocked layout.  Where
    // registers allow (the plain 128-cout direct kernels) it is computed once (NPW registers, 32-bit)
    // and a plane's gather costs ~8 instructions per piece; the pooled / concat / head / split-K
    // variants and the 64-cout tiles (12-14 pieces per wave), which are at the 256-VGPR limit,
    // rebuild it per plane from three registers (see pm_* below; hoisting there spills).
    // (64 x 64 wave tiles - the small-problem configuration - have 64 accumulator registers less: every direct variant hoists)
    constexpr bool HOIST = (MODE == SRC_DIRECT && BN == 128 && EPI == EPI_PLAIN) ||   // (the two-piece epilogue with it: 3 spilled registers)
                           (NF == 4 && DIRECT);
    // Rolling window of in-tile rows across the three ky taps of a step (24 instead of 36 fragment
    // reads per step): bf16 32-wide tiles.  The fp32 instantiations (4 MFMAs per fragment pair keep
    // more operands in flight) and the 16-wide tiles have no registers to spare for the extra row
    // and re-read every row for every tap instead; same tap order, same sums.
    constexpr bool ROLL = sizeof(T) == 2 && FR == 2 && (!epi_is_splitk(EPI) || NF == 4);
    constexpr int NPW = (NPIECE + 3) / 4;
    unsigned in_off[HOIST ? NPW : 1];
    const unsigned plane_bytes = (unsigned)(aH * aW) * 64u;
    // Walk over this wave's pieces: f(j, ok, off) with off = byte offset of the lane's 16 B inside a
    // plane of the source image (valid when ok).  Hoisted kernels read the stored offsets.  The others
    // keep THREE registers instead of one per piece: a wave's pieces are 64 in-tile pixels apart, so
    // (py, px) and the linear pixel index advance by constants with one conditional row wrap (64 rows
    // keep the swizzle phase; NPIECE * 16 == THP * TWP exactly, so py stays inside) - the walk is done
    // once per tile and leaves the first piece's offset plus two bit masks (piece jj valid / row wrap
    // after piece jj); a plane's gather then needs no coordinate arithmetic at all.
    unsigned pm_lin0 = 0, pm_valid = 0, pm_wrap = 0;
    static_assert(NPW <= 32, "one mask bit per piece of a wave");
    constexpr int PM_DY = 64 / TWP, PM_DX = 64 % TWP;
    const unsigned pm_dlin = (unsigned)(PM_DY * aW + PM_DX) * 64u, pm_dwrap = (unsigned)(aW - TWP) * 64u;
    if constexpr (!STEM) {
        // one division per tile; every further piece is the previous one + 64 in-tile pixels (the hoisted
        // kernels keep the resulting offsets, the others the first offset and two bit masks)
        const int row0 = wave * 16 + (lane >> 2);
        int py = row0 / TWP, px = row0 - py * TWP;
        int y = y0 - 1 + py, x = x0 - 1 + px;
        pm_lin0 = (unsigned)(y * aW + x) * 64u + (((lane & 3) ^ swz(row0)) << 4);
        unsigned lin = pm_lin0;
#pragma unroll
        for (int jj = 0; jj < NPW; ++jj) {
            const bool ok = (px < TW + 2) & ((unsigned)y < (unsigned)aH) & ((unsigned)x < (unsigned)aW);
            if constexpr (HOIST) in_off[jj] = ok ? lin : ~0u;
            pm_valid |= (ok ? 1u : 0u) << jj;
            px += PM_DX; x += PM_DX; y += PM_DY;
            lin += pm_dlin;
            if (px >= TWP) { px -= TWP; x -= TWP; y += 1; pm_wrap |= 1u << jj; lin += pm_dwrap; }
        }
    }
    auto for_pieces = [&](auto&& f) __attribute__((always_inline)) {
        if constexpr (HOIST) {
#pragma unroll
            for (int jj = 0; jj < NPW; ++jj) {
                const int j = wave + 4 * jj;
                if (j < NPIECE) f(j, in_off[jj] != ~0u, in_off[jj]);
            }
        } else {
            // opaque copies: without them hipcc hoists every piece's offset and mask out of the K loop
            // (they are plane-invariant), i.e. rebuilds the hoisted form and spills
            unsigned lin = pm_lin0, valid = pm_valid, wrap = pm_wrap;
            asm volatile("" : "+v"(lin), "+v"(valid), "+v"(wrap));
#pragma unroll
            for (int jj = 0; jj < NPW; ++jj) {
                const int j = wave + 4 * jj;
                if (j < NPIECE) f(j, ((valid >> jj) & 1u) != 0u, lin);
                // (pm_dwrap is negative mod 2^32 when the level is narrower than the in-tile pitch)
                lin += pm_dlin + (((wrap >> jj) & 1u) ? pm_dwrap : 0u);
            }
        }
    };
    // Padding slots of the in-tile (pixels outside the image, row-pitch filler) are the same for every
    // plane of the tile: they are zeroed ONCE here, and the per-plane DMAs simply leave those lanes
    // switched off (the interpolated planes of a concat conv write zeros there themselves).
    if constexpr (!STEM) {
        for_pieces([&](int j, bool ok, unsigned) __attribute__((always_inline)) {
            if (!ok) *reinterpret_cast<uint4*>(lds_in + j * 1024 + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
        });
    }
    auto gather_plane_dma = [&](int plane) __attribute__((always_inline)) {
        // wave-uniform plane base in SGPRs + the lane's 32-bit offset
        const char* base;
        if constexpr (X2) {  // virtual plane -> (real plane, piece): the lo planes follow the hi planes of their tensor
            const int real = plane / 3, lo = plane - real * 3 == 2;
            base = real >= p0 ? dma_src1 + (size_t)(real - p0 + (lo ? nplanes_real - p0 : 0)) * plane_bytes
                              : dma_src + (size_t)(real + (lo ? p0 : 0)) * plane_bytes;
        } else {
            base = (MODE == SRC_DIRECT && plane >= p0) ? dma_src1 + (size_t)(plane - p0) * plane_bytes
                                                       : dma_src + (size_t)plane * plane_bytes;
        }
        for_pieces([&](int j, bool ok, unsigned off) __attribute__((always_inline)) {
            if (ok) glds16s(base, off, __builtin_amdgcn_readfirstlane(lds_in_addr + (unsigned)j * 1024u));
        });
    };

    // ---- in-tile gather (b): bilinearly upsampled planes.  The low-res source tile (<= LRH x LRW
    //      pixels of this plane) is DMA-ed into the idle weight slot + spare region, then every
    //      thread interpolates its chunks LDS -> LDS: one memory round trip per plane instead of
    //      one per batch of register loads, and no VGPRs held across it. ---------------------------
    // Work split of the interpolation.  A column = (in-tile pixel column, 16-B chunk); a wave walks
    // DOWN 64 columns at once, all lanes on the same row, so the row mapping is wave-uniform (scalar
    // branches) and the horizontally interpolated low-res rows are reused from one output row to the
    // next.  The (TW+2)*4 columns are cut into groups of 64 ("main" groups, NMAIN of them) whose rows
    // are shared out over 4/NMAIN waves each, plus a tail of NTC < 64 columns whose NTC*THP elements
    // are interpolated independently, a quarter per wave: all four waves get the same amount of work
    // (the round-1 split left waves 2-3 idle and gave waves 0-1 every row).
    constexpr int UP_NCOL = (TW + 2) * 4;
    constexpr int UP_NMAIN = UP_NCOL / 64;            // 2 (TW = 32) or 1 (TW = 16)
    constexpr int UP_NTC = UP_NCOL - UP_NMAIN * 64;   // 8 tail columns
    constexpr int UP_WPG = 4 / UP_NMAIN;              // waves per main group
    constexpr int UP_SEGR = (THP + UP_WPG - 1) / UP_WPG;
    constexpr int UP_NTAIL = UP_NTC * THP;            // tail elements
    constexpr int UP_TAILW = (UP_NTAIL + 3) / 4;      // ... per wave
    static_assert(MODE != SRC_CONCAT_UP || (UP_NMAIN >= 1 && UP_NMAIN <= 2), "interpolation work split");
    int lr_y = 0, lr_x = 0;  // low-res origin of this tile's staging window
    char* const ytab = smem + Tile::TAB_OFF;          // [THP]   {off0, off1 (bytes into staging; < 0: zero row), hy, ly}
    char* const xtab = ytab + THP * 16;               // [TW+2]  {s0, s1 (bytes; < 0: zero column), hx, lx}
    uint4 yrow = make_uint4(0u, 0u, 0u, 0u);         // lane l < THP: ytab[l] (CONCAT_UP)
    if constexpr (MODE == SRC_CONCAT_UP) {
        const UpCoord u = up_coord(a, y0 - 1, x0 - 1);
        lr_y = u.y0; lr_x = u.x0;
        // the mapping of in-tile row py / column px, evaluated ONCE per tile (it is the same for
        // every plane); published by the barrier that ends the prologue
        {   // every wave keeps the row table in its own lanes 0 .. THP-1 as well: the column walk fetches
            // row py's entry with v_readlane (no LDS round trip per row; the walk is latency-bound)
            const int y = y0 - 1 + min(lane, THP - 1);
            const UpAxis uy = up_axis_y(a, min(max(y, 0), a.H - 1));
            const bool ok = uy.ok & (y >= 0) & (y < a.H);
            yrow = make_uint4(ok ? (unsigned)((uy.i0 - lr_y) * (Tile::LRP * 64)) : 0x80000000u,
                              (unsigned)((uy.i1 - lr_y) * (Tile::LRP * 64)), __float_as_uint(uy.h),
                              __float_as_uint(uy.l));
            if (tid < THP) *reinterpret_cast<uint4*>(ytab + tid * 16) = yrow;
        }
        if (tid >= 64 && tid < 64 + TW + 2) {
            const int px = tid - 64, x = x0 - 1 + px;
            const UpAxis ux = up_axis_x(a, min(max(x, 0), a.W - 1));
            const bool ok = ux.ok & (x >= 0) & (x < a.W);
            *reinterpret_cast<uint4*>(xtab + px * 16) =
                make_uint4(ok ? (unsigned)((ux.i0 - lr_x) * 64) : 0x80000000u, (unsigned)((ux.i1 - lr_x) * 64),
                           __float_as_uint(ux.h), __float_as_uint(ux.l));
        }
    }
    auto gather_plane_up = [&](int plane, int idle_slot) __attribute__((always_inline)) {
        constexpr int LRP = Tile::LRP, LRH = Tile::LRH;
        // idle slot 0: [slot0 | spare]; idle slot 1: [spare | slot1]
        const int stg_off = idle_slot == 0 ? 0 : Tile::W_BYTES;
        const char* const lsrc = (const char*)a.src1 + (size_t)b * a.lowH * a.lowW * a.C1 * sizeof(T) +
                                 (size_t)(plane - p0) * a.lowH * a.lowW * 64;
        int opq = 0;
        asm volatile("" : "+s"(opq));
        int l4 = (lane & 3) << 4;          // opaque: hipcc would otherwise form lsrc + l4 as a 64-bit
        asm volatile("" : "+v"(l4));       // per-lane pointer ahead of the K loop (and spill it)
#pragma unroll 1
        for (int j = wave; j < Tile::LR_PIECES; j += 4) {
            const int row = j * 16 + (lane >> 2) + opq;
            const int r = row / LRP, c = row - r * LRP;
            const int gy = min(lr_y + min(r, LRH - 1), a.lowH - 1), gx = min(lr_x + c, a.lowW - 1);
            const char* src = lsrc + ((unsigned)(gy * a.lowW + gx) * 64u + (unsigned)l4);
            glds16(src, __builtin_amdgcn_readfirstlane(lds_w_addr + (unsigned)(stg_off + j * 1024)));
        }
        lds_dma_wait_all();
        __syncthreads();
        STAMP_UP(6);
        const char* const stg = lds_w + stg_off;
        constexpr int NE = Elem<T>::NE;
        // ---- main groups: column walk over this wave's row segment ------------------------------
        {
            const int grp = UP_NMAIN == 1 ? 0 : (wave & 1), seg = UP_NMAIN == 1 ? wave : (wave >> 1);
            const int col = grp * 64 + lane, px = col >> 2, ch = col & 3;
            const uint4 xt = *reinterpret_cast<const uint4*>(xtab + px * 16);
            const bool okx = (int)xt.x >= 0;
            const char* const s0 = stg + (okx ? (int)xt.x : 0) + ch * 16;
            const char* const s1 = stg + (okx ? (int)xt.y : 0) + ch * 16;
            // columns outside the upsampled extent (F.pad / conv padding) get zero weights instead of a
            // per-row select: every source value is a ReLU output (>= +0), so 0 * a + 0 * b = +0 exactly
            const float hx = okx ? __uint_as_float(xt.z) : 0.f, lx = okx ? __uint_as_float(xt.w) : 0.f;
            float h0[NE], h1[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) h0[i] = h1[i] = 0.f;
            int c0 = -1, c1 = -1;  // staging row offsets currently held in h0 / h1 (wave-uniform)
            const int rbeg = seg * UP_SEGR, rend = min(THP, rbeg + UP_SEGR);
            // Row py's table entry comes from the wave's own lane py (v_readlane: no LDS round trip per row;
            // up3.0 -1.5 %, up4.0 -2.3 % against the LDS read, profiles/r03_ab_lerp_variants.txt).  Tried on
            // top of it and dropped, same file: the one new low-res row of the NEXT output row requested an
            // iteration early (1-1.5 % slower: the walk is not bound by LDS latency), the arithmetic on
            // float pairs (v_pk_fma_f32: null), s_setprio 3 for the walk (null).
#pragma unroll 1
            for (int py = rbeg; py < rend; ++py) {
                const uint4 yt = make_uint4((unsigned)__builtin_amdgcn_readlane((int)yrow.x, py),
                                            (unsigned)__builtin_amdgcn_readlane((int)yrow.y, py),
                                            (unsigned)__builtin_amdgcn_readlane((int)yrow.z, py),
                                            (unsigned)__builtin_amdgcn_readlane((int)yrow.w, py));
                const int o0 = (int)yt.x, o1 = (int)yt.y;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (o0 >= 0) {  // rows outside the image / the upsampled extent stay zero (conv pad, F.pad)
                    if (o0 != c0) {
                        if (o0 == c1) {
                            // (swapping the roles of h0 / h1 instead of copying - two instantiations of the
                            // row step chosen by a wave-uniform flag - measured 4-9 % SLOWER on up3.0 / up4.0)
#pragma unroll
                            for (int i = 0; i < NE; ++i) h0[i] = h1[i];
                        } else {
                            chunk_hlerp<T>(*reinterpret_cast<const uint4*>(s0 + o0),
                                           *reinterpret_cast<const uint4*>(s1 + o0), hx, lx, h0);
                        }
                        c0 = o0;
                    }
                    if (o1 != c1) {
                        if (o1 == c0) {
#pragma unroll
                            for (int i = 0; i < NE; ++i) h1[i] = h0[i];
                        } else {
                            chunk_hlerp<T>(*reinterpret_cast<const uint4*>(s0 + o1),
                                           *reinterpret_cast<const uint4*>(s1 + o1), hx, lx, h1);
                        }
                        c1 = o1;
                    }
                    v = chunk_vlerp<T>(h0, h1, __uint_as_float(yt.z), __uint_as_float(yt.w));
                }
                const int row = py * TWP + px;
                *reinterpret_cast<uint4*>(lds_in + row * 64 + ((ch ^ swz(row)) << 4)) = v;
            }
        }
        // ---- tail columns: UP_NTC x THP elements, a quarter per wave, each interpolated on its own
        //      (chunk_bilerp = chunk_hlerp + chunk_vlerp operation for operation: the same bits)
        for (int k = lane; k < UP_TAILW; k += 64) {
            const int e = wave * UP_TAILW + k;
            if (e < UP_NTAIL) {
                const int py = e / UP_NTC, col = UP_NMAIN * 64 + (e - py * UP_NTC), px = col >> 2, ch = col & 3;
                const uint4 xt = *reinterpret_cast<const uint4*>(xtab + px * 16);
                const uint4 yt = *reinterpret_cast<const uint4*>(ytab + py * 16);
                const bool ok = ((int)xt.x >= 0) & ((int)yt.x >= 0);
                const char* const q0 = stg + (ok ? (int)xt.x : 0) + ch * 16;
                const char* const q1 = stg + (ok ? (int)xt.y : 0) + ch * 16;
                const int o0 = ok ? (int)yt.x : 0, o1 = ok ? (int)yt.y : 0;
                uint4 v = chunk_bilerp<T>(*reinterpret_cast<const uint4*>(q0 + o0), *reinterpret_cast<const uint4*>(q1 + o0),
                                          *reinterpret_cast<const uint4*>(q0 + o1), *reinterpret_cast<const uint4*>(q1 + o1),
                                          __uint_as_float(xt.z), __uint_as_float(xt.w), __uint_as_float(yt.z),
                                          __uint_as_float(yt.w));
                if (!ok) v = make_uint4(0u, 0u, 0u, 0u);
                const int row = py * TWP + px;
                *reinterpret_cast<uint4*>(lds_in + row * 64 + ((ch ^ swz(row)) << 4)) = v;
            }
        }
        STAMP_UP(7);
    };

    // ---- in-tile gather (c): SRC_STEM.  The plane's 32 channels of relu(bn(conv3x3(frames))) are
    //      computed right here for the (TH+2)x(TW+2) window, from a raw fp32 patch of the two frames
    //      staged once per tile.  bf16 MFMA with the operands split hi+lo (x = xh + xl, w = wh + wl;
    //      xh*wh + xl*wh + xh*wl, fp32 accumulate) keeps ~2^-16 relative accuracy, far below the
    //      bf16 rounding of the result.  k = tap*2 + frame (18 of 32 slots used).
    constexpr int NIN = THP * (TW + 2);  // in-tile pixels
    // patch image: bf16, [row][hi | lo][col][frame]; the 8 k-slots of a lane group are the 16 contiguous
    // bytes (4 columns x 2 frames) at (row + dy, col): k = lane group*8 + dx*2 + frame, zero weights for dx = 3.
    char* const patch = smem + Tile::PATCH_OFF;
    constexpr int PW = Tile::PATCH_W, PH = Tile::PATCH_H, PP = Tile::PATCH_PITCH;
    auto stage_patch = [&]() __attribute__((always_inline)) {
        if constexpr (STEM) {
            // one thread = one patch pixel (both frames): one address, one dither value, one dword store
            // for the hi pair and one for the lo pair (the prologue is VALU-bound: SQ_INSTS_VALU per wave
            // tracks its time, profiles/r03_pmc_ab_stem.txt)
            unsigned* const pd = reinterpret_cast<unsigned*>(patch);  // dwords {frame1, frame2}; lo part: + PW
            constexpr int NP = PH * PW;               // patch pixels
            constexpr int NB = (NP + 255) / 256;      // all loads are issued before the first use
            float v0[NB], v1[NB];
            unsigned okm = 0;
            // unconditional loads from clamped coordinates (all issued back to back, one wait), the
            // out-of-image pixels are zeroed afterwards
            size_t at[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int r = tid + k * 256;
                const int py = r / PW, px = r - py * PW;
                const int y = y0 - 2 + py, x = x0 - 2 + px;
                const bool ok = (r < NP) & (y >= 0) & (y < aH) & (x >= 0) & (x < aW);
                okm |= (ok ? 1u : 0u) << k;
                at[k] = ((size_t)b * aH + min(max(y, 0), aH - 1)) * aW + min(max(x, 0), aW - 1);
            }
            if (a.u1) {  // wave-uniform: fiunet_forward_u8 reads the uint8 frames right here
                unsigned char q0[NB], q1[NB];
#pragma unroll
                for (int k = 0; k < NB; ++k) { q0[k] = a.u1[at[k]]; q1[k] = a.u2[at[k]]; }
#pragma unroll
                for (int k = 0; k < NB; ++k) { v0[k] = preprocess_u8_value(q0[k]); v1[k] = preprocess_u8_value(q1[k]); }
            } else {
#pragma unroll
                for (int k = 0; k < NB; ++k) { v0[k] = a.f1[at[k]]; v1[k] = a.f2[at[k]]; }
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int r = tid + k * 256;
                const int py = r / PW, px = r - py * PW;
                // ordered input dither, +d on frame 1 and -d on frame 2 (stem_dither); the conv's zero
                // padding stays exactly zero
                const float d = a.dither * stem_dither(y0 - 2 + py, x0 - 2 + px);
                const bool ok = (okm >> k) & 1u;
                v0[k] = ok ? v0[k] + d : 0.f;
                v1[k] = ok ? v1[k] - d : 0.f;
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int r = tid + k * 256;
                const int py = r / PW, px = r - py * PW;
                const unsigned hi = pack_bf16x2_pk(v0[k], v1[k]);
                const unsigned lo = pack_bf16x2_pk(v0[k] - __uint_as_float(hi << 16), v1[k] - __uint_as_float(hi & 0xffff0000u));
                if (r < NP) {
                    pd[py * PP + px] = hi;
                    pd[py * PP + px + PW] = lo;
                }
            }
            // bias operand (in the in-tile's row-pitch filler): PW dwords {1.0, 0}, then PW zero dwords (lo part)
            if (tid < 2 * PW) reinterpret_cast<unsigned*>(smem + Tile::PATCH_TAIL_OFF)[tid] = tid < PW ? 0x00003f80u : 0u;
        }
    };
    // The plane's A operands: two 16-cout tiles, hi and lo parts, BatchNorm scale folded in on the
    // host and the BatchNorm shift riding in k-slot 24 (lane group 3, whose data operand is 1.0).
    // Plane 0's come straight from global memory, requested before the patch is staged; plane 1's
    // are parked in LDS by DMA at kernel start and picked up at the plane boundary.
    struct StemW { uint4 wh[2], wl[2]; };
    StemW stem_w0;
    auto stem_park = [&](int plane) __attribute__((always_inline)) {   // LDS-DMA of one plane's stem weights into STEMW
        if constexpr (STEM && X2)   // issued again inside the K loop: scalar base + 32-bit lane offset, so that no 64-bit
            glds16s((const char*)a.stem_w + (wave >> 1) * 4096 + (2 * plane + (wave & 1)) * 1024, (unsigned)lane * 16u,   // per-lane pointer lives across it
                    __builtin_amdgcn_readfirstlane(lds_in_addr + (unsigned)(Tile::STEMW_OFF + wave * 1024)));
        else if constexpr (STEM)
            glds16((const char*)a.stem_w + (wave >> 1) * 4096 + (2 * plane + (wave & 1)) * 1024 + lane * 16,
                   __builtin_amdgcn_readfirstlane(lds_in_addr + (unsigned)(Tile::STEMW_OFF + wave * 1024)));
    };
    auto stem_load = [&](StemW& w) __attribute__((always_inline)) {
        if constexpr (STEM) {
            int lane_ofs = l15 * 64 + lc * 16;     // opaque: keeps hipcc from forming the 64-bit
            asm volatile("" : "+v"(lane_ofs));     // per-lane pointer before the K loop and spilling it
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                w.wh[h] = ldg16((const char*)a.stem_w + h * 1024 + lane_ofs);
                w.wl[h] = ldg16((const char*)a.stem_w + 4096 + h * 1024 + lane_ofs);
            }
            // plane 1 (X2: plane 0 again - its lo piece is evaluated from the same weights; plane 1's follow by
            // stem_park(1) once every wave has picked these up): wave w moves [hi h0 | hi h1 | lo h0 | lo h1][w], lane-linear
            stem_park(X2 ? 0 : 1);
        }
    };
    auto stem_parked = [&](StemW& w) __attribute__((always_inline)) {
        if constexpr (STEM) {
            const char* const base = smem + Tile::STEMW_OFF + l15 * 64 + lc * 16;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                w.wh[h] = *reinterpret_cast<const uint4*>(base + h * 1024);
                w.wl[h] = *reinterpret_cast<const uint4*>(base + 2048 + h * 1024);
            }
        }
    };
    auto gather_plane_stem = [&](const StemW& w, bool lo_piece = false) __attribute__((always_inline)) {
        if constexpr (STEM) {
            // lane groups 0, 1, 2 read patch rows py, py+2, py+1 (so that the two groups served together
            // by a ds_read2_b32, lanes 0-31, sit 2 * pitch = 16 banks apart); lane group 3 (k = 24..31, only
            // k = 24 has a weight: the BatchNorm shift) reads the {1.0, 0} dwords / their zero lo part at one
            // fixed address (a broadcast: at most one bank shared with lane group 2)
            constexpr int TAIL_IDX = (Tile::PATCH_TAIL_OFF - Tile::PATCH_OFF) / 4;  // dword index relative to the patch
            const unsigned* const ph32 = reinterpret_cast<const unsigned*>(patch);
            const unsigned* const pl32 = ph32 + PW;  // the lo part of a patch row follows its hi part
            struct Frag { uint4 bh, bl; int dst; };  // dst = in-tile row of the lane's pixel, >= THP*TWP: lane beyond the in-tile
            // A wave's fragments are 64 in-tile pixels apart: the lane's patch index `e` and in-tile row `dst`
            // advance by constants, plus a constant more when the pixel column wraps into the next row.
            // Every VALU instruction here is paid at the partner wave's MFMA cadence (~16 cycles while the
            // co-resident workgroup streams MFMAs on this SIMD), so the loop carries nothing it can do
            // without: no multiplies, no coordinates besides the column, and in-tile pixels outside the
            // image are NOT tested here - the few tiles on the image border re-zero them in a separate pass.
            constexpr int DY = 64 / (TW + 2), DX = 64 % (TW + 2);
            const int py0 = (wave * 16 + l15) / (TW + 2);
            int px = wave * 16 + l15 - py0 * (TW + 2);
            // lane group 3's address does not move (all its increments are zero)
            int e = lc < 3 ? py0 * PP + px + (lc == 0 ? 0 : (lc == 1 ? 2 * PP : PP)) : TAIL_IDX;
            const int e_step = lc < 3 ? DY * PP + DX : 0, e_wrap = lc < 3 ? PP - (TW + 2) : 0;
            int dst = py0 * TWP + px;
            auto fetch = [&](Frag& f) __attribute__((always_inline)) {
                // lanes past the last in-tile pixel (last fragment only) read one row beyond the patch - the
                // parked stem weights, finite values - and store nothing
                f.bh = make_uint4(ph32[e], ph32[e + 1], ph32[e + 2], ph32[e + 3]);
                f.bl = make_uint4(pl32[e], pl32[e + 1], pl32[e + 2], pl32[e + 3]);
                f.dst = dst;
                px += DX;
                const bool wrap = px >= TW + 2;
                px -= wrap ? TW + 2 : 0;
                e += e_step + (wrap ? e_wrap : 0);
                dst += DY * TWP + DX + (wrap ? TWP - (TW + 2) : 0);
            };
            auto compute = [&](const Frag& f) __attribute__((always_inline)) {
                f32x4 s4[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) s4[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int h = 0; h < 2; ++h) mma_chunk<__bf16>(s4[h], w.wl[h], f.bh);
#pragma unroll
                for (int h = 0; h < 2; ++h) mma_chunk<__bf16>(s4[h], w.wh[h], f.bl);
#pragma unroll
                for (int h = 0; h < 2; ++h) mma_chunk<__bf16>(s4[h], w.wh[h], f.bh);
                // packed row lc*4 + j of tile h is channel lc*8 + h*4 + j of the plane (host:
                // bf16_row_to_cout): the lane's 8 values are ONE 16-B chunk of the pixel's record - one
                // ds_write_b128 (2-way bank conflicts) instead of two ds_write_b64 (4-way)
                const int row = f.dst;
                // (the split MFMAs are bf16 whatever the output type; precision "fp16" rounds the result to fp16 here)
                uint4 pk = make_uint4(relu_pk_bf16(pack2_pk<T>(s4[0][0], s4[0][1])),
                                      relu_pk_bf16(pack2_pk<T>(s4[0][2], s4[0][3])),
                                      relu_pk_bf16(pack2_pk<T>(s4[1][0], s4[1][1])),
                                      relu_pk_bf16(pack2_pk<T>(s4[1][2], s4[1][3])));
                if constexpr (X2) {
                    if (lo_piece) {   // (wave-uniform) lo = RNE bf16 of relu(v) - hi; a negative v has hi = lo = +0
                        auto lo2 = [](float v0, float v1, unsigned hi) __attribute__((always_inline)) {
                            return pack_bf16x2_pk(fmaxf(v0, 0.f) - __uint_as_float(hi << 16),
                                                  fmaxf(v1, 0.f) - __uint_as_float(hi & 0xffff0000u));
                        };
                        pk = make_uint4(lo2(s4[0][0], s4[0][1], pk.x), lo2(s4[0][2], s4[0][3], pk.y),
                                        lo2(s4[1][0], s4[1][1], pk.z), lo2(s4[1][2], s4[1][3], pk.w));
                    }
                }
                // address = row * 64 + ((lc ^ swz(row)) << 4), with the swizzle as one xor of bit 5
                if (row < THP * TWP) *reinterpret_cast<uint4*>(lds_in + ((row * 64 + lc * 16) ^ ((row & 4) << 3))) = pk;
            };
            // two fragments per trip, operands of the next one in flight during the MFMAs of this one
            constexpr int NQ = (NIN + 15) / 16;
            Frag fa, fb;
            fetch(fa);
#pragma unroll 1
            for (int q = wave; q < NQ; q += 8) {
                fetch(fb);
                compute(fa);
                fetch(fa);
                if (q + 4 < NQ) compute(fb);
            }
            // Tiles on the image border (6 % of them at 1080p): the in-tile pixels outside the image are
            // the NEXT conv's zero padding, not stem outputs - overwrite them with zeros once every wave's
            // stores are done (workgroup-uniform branch; the caller's barrier publishes the result).
            if ((y0 == 0) | (x0 == 0) | (y0 + TH >= aH) | (x0 + TW >= aW)) {
                __syncthreads();
                for (int i = tid; i < THP * (TW + 2) * 4; i += 256) {
                    const int q = i >> 2, ch = i & 3;
                    const int qy = q / (TW + 2), qx = q - qy * (TW + 2);
                    const bool in = ((unsigned)(y0 - 1 + qy) < (unsigned)aH) & ((unsigned)(x0 - 1 + qx) < (unsigned)aW);
                    const int row = qy * TWP + qx;
                    if (!in) *reinterpret_cast<uint4*>(lds_in + row * 64 + ((ch ^ swz(row)) << 4)) = make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
    };
    auto gather_plane = [&](int plane, int idle_slot, bool first) __attribute__((always_inline)) {
        if constexpr (STEM && X2) {   // virtual planes 0 / 2 / 3 / 5 = (plane 0 hi, plane 0 lo, plane 1 hi, plane 1 lo)
            if (first) {
                gather_plane_stem(stem_w0, false);
            } else {
                StemW w;
                stem_parked(w);   // plane 0's weights at virtual plane 2, plane 1's at 3 and 5 (see the K loop)
                gather_plane_stem(w, plane == 2 || plane == 5);
            }
        } else if constexpr (STEM) {  // exactly two planes (64 stem channels)
            if (first) {
                gather_plane_stem(stem_w0);
            } else {
                StemW w1;
                stem_parked(w1);
                gather_plane_stem(w1);
            }
        }
        else if (DIRECT || plane < p0) gather_plane_dma(plane);
        else gather_plane_up(plane, idle_slot);
    };

    PSTAMP(11);
    if constexpr (STEM) {
        stem_load(stem_w0);
        stage_patch();
        __syncthreads();
        PSTAMP(12);
    }
    // timing diagnostics (results are garbage, only the clock matters; round 6, review item 1): -DFIUNET_DIAG_FREE_PROLOGUE drops W(0) and
    // the first in-tile gather of every kernel that fetches it by DMA - the kernel as it would run if a cross-tile prefetch
    // had delivered both for free (the upper bound of lever (a)); -DFIUNET_DIAG_NO_WSTREAM drops the whole weight stream - the
    // upper bound of weights held in LDS for the kernel's lifetime (lever (b))
    // (staging area of an upsampled first plane - a K slice may start in the upsampled half: slot 1, W(0) being in slot 0)
#ifdef FIUNET_DIAG_FREE_PROLOGUE
    if constexpr (STEM || MODE == SRC_CONCAT_UP) gather_plane(pbeg, 1, true);
#else
    gather_plane(pbeg, 1, true);
#endif
    PSTAMP(13);
    lds_dma_wait_all();
    PSTAMP(14);
    __syncthreads();
    PSTAMP(15);
    STAMP(1);
#ifdef FIUNET_CLOCK
    // diagnostic build (-DFIUNET_CLOCK, no other stamp executes): shader cycles (s_memtime) and constant 100 MHz ticks
    // (s_memrealtime) ONCE around the K loop -> the clock this wave ran at (MI355X_MICROARCH.md, DVFS give-back item 6)
    const unsigned long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    int step = 0;
    int vj = X2 ? pbeg % 3 : 0;   // X2: piece combination of the current virtual plane
    for (int plane = pbeg; plane < pend; ++plane) {
        // X2: the plane after an (xh, wh) plane multiplies the same in-tile by wl - no gather, no boundary
        const bool gather_next = plane + 1 < pend && !(X2 && vj == 0);
        if constexpr (X2) vj = vj == 2 ? 0 : vj + 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx, ++step) {
            // W(step) and the in-tile of `plane` are resident.  Stream W(step+1) into the other
            // ring slot (its last readers passed the barrier that ended step-1).
#ifndef FIUNET_DIAG_NO_WSTREAM
            if (step + 1 < nsteps) issue_w(step + 1);
#endif
            const char* wcur = lds_w + (step & 1) * Tile::W_STRIDE + a_off;
            // this wave's in-tile rows 0 .. ROWS_W+1 at column offset kx: row i serves tap ky for the
            // output row i - ky, so every fragment is read once and used by up to three taps
            // Last step of a plane whose successor arrives by plain LDS-DMA: after the load of the last
            // in-tile row (tap ky = 1) the rolling window holds everything the rest of the step needs,
            // so a barrier there declares the in-tile dead and the next plane's DMA is issued BEFORE
            // the remaining 64 MFMAs, which cover its round trip (no second in-tile buffer needed).
            constexpr bool EARLY_OK = ROLL && DIRECT;  // (the concat kernels would spill 6-8 registers)
            bool early = false;
            if constexpr (EARLY_OK)
                early = kx == 2 && gather_next && (DIRECT || plane + 1 < p0);
            if constexpr (ROLL) {
                uint4 xb[ROWS_W + 2][FR];
                auto load_row = [&](int i) __attribute__((always_inline)) {
#pragma unroll
                    for (int f = 0; f < FR; ++f)
                        xb[i][f] = *reinterpret_cast<const uint4*>(lds_in + b_off[kx] + (i * TWP + f * 16) * 64);
                };
#pragma unroll
                for (int i = 0; i < ROWS_W; ++i) load_row(i);   // rows of tap ky = 0
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    uint4 wa[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        wa[m] = *reinterpret_cast<const uint4*>(wcur + (ky * BN + m * 16) * 64);
                    if (ky < 2) load_row(ROWS_W + ky);  // the one new row of the next tap (row ky dies after this one)
                    if (ky == 1 && early) {
                        // that was this wave's last read of the plane's in-tile (rows 1 .. ROWS_W+1 are
                        // in registers): once every wave is here the in-tile is dead and the next
                        // plane's DMA goes out, 64 MFMAs ahead of the boundary
                        __syncthreads();
                        gather_plane(plane + 1, step & 1, false);
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < NF; ++n) mma_chunk<T>(acc[m][n], wa[m], xb[n / FR + ky][n % FR]);
                }
            } else {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    // compiler-only barrier: without it hipcc merges the fragment reads that
                    // consecutive taps share and keeps them in registers, i.e. builds the rolling
                    // window after all (and spills)
                    asm volatile("" ::: "memory");
                    uint4 wa[4], xb[NF];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        wa[m] = *reinterpret_cast<const uint4*>(wcur + (ky * BN + m * 16) * 64);
#pragma unroll
                    for (int n = 0; n < NF; ++n)
                        xb[n] = *reinterpret_cast<const uint4*>(
                            lds_in + b_off[kx] + (((n / FR) + ky) * TWP + (n % FR) * 16) * 64);
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int n = 0; n < NF; ++n) mma_chunk<T>(acc[m][n], wa[m], xb[n]);
                }
            }
#ifdef FIUNET_STAMP
            asm volatile("" :: "v"(acc[3][NF - 1][3]));  // keep the stamp behind the last MFMA
            __builtin_amdgcn_sched_barrier(0);
#endif
            STAMP(2);
            if (kx == 2 && gather_next && !early) {
                __syncthreads();  // every wave is done with this plane's in-tile and with W(step)
                gather_plane(plane + 1, step & 1, false);
                lds_dma_wait_all();
                __syncthreads();
                // fused x2 stem: every wave has read plane 0's parked weights for the last time (lo piece): plane 1's
                // take their place, landing under the next three steps (each step end waits for this wave's DMAs)
                if constexpr (STEM && X2) { if (plane + 1 == 2) stem_park(1); }
                STAMP(4);
            } else {
                lds_dma_wait_all();   // this wave's pieces of W(step+1) landed
                __syncthreads();      // ... and so have everyone else's
                STAMP(3);
            }
        }
    }

#ifdef FIUNET_CLOCK
    {
        asm volatile("" :: "v"(acc[3][NF - 1][3]));  // keep the stamp behind the last MFMA
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long ck_t1 = __builtin_amdgcn_s_memtime(), ck_r1 = __builtin_amdgcn_s_memrealtime();
        const unsigned st_idx = blockIdx.x * 4u + (unsigned)wave;
        if (a.stamp && lane == 0 && st_idx < a.stamp_cap) {  // one private 128-B record per wave, read by nothing else in the kernel
            unsigned long long* rec = a.stamp + (size_t)st_idx * 16;
            rec[0] = ck_t1 - ck_t0;
            rec[1] = ck_r1 - ck_r0;
            rec[8] = 1ull;
        }
    }
#endif
    conv_epilogue<T, BN, TH, TW, EPI, X2>(a, acc, b, y0, x0, ct, split, wc, wp, l15, lc);
#ifdef FIUNET_STAMP
    STAMP(5);
    st_sum[0] = st_prev - st_t0;
    const unsigned st_idx = blockIdx.x * 4u + (unsigned)wave;
    if (a.stamp && lane == 0 && st_idx < a.stamp_cap) {  // one private 128-B record per wave: no atomics, no contention
        unsigned long long* rec = a.stamp + (size_t)st_idx * 16;
#pragma unroll
        for (int k = 0; k < 16; ++k) rec[k] = k == 8 ? 1ull : st_sum[k];
    }
#endif
}

// Second pass of a K-split conv (small problems: fewer workgroups than the chip has CUs, e.g. the deep levels of the ONE
// 256x256 pair the reference runs, /root/reference/model/inference.py:29): one wave per (tile, cout tile, conv wave) adds the
// `ksplit` fp32 partial-sum slices in index order - deterministic, no atomics - on top of the BatchNorm shift, and then
// runs the conv kernel's OWN epilogue on the sums: ReLU, the blocked store, the fused MaxPool2d(2) copy (EPI_POOL) and the
// two-piece split of precision "bf16x2", all from one code path (rounds 1-5: a pixel-major slab, an element-wise
// finalize kernel and a separate max-pool launch).  The slab is read in the fragment order the conv wrote it in
// (conv_epilogue, EPI_SPLITK): 1 KiB contiguous per load instruction.
// Tried instead and NOT shipped (round 6): the reduction inside the conv kernel by the last workgroup of a tile to
// arrive (arrival counter, no waiting, one dispatch less per cut stage).  With agent-scope fences around the slab
// accesses (`buffer_wbl2` + `buffer_inv`: each workgroup writes back / drops its XCD's whole L2) it is correct - all
// GPU tests, 5 400 forwards bit-identical - and 1.2-1.6x SLOWER end to end (ONE 256x256 pair: bf16 0.295 -> 0.486 ms,
// fp32 0.913 -> 1.134); with write-through (sc0 sc1) stores instead of the release fence it is fast and WRONG (stale
// slices across XCDs: golden 135x240 fails).  The dispatch boundary is the cheapest coherence point this chip offers.
// One 64-thread workgroup per (tile, conv wave): the pass is bound by how many CUs pull slab bytes at once (a deep fp32
// level is 16 tiles x 16 slices x 64 KiB), not by arithmetic, and nothing in the epilogue crosses a wave.
template <typename T, int BN, int TH, int TW, int EPI, bool X2>
__global__ __launch_bounds__(64) void splitk_finalize_tile_kernel(const ConvArgs a)
{
    static_assert(EPI == EPI_PLAIN || EPI == EPI_POOL, "a fused head is never K-split");
    constexpr int WAVES_C = BN / 64;
    constexpr int NF = conv_wave_frags(BN, TH, TW);
    int t = blockIdx.x >> 2;                  // = the conv's logical tile index (its slab record)
    const int tile = t;
    const int ct = t % a.nct; t /= a.nct;
    const int tx = t % a.tilesX; t /= a.tilesX;
    const int ty = t % a.tilesY;
    const int b = t / a.tilesY;
    const int lane = threadIdx.x & 63, wave = blockIdx.x & 3;   // the conv wave whose fragments this workgroup reduces
    const int l15 = lane & 15, lc = lane >> 4;
    const int wc = wave % WAVES_C, wp = wave / WAVES_C;
    const int ntile = a.B * a.tilesY * a.tilesX * a.nct;
    f32x4 acc[4][NF];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float4* p = reinterpret_cast<const float4*>(a.kslab) + (((size_t)tile * 4 + wave) * (4 * NF)) * 64 + lane;
    const size_t slice = (size_t)ntile * 4 * (4 * NF) * 64;
    // slices in chunks: the CH x NF loads of a cout tile are independent and issued together (the pass is a chain of
    // memory round trips, not bandwidth: one slice per trip took ~0.5 us per slice), the additions stay in slice order
    const int ks = a.ksplit;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float4* pm = p + (size_t)m * NF * 64;
        constexpr int CH = NF == 8 ? 2 : 4;   // (128 accumulator registers leave room for two slices in flight, 64 for four)
        for (int s0 = 0; s0 < ks; s0 += CH, pm += CH * slice) {
            float4 q[CH][NF];
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (s0 + j < ks) {
#pragma unroll
                    for (int n = 0; n < NF; ++n) q[j][n] = pm[j * slice + n * 64];
                }
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (s0 + j < ks) {
#pragma unroll
                    for (int n = 0; n < NF; ++n) {
                        acc[m][n][0] += q[j][n].x; acc[m][n][1] += q[j][n].y; acc[m][n][2] += q[j][n].z; acc[m][n][3] += q[j][n].w;
                    }
                }
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {   // BatchNorm shift (the scale is folded into the weights)
        const float4 sh = *reinterpret_cast<const float4*>(a.shift + ct * BN + wc * 64 + conv_cout_ofs<T>(m, lc));
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            acc[m][n][0] += sh.x; acc[m][n][1] += sh.y; acc[m][n][2] += sh.z; acc[m][n][3] += sh.w;
        }
    }
    conv_epilogue<T, BN, TH, TW, EPI, X2>(a, acc, b, ty * TH, tx * TW, ct, 0, wc, wp, l15, lc);
}

}  // namespace fiunet
