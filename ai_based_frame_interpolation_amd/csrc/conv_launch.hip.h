// conv_launch.hip.h -- the host side of one conv launch: tile shape, K cut and kernel of a (gather mode, epilogue,
// configuration), down to hipLaunchKernelGGL.  Included by the conv units alone (conv_f32.hip, conv_f16.hip,
// conv_bf16.hip, conv_bf16x2.hip), each of which instantiates its share of launch_conv and with it its share of the conv
// kernels; the rest of the library calls launch_conv through fiunet_internal.h.
#pragma once
#include "fiunet_internal.h"
#include "conv3x3_kwave.hip.h"

#include <atomic>
#include <cstdio>

namespace fiunet {
namespace {

// One conv kernel on `nblk` workgroups of 256 threads with `lds` bytes of dynamic LDS: more than 64 KiB needs the opt-in
// attribute, set once per kernel and device (a duplicate hipFuncSetAttribute is harmless); `name` is what the profiler
// reports for the stage (fiunet_profile_read).
template <auto Kernel>
int launch_lds(const char* name, long long nblk, int lds, const ConvArgs& a, hipStream_t s)
{
    if (name_out()) *name_out() = name;
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

template <typename T, int BN, int TH, int TW, int MODE, int EPI>
int launch_conv_cfg(ConvArgs a, hipStream_t s)
{
    char name[128] = "";
    if (name_out())
        std::snprintf(name, sizeof name, "conv3x3_mfma_kernel<%s,%d,%d,%d,%d,%d>", elem_name<T>(), BN, TH, TW,
                      MODE, EPI);
    a.tilesX = (a.W + TW - 1) / TW;
    a.tilesY = (a.H + TH - 1) / TH;
    a.nct = a.Cout / BN;
    const long long nblk = (long long)a.B * a.tilesX * a.tilesY * a.nct * (epi_is_splitk(EPI) ? a.ksplit : 1);
    return launch_lds<&conv3x3_mfma_kernel<T, BN, TH, TW, MODE, EPI>>(name, nblk, ConvTile<BN, TH, TW, MODE>::LDS_BYTES, a, s);
}

// The K loop cut over the four waves of a workgroup (small problems, direct sources, every precision): conv3x3_kwave.hip.h.
template <typename T, int EPI, bool X2> int launch_kwave(ConvArgs a, hipStream_t s)
{
    using Tile = KWaveTile;
    char name[96] = "";
    if (name_out())
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
            if (name_out()) *name_out() += "+splitk" + std::to_string(ksplit);
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

}  // namespace

// (fiunet_internal.h says what the arguments are)
template <typename T> int launch_conv(const ConvArgs& a, int mode, int epi, const ConvCfg& cfg, hipStream_t s)
{
    constexpr int PL = Elem<T>::PL;
    if (a.C0 % PL || a.C1 % PL) return fail(FIUNET_ERR_INVALID_ARG, "channels not a plane multiple");
    if (mode == SRC_CONCAT_UP && epi == EPI_PLAIN) return launch_conv_shape<T, SRC_CONCAT_UP, EPI_PLAIN>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_PLAIN) return launch_conv_shape<T, SRC_DIRECT, EPI_PLAIN>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_HEAD) return launch_conv_shape<T, SRC_DIRECT, EPI_HEAD>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_HEAD3) return launch_conv_shape<T, SRC_DIRECT, EPI_HEAD3>(a, cfg, s);
    if (mode == SRC_DIRECT && epi == EPI_POOL) return launch_conv_shape<T, SRC_DIRECT, EPI_POOL>(a, cfg, s);
    if constexpr (std::is_same_v<T, __bf16>) {   // FIUNET_BF16X2: two-piece operands (conv_bf16x2.hip)
        if (src_is_x2(mode)) return launch_conv_x2(a, mode, epi, cfg, s);
    }
    if constexpr (sizeof(T) == 2) {   // the fused gray stem (bf16, fp16): 32-wide tiles only (the patch layout)
        if (mode == SRC_STEM && epi == EPI_POOL && a.Cout == 64)
            return cfg.small ? launch_conv_cfg<T, 64, 8, 32, SRC_STEM, EPI_POOL>(a, s)
                             : launch_conv_cfg<T, 64, 16, 32, SRC_STEM, EPI_POOL>(a, s);
    }
    return fail(FIUNET_ERR_INVALID_ARG, "unsupported gather/epilogue combination");
}

}  // namespace fiunet
