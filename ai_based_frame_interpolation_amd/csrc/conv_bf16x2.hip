// conv_bf16x2.hip -- the conv kernels of FIUNET_BF16X2: the two-piece gather modes SRC_DIRECT_X2 / SRC_STEM_X2 of __bf16,
// with their splitk_finalize_tile_kernel and conv3x3_kwave_kernel instantiations.
#include "conv_launch.hip.h"

namespace fiunet {

int launch_conv_x2(const ConvArgs& a, int mode, int epi, const ConvCfg& cfg, hipStream_t s)
{
    using T = __bf16;
    if (mode == SRC_DIRECT_X2 && epi == EPI_PLAIN) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_PLAIN>(a, cfg, s);
    if (mode == SRC_DIRECT_X2 && epi == EPI_POOL) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_POOL>(a, cfg, s);
    if (mode == SRC_DIRECT_X2 && epi == EPI_HEAD) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_HEAD>(a, cfg, s);
    if (mode == SRC_DIRECT_X2 && epi == EPI_HEAD3) return launch_conv_shape<T, SRC_DIRECT_X2, EPI_HEAD3>(a, cfg, s);
    if (mode == SRC_STEM_X2 && epi == EPI_POOL && a.Cout == 64)
        return cfg.small ? launch_conv_cfg<T, 64, 8, 32, SRC_STEM_X2, EPI_POOL>(a, s)
                         : launch_conv_cfg<T, 64, 16, 32, SRC_STEM_X2, EPI_POOL>(a, s);
    return fail(FIUNET_ERR_INVALID_ARG, "unsupported gather/epilogue combination");
}

}  // namespace fiunet
