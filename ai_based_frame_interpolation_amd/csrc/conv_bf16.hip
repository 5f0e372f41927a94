// conv_bf16.hip -- the conv kernels of FIUNET_BF16 (one-piece gather modes; FIUNET_BF16X2: conv_bf16x2.hip): launch_conv<__bf16> and with it every conv3x3_mfma_kernel,
// splitk_finalize_tile_kernel and conv3x3_kwave_kernel instantiation of that element type.
#include "conv_launch.hip.h"

namespace fiunet {

template int launch_conv<__bf16>(const ConvArgs&, int, int, const ConvCfg&, hipStream_t);

}  // namespace fiunet
