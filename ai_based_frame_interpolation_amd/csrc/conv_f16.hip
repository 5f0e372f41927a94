// conv_f16.hip -- the conv kernels of FIUNET_FP16: launch_conv<_Float16> and with it every conv3x3_mfma_kernel,
// splitk_finalize_tile_kernel and conv3x3_kwave_kernel instantiation of that element type.
#include "conv_launch.hip.h"

namespace fiunet {

template int launch_conv<_Float16>(const ConvArgs&, int, int, const ConvCfg&, hipStream_t);

}  // namespace fiunet
