// f16 instantiations of the producer/consumer 32x32x16-MFMA convolution kernel (conv_m32p_kernel.h).
#include <type_traits>

#include "conv_m32p_kernel.h"

namespace scpose {
int32_t conv_m32p_dispatch_f16(int stride, int mr, int nr, int c16, const ConvLaunch& L, size_t lds, hipStream_t st) {
  return m32p_dispatch<1>(stride, mr, nr, c16, L, lds, st);
}
}  // namespace scpose
