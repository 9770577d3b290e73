// vae_conv_v2.hip -- launchers of the second convolution engine (conv_bwd_v2.hpp): decnn.7 and decnn.4 d/d input.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gp_launch.hpp"
#include "conv_layers.hpp"
#include "conv_bwd_v2.hpp"

namespace gp {

template <class L> static int launch_bwd_data_v2(const float* gy, const float* w, float* gx, int B, hipStream_t st, const char* what) {
  using E = BdV2<L>;
  constexpr size_t lds = E::lds_bytes();
  static_assert(lds <= 160 * 1024, "LDS budget");
  auto km = k_conv_bwd_data_v2<L>;
  if (set_max_lds((const void*)km, lds)) return 1;
  hipLaunchKernelGGL(km, B < num_cus() ? B : num_cus(), E::NTHR, lds, st, gy, w, gx, B);
  return check_launch(what);
}

int conv_v2_dec7_bwd_data(const float* gy, const float* w, float* gx, int B, hipStream_t st) {
  return launch_bwd_data_v2<Dec7>(gy, w, gx, B, st, "conv_v2_dec7_bwd_data");
}

int conv_v2_dec4_bwd_data(const float* gy, const float* w, float* gx, int B, hipStream_t st) {
  return launch_bwd_data_v2<Dec4>(gy, w, gx, B, st, "conv_v2_dec4_bwd_data");
}

}  // namespace gp
