// vae_conv_v2.hip -- launchers of the second convolution engine: decnn.7 and decnn.4 d/d input (conv_bwd_v2.hpp), decnn.7 forward
// (conv_fwd_v2.hpp).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gp_launch.hpp"
#include "conv_layers.hpp"
#include "conv_bwd_v2.hpp"
#include "conv_fwd_v2.hpp"

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

template <class L, bool HAS_BN, bool STATS>
static int launch_fwd_v2(const float* x, const float* w, const float* bias, float* y, int B, const float* in_bn, const BnSink* sink,
                         hipStream_t st, const char* what) {
  using E = FwV2<L>;
  constexpr size_t lds = E::lds_bytes(STATS);
  static_assert(lds + (STATS ? sizeof(float) * (E::NTHR + 1) : 0) <= 160 * 1024, "LDS budget (with bn_sink_publish's static arrays)");
  auto km = k_conv_fwd_v2<L, HAS_BN, STATS>;
  if (set_max_lds((const void*)km, lds)) return 1;
  // a BnSink's scratch holds the partial sums of kSinkMaxWg = 512 workgroups (vae_conv_tiled.hip, convT_fwd_stats_scratch)
  if (STATS && num_cus() > 512) return set_error("%s: more workgroups than the statistics scratch holds", what);
  const int nwork = STATS ? (B + E::IPG - 1) / E::IPG : B;     // STATS: the first engine's grid, one workgroup per image group
  hipLaunchKernelGGL(km, nwork < num_cus() ? nwork : num_cus(), E::NTHR, lds, st, x, w, bias, y, B, in_bn, STATS ? *sink : BnSink{});
  return check_launch(what);
}

// ConvTranspose2d forward of decnn.7: in_bn = nullptr or the {mean, invstd, gamma, beta} table of the BatchNorm + ReLU in front,
// sink = nullptr or where the statistics of the output go (at most num_cus() <= 256 workgroups: within every sink's scratch)
int conv_v2_dec7_fwd(const float* x, const float* w, const float* bias, float* y, int B, const float* in_bn, const BnSink* sink,
                     hipStream_t st) {
  if (in_bn && sink) return launch_fwd_v2<Dec7, true, true>(x, w, bias, y, B, in_bn, sink, st, "conv_v2_dec7_fwd_bn_stats");
  if (sink) return launch_fwd_v2<Dec7, false, true>(x, w, bias, y, B, in_bn, sink, st, "conv_v2_dec7_fwd_stats");
  if (in_bn) return launch_fwd_v2<Dec7, true, false>(x, w, bias, y, B, in_bn, sink, st, "conv_v2_dec7_fwd_bn");
  return launch_fwd_v2<Dec7, false, false>(x, w, bias, y, B, in_bn, sink, st, "conv_v2_dec7_fwd");
}

}  // namespace gp
