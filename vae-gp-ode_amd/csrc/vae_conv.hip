// vae_conv.hip -- conv VAE building blocks (encoder vae.py:47-98, decoder vae.py:101-153), NCHW fp32.
//
// Three convolution kernels cover all seven layers, forward and backward:
//   conv_fwd        y  = conv(x, w) + b                          Conv2d forward;  ConvTranspose2d d/d input
//   conv_bwd_data   gx = sum_co sum_taps gy * w  (+ b)           Conv2d d/d input; ConvTranspose2d FORWARD
//   conv_bwd_weight gw = sum_{b,oy,ox} gy * x                    both (roles of x / gy swap for ConvTranspose2d)
// nn.ConvTranspose2d stores its weight as (C_in, C_out, k, k), which is exactly the (Co, Ci, k, k) weight of
// the convolution it is the adjoint of -- the same buffer serves both directions.
// K (kernel size) and STRIDE are template parameters so the tap loops unroll and the stride test of the
// transposed direction folds into the loop bounds (only contributing taps are visited).
//
// Round-1 status: direct (gather) form, one thread per output element, weights/inputs through L1/L2.
// This is the correctness baseline of the decoder; the LDS-resident implicit-GEMM MFMA version of the two
// FLOP-dominant layers (decnn.4, decnn.7) is the next optimisation step.
#include <hip/hip_runtime.h>
#include "gp_launch.hpp"
#include "bn_sink.hpp"
#include "wave_reduce.hpp"

namespace gp {

struct ConvDims { int B, Ci, H, W, Co, P, Ho, Wo; size_t xbs; };   // xbs: floats between consecutive images of x (dense: Ci * H * W)
int chan_sum(const float* v, float* out, int B, int C, int HW, float* scratch, hipStream_t st);

template <int K, int S>
__global__ __launch_bounds__(256) void k_conv_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ y, ConvDims d) {
  const size_t total = (size_t)d.B * d.Co * d.Ho * d.Wo;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(e % d.Wo), oy = (int)((e / d.Wo) % d.Ho), co = (int)((e / ((size_t)d.Wo * d.Ho)) % d.Co);
    const int b = (int)(e / ((size_t)d.Wo * d.Ho * d.Co));
    float acc = bias ? bias[co] : 0.f;
    const int iy0 = oy * S - d.P, ix0 = ox * S - d.P;
    const float* xb = x + (size_t)b * d.xbs;
    const float* wc = w + (size_t)co * d.Ci * K * K;
    for (int ci = 0; ci < d.Ci; ++ci) {
      const float* xc = xb + (size_t)ci * d.H * d.W;
      const float* wk = wc + ci * K * K;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int iy = iy0 + ky;
        if (iy < 0 || iy >= d.H) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ix0 + kx;
          if (ix < 0 || ix >= d.W) continue;
          acc = fmaf(xc[iy * d.W + ix], wk[ky * K + kx], acc);
        }
      }
    }
    y[e] = acc;
  }
}

// gx[b,ci,iy,ix] = bias[ci] + sum_{co,ky,kx} gy[b,co,oy,ox] w[co,ci,ky,kx],  oy = (iy + P - ky)/S when divisible
template <int K, int S>
__global__ __launch_bounds__(256) void k_conv_bwd_data(const float* __restrict__ gy, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ gx, ConvDims d) {
  const size_t total = (size_t)d.B * d.Ci * d.H * d.W;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int ix = (int)(e % d.W), iy = (int)((e / d.W) % d.H), ci = (int)((e / ((size_t)d.W * d.H)) % d.Ci);
    const int b = (int)(e / ((size_t)d.W * d.H * d.Ci));
    float acc = bias ? bias[ci] : 0.f;
    const float* gb = gy + (size_t)b * d.Co * d.Ho * d.Wo;
    const int ky0 = (iy + d.P) % S, kx0 = (ix + d.P) % S;  // only taps with (iy + P - ky) % S == 0 contribute
    for (int co = 0; co < d.Co; ++co) {
      const float* gc = gb + (size_t)co * d.Ho * d.Wo;
      const float* wk = w + ((size_t)co * d.Ci + ci) * K * K;
#pragma unroll
      for (int t = 0; t < (K + S - 1) / S; ++t) {
        const int ky = ky0 + t * S;
        if (ky >= K) continue;
        const int oy = (iy + d.P - ky) / S;
        if (iy + d.P - ky < 0 || oy >= d.Ho) continue;
#pragma unroll
        for (int u = 0; u < (K + S - 1) / S; ++u) {
          const int kx = kx0 + u * S;
          if (kx >= K) continue;
          const int ox = (ix + d.P - kx) / S;
          if (ix + d.P - kx < 0 || ox >= d.Wo) continue;
          acc = fmaf(gc[oy * d.Wo + ox], wk[ky * K + kx], acc);
        }
      }
    }
    gx[e] = acc;
  }
}

// gw[co,ci,ky,kx] = sum_{b,oy,ox} gy[b,co,oy,ox] x[b,ci,oy*S-P+ky,ox*S-P+kx].  grid (Co*Ci, nsplit): each workgroup
// sums a slice of the batch for one (co,ci) pair into part[split][co][ci][K*K]; a second kernel adds the splits.
template <int K, int S>
__global__ __launch_bounds__(256) void k_conv_bwd_weight(const float* __restrict__ x, const float* __restrict__ gy,
                                                          float* __restrict__ part, ConvDims d, int b_per_split) {
  __shared__ float red[4][K * K];
  const int co = blockIdx.x / d.Ci, ci = blockIdx.x % d.Ci;
  const int b0 = blockIdx.y * b_per_split, b1 = min(d.B, b0 + b_per_split);
  float acc[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
  const int npix = d.Ho * d.Wo;
  const size_t work = (size_t)(b1 - b0) * npix;
  for (size_t e = threadIdx.x; e < work; e += 256) {
    const int b = b0 + (int)(e / npix), p = (int)(e % npix);
    const int oy = p / d.Wo, ox = p % d.Wo;
    const float g = gy[((size_t)b * d.Co + co) * npix + p];
    const float* xc = x + (size_t)b * d.xbs + (size_t)ci * d.H * d.W;
    const int iy0 = oy * S - d.P, ix0 = ox * S - d.P;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = iy0 + ky;
      const bool oky = iy >= 0 && iy < d.H;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ix0 + kx;
        const float xv = (oky && ix >= 0 && ix < d.W) ? xc[iy * d.W + ix] : 0.f;
        acc[ky * K + kx] = fmaf(g, xv, acc[ky * K + kx]);
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < K * K; ++t) {
    const float s = row_allreduce16(acc[t]);  // 16-lane rows; the four rows are added below
    float tot = GP_LANE(s, 0) + GP_LANE(s, 16) + GP_LANE(s, 32) + GP_LANE(s, 48);
    if (lane == 0) red[wv][t] = tot;
  }
  __syncthreads();
  if (threadIdx.x < K * K)
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (K * K) + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void k_sum_splits(const float* __restrict__ part, int nsplit, size_t n, float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float acc = 0.f;
  for (int s = 0; s < nsplit; ++s) acc += part[(size_t)s * n + e];
  out[e] = acc;
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------

#define GP_CONV_KS(X) X(5, 2) X(5, 1) X(3, 1) X(3, 2)

// LDS-tiled specialisations of the heavy decoder layers (vae_conv_tiled.hip); -1 = geometry not covered
int tiled_fwd(const float* x, const float* w, const float* bias, float* y, const ConvGeom& g, hipStream_t st);
int tiled_bwd_data(const float* gy, const float* w, const float* bias, float* gx, const ConvGeom& g, const float* in_bn, hipStream_t st,
                   const BnSink* sink);
int tiled_bwd_weight(const float* x, const float* gy, float* gw, float* scratch, const ConvGeom& g, const float* in_bn, hipStream_t st);

// what the direct kernels take; xbs = 0: x is dense
static ConvDims conv_dims(const ConvGeom& g, size_t xbs) {
  return ConvDims{g.B, g.Ci, g.H, g.W, g.Co, g.P, g.Ho, g.Wo, xbs ? xbs : (size_t)g.Ci * g.H * g.W};
}

// xbs != 0: x is batch-strided (xbs floats between images, each image dense) -- generic kernels only
int conv2d_fwd(const float* x, const float* w, const float* bias, float* y, const ConvGeom& g, hipStream_t st, size_t xbs) {
  if (xbs == (size_t)g.Ci * g.H * g.W) xbs = 0;
  if (!xbs) { const int r = tiled_fwd(x, w, bias, y, g, st); if (r >= 0) return r; }
  else if (g.Ci % 4 == 0) return set_error("gpode_conv2d_fwd_bs: batch-strided input is for the generic kernels (input channels not a multiple of 4)");
  const ConvDims d = conv_dims(g, xbs);
  const size_t total = (size_t)g.B * g.Co * g.Ho * g.Wo;
#define X(k, s) if (g.K == k && g.S == s) { hipLaunchKernelGGL((k_conv_fwd<k, s>), ew_grid(total), 256, 0, st, x, w, bias, y, d); return check_launch("conv_fwd"); }
  GP_CONV_KS(X)
#undef X
  return set_error("gpode_conv2d_fwd: kernel %d stride %d not built", g.K, g.S);
}

// gy_bn (optional, [Co][4] = mean, invstd, gamma, beta): gy is the raw output of the previous layer and the BatchNorm + ReLU
// between the two layers is applied on the fly (matrix-core specialisations only)
// ConvTranspose2d forward that also produces the training-mode BatchNorm statistics of its output (bn_sink.hpp): matrix-core
// specialisations only.  scratch: convT_fwd_stats_scratch() floats; slot: which of the library's ticket counters this layer uses
// (launches that may run concurrently need different slots).
__device__ unsigned g_bn_sink_tickets[64];
size_t convT_fwd_stats_scratch(int Co_out) { return (size_t)512 * Co_out * 2; }
int convT_fwd_stats(const float* x, const float* x_bn, const float* w, const float* bias, float* y, const ConvGeom& g, const float* gamma,
                    const float* beta, float* save_mean, float* save_invstd, float* running_mean, float* running_var, long long* nbt,
                    float momentum, float eps, float* table, float* scratch, int slot, hipStream_t st) {
  static unsigned* tickets = nullptr;
  if (!tickets) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_bn_sink_tickets)) != hipSuccess) return set_error("gpode_convT_fwd_stats: no ticket storage");
    tickets = static_cast<unsigned*>(p);
  }
  if (slot < 0 || slot >= 64) return set_error("gpode_convT_fwd_stats: slot 0 .. 63");
  BnSink sink{scratch, tickets + slot, gamma, beta, save_mean, save_invstd, running_mean, running_var, nbt, table, momentum, eps,
              (float)g.B * (float)(g.H * g.W)};
  const int r = tiled_bwd_data(x, w, bias, y, g, x_bn, st, &sink);
  return r < 0 ? set_error("gpode_convT_fwd_stats: no specialisation for this geometry") : r;
}

int conv2d_bwd_data(const float* gy, const float* w, const float* bias, float* gx, const ConvGeom& g, const float* gy_bn, hipStream_t st) {
  { const int r = tiled_bwd_data(gy, w, bias, gx, g, gy_bn, st, nullptr); if (r >= 0) return r; }
  if (gy_bn) return set_error("gpode_conv2d_bwd_data_bn: no matrix-core specialisation for this geometry");
  const ConvDims d = conv_dims(g, 0);
  const size_t total = (size_t)g.B * g.Ci * g.H * g.W;
#define X(k, s) if (g.K == k && g.S == s) { hipLaunchKernelGGL((k_conv_bwd_data<k, s>), ew_grid(total), 256, 0, st, gy, w, bias, gx, d); return check_launch("conv_bwd_data"); }
  GP_CONV_KS(X)
#undef X
  return set_error("gpode_conv2d_bwd_data: kernel %d stride %d not built", g.K, g.S);
}

static inline int pick_split(int B, int nblocks_per_split) {
  int s = 1024 / (nblocks_per_split > 0 ? nblocks_per_split : 1);  // aim for ~1024 workgroups
  if (s < 1) s = 1;
  if (s > B) s = B;
  if (s > 64) s = 64;
  return s;
}

// scratch: conv_wgrad_scratch_floats(...) floats
size_t conv_wgrad_scratch(int B, int Ci, int Co, int K) {
  const size_t generic = (size_t)pick_split(B, Co * Ci) * Co * Ci * K * K + (size_t)64 * Co * 2;
  // the tiled weight-gradient kernels split the batch into up to 512 slabs (two workgroups per CU) of Co*Ci*K*K floats
  const size_t tiled = (size_t)(B < 512 ? B : 512) * Co * Ci * K * K + (size_t)64 * Co * 2;
  return generic > tiled ? generic : tiled;
}

int conv2d_bwd_weight(const float* x, const float* gy, float* gw, float* gbias, float* scratch, const ConvGeom& g, const float* gy_bn,
                      hipStream_t st, size_t xbs) {
  const int B = g.B, Ci = g.Ci, Co = g.Co, K = g.K;
  if (xbs == (size_t)Ci * g.H * g.W) xbs = 0;
  if (xbs && Ci % 4 == 0) return set_error("gpode_conv2d_bwd_weight_bs: batch-strided input is for the generic kernels");
  // chan_sum's own argument check, made before the weight gradient is launched: a refused call writes nothing
  if (gbias && ((g.Ho * g.Wo) & 3) == 0 && !aligned16(gy)) return set_error("gpode_conv2d_bwd_weight: the bias gradient needs a 16-byte aligned gy");
  if (!xbs) {
    const int r = tiled_bwd_weight(x, gy, gw, scratch, g, gy_bn, st);
    if (r > 0) return r;
    if (r == 0) {
      // the bias partials go BEHIND the weight-gradient slabs (the tail conv_wgrad_scratch reserves): with deferred reductions
      // (gpode_defer_reductions) the slabs are still unread when k_chan_sum runs
      if (gbias) return chan_sum(gy, gbias, B, Co, g.Ho * g.Wo, scratch + (size_t)(B < 512 ? B : 512) * Co * Ci * K * K, st);
      return 0;
    }
  }
  if (gy_bn) return set_error("gpode_conv2d_bwd_weight_bn: no matrix-core specialisation for this geometry");
  const ConvDims d = conv_dims(g, xbs);
  const int nsplit = pick_split(B, Co * Ci);
  const int bps = (B + nsplit - 1) / nsplit;
  const int used = (B + bps - 1) / bps;
  const size_t n = (size_t)Co * Ci * K * K;
  bool ok = false;
#define X(k, s) if (K == k && g.S == s) { hipLaunchKernelGGL((k_conv_bwd_weight<k, s>), dim3(Co * Ci, used), 256, 0, st, x, gy, scratch, d, bps); ok = true; }
  GP_CONV_KS(X)
#undef X
  if (!ok) return set_error("gpode_conv2d_bwd_weight: kernel %d stride %d not built", K, g.S);
  if (reduce_job(RedJob{scratch, gw, used, (int)n, 0, 0, 0, 0}, st)) return 1;
  if (gbias) return chan_sum(gy, gbias, B, Co, g.Ho * g.Wo, scratch + (size_t)nsplit * n, st);
  return check_launch("conv_bwd_weight");
}

}  // namespace gp
