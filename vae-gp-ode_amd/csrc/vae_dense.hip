// vae_dense.hip -- the conv VAE's elementwise activations and linear layers (encoder fc vae.py:58-62, decoder fc vae.py:66), fp32.
#include <hip/hip_runtime.h>
#include "gp_launch.hpp"
#include "wave_reduce.hpp"

namespace gp {

// elementwise activations: mode 0 relu, 1 sigmoid
__global__ void k_act_fwd(const float* __restrict__ x, float* __restrict__ y, size_t n, int mode) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float v = x[e];
    y[e] = mode == 0 ? fmaxf(v, 0.f) : 1.f / (1.f + expf(-v));
  }
}
__global__ void k_act_bwd(const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ gx, size_t n, int mode) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float v = y[e];
    gx[e] = mode == 0 ? (v > 0.f ? gy[e] : 0.f) : gy[e] * v * (1.f - v);
  }
}

// Linear: y[b,o] = bias[o] + sum_i x[b,i] w[o,i]
__global__ void k_linear_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                             float* __restrict__ y, int B, int In, int Out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)B * Out) return;
  const int b = (int)(e / Out), o = (int)(e % Out);
  float acc = bias ? bias[o] : 0.f;
  const float* xr = x + (size_t)b * In;
  const float* wr = w + (size_t)o * In;
  for (int i = 0; i < In; ++i) acc = fmaf(xr[i], wr[i], acc);
  y[e] = acc;
}
// xpre != nullptr: the layer's input was relu(xpre) (applied on load by the forward) -- the gradient passes where xpre > 0
__global__ void k_linear_bwd_x(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ gx, int B, int In, int Out,
                               const float* __restrict__ xpre) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)B * In) return;
  const int b = (int)(e / In), i = (int)(e % In);
  float acc = 0.f;
  for (int o = 0; o < Out; ++o) acc = fmaf(gy[(size_t)b * Out + o], w[(size_t)o * In + i], acc);
  gx[e] = (xpre && !(xpre[e] > 0.f)) ? 0.f : acc;
}
// gw[o,i] = sum_b gy[b,o] x[b,i]; gb[o] = sum_b gy[b,o].  One wave per (o,i) (i == In -> bias).
__global__ __launch_bounds__(256) void k_linear_bwd_w(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gw,
                                                       float* __restrict__ gb, int B, int In, int Out, int relu_in) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= Out * (In + 1)) return;
  const int o = wave / (In + 1), i = wave % (In + 1);
  if (i < In ? !gw : !gb) return;                    // gw == NULL: only the bias column is summed
  float acc = 0.f;
  for (int b = lane; b < B; b += 64) {
    float xv = i < In ? x[(size_t)b * In + i] : 1.f;
    if (relu_in && i < In) xv = fmaxf(xv, 0.f);
    acc = fmaf(gy[(size_t)b * Out + o], xv, acc);
  }
  float in1[1] = {acc}, out1[1];
  wave_sum_multi<1>(in1, out1);
  if (lane == 0) { if (i < In) gw[(size_t)o * In + i] = out1[0]; else gb[o] = out1[0]; }
}

// The same sums for the decoder's fc layer at thousands of rows (q -> 512 on batch x T latent states, vae.py:101): a workgroup owns 64
// consecutive outputs and a slab of rows -- gy is read in 256-byte rows (one wavefront per (o, i) pair re-read every cache line of gy
// 16 times through 2 KB strides: 36 us at 4096 rows), x[b][i] is wave-uniform.  partW[slab][o][i], partB[slab][o] are summed in a
// fixed order by reduce_jobs.  grid (Out / 64, nslab), block 256 = 64 outputs x 4 row groups.
//
// The slab is walked in tiles of LINW_TILE rows, and everything a tile needs is requested before its first FMA: a thread's
// LINW_TILE / 4 values of gy (clamped row index, no branch around the load; a row past the tile is loaded twice and not used), and
// the tile's rows of x, which the workgroup copies to LDS with one coalesced load and reads back as broadcasts.  (A thread that
// loaded gy and x row by row waited out one memory latency per four rows: 23 us for 8 MB.)  Each accumulator still takes its rows
// in the order b0 + g, b0 + g + 4, ...
constexpr int LINW_SLABS = 32;
constexpr int LINW_TILE = 128;
__global__ __launch_bounds__(256) void k_linear_bwd_w_cols(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ partW,
                                                            float* __restrict__ partB, int B, int In, int Out, int rps) {
  __shared__ float red[4][9][64];
  __shared__ float xs[LINW_TILE * 8];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, o = blockIdx.x * 64 + lane;
  const int b0 = blockIdx.y * rps, b1 = min(B, b0 + rps);
  float acc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = 0.f;
  for (int t0 = b0; t0 < b1; t0 += LINW_TILE) {
    const int nr = min(LINW_TILE, b1 - t0);          // >= 1
    float gv[LINW_TILE / 4];
#pragma unroll
    for (int k = 0; k < LINW_TILE / 4; ++k) gv[k] = gy[(size_t)(t0 + min(g + 4 * k, nr - 1)) * Out + o];
    if (t0 != b0) __syncthreads();                   // the previous tile's readers are done with xs
    for (int e = threadIdx.x; e < nr * In; e += 256) xs[e] = x[(size_t)t0 * In + e];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LINW_TILE / 4; ++k) {
      const int r = g + 4 * k;
      if (r < nr) {
        const float* xr = xs + r * In;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < In) acc[i] = fmaf(gv[k], xr[i], acc[i]);
        acc[8] += gv[k];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) red[g][i][lane] = acc[i];
  __syncthreads();
  for (int e = threadIdx.x; e < 9 * 64; e += 256) {
    const int i = e >> 6, l = e & 63, oo = blockIdx.x * 64 + l;
    const float v = (red[0][i][l] + red[1][i][l]) + (red[2][i][l] + red[3][i][l]);
    if (i < In) partW[((size_t)blockIdx.y * Out + oo) * In + i] = v;
    else if (i == 8) partB[(size_t)blockIdx.y * Out + oo] = v;
  }
}

// ---- wide fan-in, few outputs (the encoder's fc layer, 512 -> 2q on the minibatch, vae.py:62): one wavefront per output
//      element, lanes along the reduction
__global__ __launch_bounds__(256) void k_linear_fwd_fanin(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, int B, int In, int Out,
                                                           int relu_in) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= B * Out) return;
  const int b = e / Out, o = e % Out;
  const float* xr = x + (size_t)b * In;
  const float* wr = w + (size_t)o * In;
  float acc = 0.f;
  if (relu_in) { for (int i = lane; i < In; i += 64) acc = fmaf(fmaxf(xr[i], 0.f), wr[i], acc); }
  else { for (int i = lane; i < In; i += 64) acc = fmaf(xr[i], wr[i], acc); }
  const float in1[1] = {acc};
  float out1[1];
  wave_sum_multi<1>(in1, out1);
  if (lane == 0) y[e] = out1[0] + (bias ? bias[o] : 0.f);
}

// ---- small fan-in (In <= 16, Out a multiple of 64): the decoder's fc layer (latent -> 512, vae.py:66) on all
//      batch*T latent states.  Threads run along Out (coalesced rows of y / gy); the few weights per output live in
//      registers.
constexpr int LIN_MAXIN = 16;
__global__ __launch_bounds__(256) void k_linear_fwd_fanout(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, int B, int In, int Out,
                                                            int rows_per_block) {
  const int b0 = blockIdx.x * rows_per_block, b1 = min(B, b0 + rows_per_block);
  // (grid.y splits Out: one pass per thread -- a second pass waited out a second round of weight loads)
  for (int o = blockIdx.y * 256 + threadIdx.x; o < Out; o += 256 * gridDim.y) {
    float wr[LIN_MAXIN];
#pragma unroll
    for (int i = 0; i < LIN_MAXIN; ++i) wr[i] = i < In ? w[(size_t)o * In + i] : 0.f;
    const float bo = bias ? bias[o] : 0.f;
    for (int b = b0; b < b1; ++b) {
      const float* xr = x + (size_t)b * In;          // wave-uniform
      float acc = bo;
#pragma unroll
      for (int i = 0; i < LIN_MAXIN; ++i)
        if (i < In) acc = fmaf(xr[i], wr[i], acc);
      y[(size_t)b * Out + o] = acc;
    }
  }
}
// gx[b][i] = sum_o gy[b][o] w[o][i]: one wavefront per row b, lanes along o
template <int OPL>  // outputs per lane = Out / 64
__global__ __launch_bounds__(256) void k_linear_bwd_x_fanout(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ gx,
                                                              int B, int In) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = gridDim.x * 4;
  constexpr int Out = OPL * 64;
  float wr[OPL][LIN_MAXIN];
#pragma unroll
  for (int k = 0; k < OPL; ++k)
#pragma unroll
    for (int i = 0; i < LIN_MAXIN; ++i) wr[k][i] = i < In ? w[(size_t)(lane + 64 * k) * In + i] : 0.f;
  for (int b = blockIdx.x * 4 + wave; b < B; b += nw) {
    float acc[LIN_MAXIN];
#pragma unroll
    for (int i = 0; i < LIN_MAXIN; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < OPL; ++k) {
      const float g = gy[(size_t)b * Out + lane + 64 * k];
#pragma unroll
      for (int i = 0; i < LIN_MAXIN; ++i) acc[i] = fmaf(g, wr[k][i], acc[i]);
    }
    float tot[LIN_MAXIN];
    wave_sum_all<LIN_MAXIN>(acc, tot);
    if (lane < In) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < LIN_MAXIN; ++i) v = (lane == i) ? tot[i] : v;
      gx[(size_t)b * In + lane] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
int act_fwd(const float* x, float* y, size_t n, int mode, hipStream_t st) {
  hipLaunchKernelGGL(k_act_fwd, ew_grid(n), 256, 0, st, x, y, n, mode);
  return check_launch("act_fwd");
}
int act_bwd(const float* y, const float* gy, float* gx, size_t n, int mode, hipStream_t st) {
  hipLaunchKernelGGL(k_act_bwd, ew_grid(n), 256, 0, st, y, gy, gx, n, mode);
  return check_launch("act_bwd");
}

int linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, hipStream_t st) {
  if (In <= LIN_MAXIN && Out % 64 == 0 && B >= 256) {
    const int rows = 8;
    hipLaunchKernelGGL(k_linear_fwd_fanout, dim3((B + rows - 1) / rows, (Out + 255) / 256), 256, 0, st, x, w, bias, y, B, In, Out, rows);
    return check_launch("linear_fwd_fanout");
  }
  if (In >= 128 && (size_t)B * Out <= (size_t)1 << 22) {
    hipLaunchKernelGGL(k_linear_fwd_fanin, (unsigned)(((size_t)B * Out + 3) / 4), 256, 0, st, x, w, bias, y, B, In, Out, 0);
    return check_launch("linear_fwd_fanin");
  }
  hipLaunchKernelGGL(k_linear_fwd, (unsigned)(((size_t)B * Out + 255) / 256), 256, 0, st, x, w, bias, y, B, In, Out);
  return check_launch("linear_fwd");
}
size_t linear_bwd_scratch(int B, int In, int Out) { (void)B; return (size_t)LINW_SLABS * Out * (In + 1); }

int linear_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out, float* scratch,
               hipStream_t st) {
  if (In <= LIN_MAXIN && Out % 64 == 0 && Out <= 512 && B >= 256) {
    const int nb = B / 4 < 256 ? (B + 3) / 4 : 256;
    if (gx) {
      switch (Out / 64) {
#define X(k) case k: hipLaunchKernelGGL(k_linear_bwd_x_fanout<k>, nb, 256, 0, st, gy, w, gx, B, In); break;
        X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
      }
    }
    bool slabs = false;
    if (gw || gb) {
      if (gw && scratch && In <= 8 && B >= 1024) {
        slabs = true;
        const int rps = (B + LINW_SLABS - 1) / LINW_SLABS, used = (B + rps - 1) / rps;
        float* partW = scratch;
        float* partB = scratch + (size_t)LINW_SLABS * Out * In;
        hipLaunchKernelGGL(k_linear_bwd_w_cols, dim3(Out / 64, used), 256, 0, st, x, gy, partW, partB, B, In, Out, rps);
        const RedJob jobs[2] = {RedJob{partW, gw, used, Out * In, 0, 0, 0, 0}, RedJob{partB, gb, used, Out, 0, 0, 0, 0}};
        if (reduce_jobs(jobs, gb ? 2 : 1, st)) return 1;
      } else {
        hipLaunchKernelGGL(k_linear_bwd_w, (unsigned)(((size_t)Out * (In + 1) * 64 + 255) / 256), 256, 0, st, x, gy, gw, gb, B, In, Out, 0);
      }
    }
    return check_launch(slabs ? "linear_bwd_fanout (row slabs)" : "linear_bwd_fanout");
  }
  if (gx) hipLaunchKernelGGL(k_linear_bwd_x, (unsigned)(((size_t)B * In + 255) / 256), 256, 0, st, gy, w, gx, B, In, Out, (const float*)nullptr);
  if (gw || gb) hipLaunchKernelGGL(k_linear_bwd_w, (unsigned)(((size_t)Out * (In + 1) * 64 + 255) / 256), 256, 0, st, x, gy, gw, gb, B, In, Out, 0);
  return check_launch("linear_bwd");
}

// y = relu(x) W^T + b and its backward with the ReLU of the INPUT folded in (the encoder's cnn.6 -> ReLU -> Flatten -> fc,
// vae.py:58-61, 72-74): x is the convolution's raw output; no activation tensor, no separate ReLU launches.  Wide fan-in only.
int linear_relu_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, hipStream_t st) {
  if (In < 128 || (size_t)B * Out > ((size_t)1 << 22)) return set_error("gpode_linear_relu_fwd: built for wide fan-in layers (In >= 128)");
  hipLaunchKernelGGL(k_linear_fwd_fanin, (unsigned)(((size_t)B * Out + 3) / 4), 256, 0, st, x, w, bias, y, B, In, Out, 1);
  return check_launch("linear_relu_fwd");
}
int linear_relu_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out, hipStream_t st) {
  if (In < 128) return set_error("gpode_linear_relu_bwd: built for wide fan-in layers (In >= 128)");
  if (gx) hipLaunchKernelGGL(k_linear_bwd_x, (unsigned)(((size_t)B * In + 255) / 256), 256, 0, st, gy, w, gx, B, In, Out, x);
  if (gw || gb) hipLaunchKernelGGL(k_linear_bwd_w, (unsigned)(((size_t)Out * (In + 1) * 64 + 255) / 256), 256, 0, st, x, gy, gw, gb, B, In, Out, 1);
  return check_launch("linear_relu_bwd");
}

}  // namespace gp
