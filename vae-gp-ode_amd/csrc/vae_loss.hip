// vae_loss.hip -- the loss stage: Bernoulli likelihood (padded, ragged and compact rows), reparameterisation, the ELBO in one launch,
// the importance-weighted bound and the frame gather of the compact route (create_model.py:40-73, vae.py:75-78, 136-153), fp32.
#include <hip/hip_runtime.h>
#include "gp_launch.hpp"
#include "wave_reduce.hpp"

namespace gp {

// Bernoulli log-likelihood (vae.py:136-153, no epsilon -- SURVEY F9): ll = log(z) X + log(1-z) (1-X).
// z has `reps` copies of X's extent (X.repeat([L,...])): X index = e % nX.
__global__ void k_loglik_fwd(const float* __restrict__ X, const float* __restrict__ z, float* __restrict__ ll, size_t n, size_t nX) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float xv = X[e % nX], zv = z[e];
    ll[e] = logf(zv) * xv + logf(1.f - zv) * (1.f - xv);
  }
}
__global__ void k_loglik_bwd(const float* __restrict__ X, const float* __restrict__ z, const float* __restrict__ g,
                             float* __restrict__ gz, size_t n, size_t nX) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const float xv = X[e % nX], zv = z[e];
    gz[e] = g[e] * (xv / zv - (1.f - xv) / (1.f - zv));
  }
}
// Ragged minibatches (the *_len entry points): a row is (draw, sequence), sequence n = row % N owns the frames t < n_obs[n] of its T
// padded ones, `frame` elements each, so offset p of a row is observed iff p < obs_limit(...) -- a select, never a multiply: what a
// padded target or logit holds (NaN, Inf) reaches no sum and no gradient.  Counts <= 0 mean no frame, counts >= T all of them.
__device__ __forceinline__ size_t obs_limit(const int* __restrict__ n_obs, size_t seq, int T, size_t frame) {
  const int k = n_obs[seq];
  return (size_t)(k < 0 ? 0 : (k > T ? T : k)) * frame;
}
// fused reduction used by the ELBO (create_model.py:52-53): out[row] = sum over `inner` of ll; row = (l,n)
// MASK: the observed terms only (k_loglik_rowsum<false> is the kernel as it was; n_obs, T, frame are not read)
template <bool MASK>
__global__ __launch_bounds__(256) void k_loglik_rowsum(const float* __restrict__ X, const float* __restrict__ z, float* __restrict__ out,
                                                        size_t inner, size_t nX, const int* __restrict__ n_obs, int T, size_t frame) {
  __shared__ float red[4];
  const size_t row = blockIdx.x;
  size_t lim = inner;
  if constexpr (MASK) lim = obs_limit(n_obs, row % (nX / inner), T, frame);
  float acc = 0.f;
  for (size_t p = threadIdx.x; p < lim; p += 256) {
    const size_t e = row * inner + p;
    const float xv = X[e % nX], zv = z[e];
    acc += logf(zv) * xv + logf(1.f - zv) * (1.f - xv);
  }
  float in1[1] = {acc}, out1[1];
  wave_sum_multi<1>(in1, out1);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = out1[0];
  __syncthreads();
  if (threadIdx.x == 0) out[row] = red[0] + red[1] + red[2] + red[3];
}
template <bool MASK>
__global__ void k_loglik_rowsum_bwd(const float* __restrict__ X, const float* __restrict__ z, const float* __restrict__ grow,
                                    float* __restrict__ gz, size_t n, size_t inner, size_t nX, const int* __restrict__ n_obs, int T,
                                    size_t frame) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    if constexpr (MASK) {
      const size_t ex = e % nX;
      if (ex % inner >= obs_limit(n_obs, ex / inner, T, frame)) { gz[e] = 0.f; continue; }   // padded: X and z are not read
    }
    const float xv = X[e % nX], zv = z[e];
    gz[e] = grow[e / inner] * (xv / zv - (1.f - xv) / (1.f - zv));
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
int loglik_fwd(const float* X, const float* z, float* ll, size_t n, size_t nX, hipStream_t st) {
  hipLaunchKernelGGL(k_loglik_fwd, ew_grid(n), 256, 0, st, X, z, ll, n, nX);
  return check_launch("loglik_fwd");
}
int loglik_bwd(const float* X, const float* z, const float* g, float* gz, size_t n, size_t nX, hipStream_t st) {
  hipLaunchKernelGGL(k_loglik_bwd, ew_grid(n), 256, 0, st, X, z, g, gz, n, nX);
  return check_launch("loglik_bwd");
}
// what every launcher that takes frame counts refuses, with nothing written: rows of T frames of `frame` elements, X a whole number of them
static const char* len_refusal(size_t inner, size_t nX, const FrameMask& m) {
  if (m.n_obs == nullptr) return "n_obs is NULL";
  if (m.T < 1 || m.frame < 1 || inner != (size_t)m.T * m.frame) return "inner must be T * frame";
  if (nX < inner || nX % inner != 0) return "X must hold a whole number of sequences (nX a multiple of inner)";
  return nullptr;
}
int loglik_rowsum_fwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, float* out, hipStream_t st) {
  if (!ragged) {
    hipLaunchKernelGGL(k_loglik_rowsum<false>, (unsigned)r.rows, 256, 0, st, r.X, r.z, out, r.inner, r.nX, (const int*)nullptr, 0, (size_t)0);
    return check_launch("loglik_rowsum");
  }
  if (const char* why = len_refusal(r.inner, r.nX, m)) return set_error("%s: %s", who, why);
  if (r.rows == 0 || (r.rows * r.inner) % r.nX != 0) return set_error("%s: X must tile the rows", who);
  hipLaunchKernelGGL(k_loglik_rowsum<true>, (unsigned)r.rows, 256, 0, st, r.X, r.z, out, r.inner, r.nX, m.n_obs, m.T, m.frame);
  return check_launch("loglik_rowsum_len");
}
int loglik_rowsum_bwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, const float* grow, float* gz, hipStream_t st) {
  const size_t n = r.rows * r.inner;
  if (!ragged) {
    hipLaunchKernelGGL(k_loglik_rowsum_bwd<false>, ew_grid(n), 256, 0, st, r.X, r.z, grow, gz, n, r.inner, r.nX, (const int*)nullptr, 0, (size_t)0);
    return check_launch("loglik_rowsum_bwd");
  }
  if (const char* why = len_refusal(r.inner, r.nX, m)) return set_error("%s: %s", who, why);
  if (r.rows == 0 || (r.rows * r.inner) % r.nX != 0) return set_error("%s: X must tile the rows", who);
  hipLaunchKernelGGL(k_loglik_rowsum_bwd<true>, ew_grid(n), 256, 0, st, r.X, r.z, grow, gz, n, r.inner, r.nX, m.n_obs, m.T, m.frame);
  return check_launch("loglik_rowsum_bwd_len");
}

// ---------------------------------------------------------------------------------------------
// ELBO glue on (N, q)-sized tensors, one launch each instead of ~10 elementwise launches apiece:
//   reparameterisation  z = mu + exp(logvar / 2) eps                                   (vae.py:75-78)
//   KL(N(mu, sigma) || N(0, 1)) summed over the latent dimension, per sample          (create_model.py:47-49 via
//       torch.distributions: 0.5 (sigma^2 + mu^2 - 1 - log sigma^2), sigma = exp(logvar / 2))
//   loss = -(mean(lhood) n - mean(kl) n - kl_u), with the three logged terms           (create_model.py:61-73)
// ---------------------------------------------------------------------------------------------
// mu / logvar: (N, q) with row stride ld (ld = q: separate tensors; ld = 2q: the two halves of the encoder's fc output);
// gradients go to gmu / glogvar with row stride ldg
__global__ void k_reparam_fwd(const float* __restrict__ mu, const float* __restrict__ logvar, int ld, const float* __restrict__ eps,
                              float* __restrict__ z, int N, int q) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * q) return;
  const int n = e / q, d = e % q;
  z[e] = mu[(size_t)n * ld + d] + expf(0.5f * logvar[(size_t)n * ld + d]) * eps[e];
}
// L draws of one (mu, logvar) and their importance log-weights log p(z) - log q(z | x) (evaluate.predict_marginal).  One lane per
// (draw, sample) row: q <= 16 terms summed serially in the order of the latent dimension -- a fixed order, no atomics.  z is the
// expression of k_reparam_fwd, so it contracts to the same fma and gives the same bits.  Rows of z are ldz apart.
__global__ __launch_bounds__(256) void k_reparam_draws_fwd(const float* __restrict__ mu, const float* __restrict__ logvar, int ld,
                                                            const float* __restrict__ eps, float* __restrict__ z, int ldz,
                                                            float* __restrict__ lw, int accumulate, int rows, int N, int q) {
  const int r = blockIdx.x * 256 + threadIdx.x;      // r = l N + n
  if (r >= rows) return;
  const int n = r % N;
  const float* m = mu + (size_t)n * ld;
  const float* lv = logvar + (size_t)n * ld;
  const float* e = eps + (size_t)r * q;
  float* zr = z + (size_t)r * ldz;
  float acc = 0.f;
  for (int d = 0; d < q; ++d) {
    const float ed = e[d], lvd = lv[d];
    const float zd = m[d] + expf(0.5f * lvd) * ed;
    zr[d] = zd;
    acc += 0.5f * (ed * ed) - 0.5f * (zd * zd) + 0.5f * lvd;
  }
  lw[r] = accumulate ? lw[r] + acc : acc;
}
// The adjoint of k_reparam_draws_fwd (training on the importance-weighted bound): gz (K,N,.) with row stride ldgz, glw (K,N), either
// may be NULL (zero).  With sigma = exp(logvar / 2), z = mu + sigma eps:  d z / d mu = 1, d z / d logvar = sigma eps / 2,
// d lw / d mu = -z, d lw / d logvar = 1/2 - z sigma eps / 2.  One lane per (n, i) sums the draws k = 0 .. K-1 in that order: a fixed
// order, no atomics.
__global__ __launch_bounds__(256) void k_reparam_draws_bwd(const float* __restrict__ gz, int ldgz, const float* __restrict__ glw,
                                                            const float* __restrict__ mu, const float* __restrict__ logvar, int ld,
                                                            const float* __restrict__ eps, float* __restrict__ gmu,
                                                            float* __restrict__ glogvar, int ldg, int K, int N, int q) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N * q) return;
  const int n = e / q, d = e % q;
  const float m = mu[(size_t)n * ld + d], sg = expf(0.5f * logvar[(size_t)n * ld + d]);
  float am = 0.f, al = 0.f;
  for (int k = 0; k < K; ++k) {
    const size_t r = (size_t)k * N + n;
    const float g = gz ? gz[r * ldgz + d] : 0.f, gl = glw ? glw[r] : 0.f;
    const float se = sg * eps[r * q + d];
    const float zd = m + se;
    am += g - gl * zd;
    al += g * (0.5f * se) + gl * (0.5f - zd * (0.5f * se));
  }
  gmu[(size_t)n * ldg + d] = am;
  glogvar[(size_t)n * ldg + d] = al;
}
__global__ void k_reparam_bwd(const float* __restrict__ gz, const float* __restrict__ logvar, int ld, const float* __restrict__ eps,
                              float* __restrict__ gmu, float* __restrict__ glogvar, int ldg, int N, int q) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * q) return;
  const int n = e / q, d = e % q;
  const float g = gz[e];
  gmu[(size_t)n * ldg + d] = g;
  glogvar[(size_t)n * ldg + d] = g * eps[e] * (0.5f * expf(0.5f * logvar[(size_t)n * ld + d]));
}
// z = mu + exp(logvar / 2) eps AND the workgroup's share of sum_{n,d} KL(N(mu, sigma) || N(0, 1)): klpart[blockIdx.x] (summed by the ELBO
// kernel, so the KL term needs no pass of its own over (mu, logvar)); backward: the two gradients of (mu, logvar) -- through z and through the
// KL sum (gkl: the same value for every term) -- in one write, instead of two tensors that autograd then adds
__global__ __launch_bounds__(256) void k_reparam_kl_fwd(const float* __restrict__ mu, const float* __restrict__ logvar, int ld,
                                                         const float* __restrict__ eps, float* __restrict__ z, float* __restrict__ klpart, int N,
                                                         int q) {
  __shared__ float red[4];
  const int e = blockIdx.x * 256 + threadIdx.x;
  float kl = 0.f;
  if (e < N * q) {
    const int n = e / q, d = e % q;
    const float m = mu[(size_t)n * ld + d], sg = expf(0.5f * logvar[(size_t)n * ld + d]);
    z[e] = m + sg * eps[e];
    const float vr = sg * sg;
    kl = 0.5f * (vr + m * m - 1.f - logf(vr));
  }
  const float in1[1] = {kl};
  float out1[1];
  wave_sum_multi<1>(in1, out1);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = out1[0];
  __syncthreads();
  if (threadIdx.x == 0) klpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void k_reparam_kl_bwd(const float* __restrict__ gz, const float* __restrict__ gklpart, const float* __restrict__ mu,
                                 const float* __restrict__ logvar, int ld, const float* __restrict__ eps, float* __restrict__ gmu,
                                 float* __restrict__ glogvar, int ldg, int N, int q) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * q) return;
  const int n = e / q, d = e % q;
  const float g = gz ? gz[e] : 0.f, gk = gklpart ? gklpart[blockIdx.x] : 0.f;
  const float m = mu[(size_t)n * ld + d], lv = logvar[(size_t)n * ld + d];
  gmu[(size_t)n * ldg + d] = g + gk * m;
  glogvar[(size_t)n * ldg + d] = g * eps[e] * (0.5f * expf(0.5f * lv)) + gk * 0.5f * (expf(lv) - 1.f);
}
// one thread per sample
__global__ void k_normal_kl_fwd(const float* __restrict__ mu, const float* __restrict__ logvar, int ld, float* __restrict__ klrow, int N,
                                int q) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int d = 0; d < q; ++d) {
    const float m = mu[(size_t)n * ld + d], sg = expf(0.5f * logvar[(size_t)n * ld + d]);
    const float vr = sg * sg;                        // var_ratio = (sigma_q / sigma_p)^2, t1 = mu^2 (torch/distributions/kl.py _kl_normal_normal)
    acc += 0.5f * (vr + m * m - 1.f - logf(vr));
  }
  klrow[n] = acc;
}
__global__ void k_normal_kl_bwd(const float* __restrict__ grow, const float* __restrict__ mu, const float* __restrict__ logvar, int ld,
                                float* __restrict__ gmu, float* __restrict__ glogvar, int ldg, int N, int q) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * q) return;
  const int n = e / q, d = e % q;
  const float g = grow[n];
  gmu[(size_t)n * ldg + d] = g * mu[(size_t)n * ld + d];
  glogvar[(size_t)n * ldg + d] = g * 0.5f * (expf(logvar[(size_t)n * ld + d]) - 1.f);
}
// out[0..3] = {loss, -mean lhood, mean kl, kl_u}; one workgroup
__global__ __launch_bounds__(256) void k_elbo_fwd(const float* __restrict__ lhood, int nl, const float* __restrict__ klrow, int nk,
                                                   const float* __restrict__ kl_u, float nobs, float* __restrict__ out) {
  __shared__ float red[4][2];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nl; i += 256) a += lhood[i];
  for (int i = threadIdx.x; i < nk; i += 256) b += klrow[i];
  const float in2[2] = {a, b};
  float out2[2];
  wave_sum_multi<2>(in2, out2);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = out2[0]; red[threadIdx.x >> 6][1] = out2[1]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float lh = ((red[0][0] + red[1][0]) + (red[2][0] + red[3][0])) / (float)nl;
    const float kr = ((red[0][1] + red[1][1]) + (red[2][1] + red[3][1])) / (float)nk;
    const float ku = kl_u[0];
    out[0] = -(lh * nobs - kr * nobs - ku);
    out[1] = -lh;
    out[2] = kr;
    out[3] = ku;
  }
}
// gout[0..3]: gradients w.r.t. the four outputs -> gradients of the likelihood rows, the KL rows and kl_u
__global__ void k_elbo_bwd(const float* __restrict__ gout, int nl, int nk, float nobs, float* __restrict__ glhood,
                           float* __restrict__ gklrow, float* __restrict__ gklu) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const float g0 = gout[0];
  const float gl = (-g0 * nobs - gout[1]) / (float)nl;
  const float gk = (g0 * nobs + gout[2]) / (float)nk;
  if (e < nl) glhood[e] = gl;
  if (e < nk) gklrow[e] = gk;
  if (e == 0) gklu[0] = g0 + gout[3];
}

// ---- the decoder's output activation fused with the likelihood, and the ELBO assembled in one launch -------------------
// z = sigmoid(a) (vae.py:84, nn.Sigmoid) and sum over a row slice of log(z) X + log(1 - z)(1 - X) (vae.py:136-153 summed as
// create_model.py:49 does): grid (nsplit, rows); part[row][split].  Same expressions as k_act_fwd / k_loglik_rowsum, so z and
// every term are bit-identical to the separate kernels; only the order of the row sum differs.
// MASK (gpode_sigmoid_loglik_fwd_len): z is written for every element as ever, the sum takes the observed terms only (obs_limit above):
// a select, so what a padded target or logit holds reaches nothing, and the padded targets are not loaded.  With full lengths part has
// the unmasked kernel's bits, which takes two things.  (1) The 16-byte path keeps its element-to-thread assignment, and so the order of
// the sum, whatever the frame size; its float4 LOADS are used only where a float4 cannot straddle two frames (frame % 4 == 0), otherwise
// the four elements are loaded one by one.  (2) The roundings of a term are spelt out as the compiler contracts them in the unmasked
// kernel (-ffp-contract=fast): fma(log z, x, log(1 - z) (1 - x)) on the 16-byte path, two products and a sum on the scalar path;
// tests/test_gpu_ragged_loss.py (full lengths) holds the two kernels together.  A slice boundary inside a frame and a mask boundary
// inside a slice need nothing special.  <false> is the kernel as it was (n_obs, T, frame are not read).
template <bool MASK>
__global__ __launch_bounds__(256) void k_sigmoid_loglik_fwd(const float* __restrict__ X, const float* __restrict__ a, float* __restrict__ z,
                                                             float* __restrict__ part, size_t inner, size_t nX, size_t chunk,
                                                             const int* __restrict__ n_obs, int T, size_t frame) {
  __shared__ float red[4];
  const size_t row = blockIdx.y, p0 = (size_t)blockIdx.x * chunk, p1 = p0 + chunk < inner ? p0 + chunk : inner;
  float acc = 0.f;
  if constexpr (!MASK) {
    auto one = [&](float av, float xv) {
      const float zv = 1.f / (1.f + expf(-av));
      acc += logf(zv) * xv + logf(1.f - zv) * (1.f - xv);
      return zv;
    };
    if (((inner | nX | chunk) & 3) == 0) {           // rows, wraps of X and slices all start on 16-byte boundaries
      for (size_t p = p0 + 4 * threadIdx.x; p < p1; p += 1024) {
        const size_t e = row * inner + p;
        const float4 av = *reinterpret_cast<const float4*>(a + e), xv = *reinterpret_cast<const float4*>(X + e % nX);
        float4 zv;
        zv.x = one(av.x, xv.x); zv.y = one(av.y, xv.y); zv.z = one(av.z, xv.z); zv.w = one(av.w, xv.w);
        *reinterpret_cast<float4*>(z + e) = zv;
      }
    } else {
      for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const size_t e = row * inner + p;
        z[e] = one(a[e], X[e % nX]);
      }
    }
  } else {
    const size_t lim = obs_limit(n_obs, row % (nX / inner), T, frame);
    if (((inner | nX | chunk) & 3) == 0) {
      auto one = [&](float av, float xv, bool obs) {
        const float zv = 1.f / (1.f + expf(-av));
        const float t = __fmaf_rn(logf(zv), xv, __fmul_rn(logf(1.f - zv), 1.f - xv));
        acc = obs ? __fadd_rn(acc, t) : acc;
        return zv;
      };
      const bool whole = (frame & 3) == 0;           // a float4 lies in one frame: observed or padded as a whole
      for (size_t p = p0 + 4 * threadIdx.x; p < p1; p += 1024) {
        const size_t e = row * inner + p;
        const float* xp = X + e % nX;
        float4 av, xv = {0.f, 0.f, 0.f, 0.f}, zv;
        if (whole) {
          av = *reinterpret_cast<const float4*>(a + e);
          if (p < lim) xv = *reinterpret_cast<const float4*>(xp);
        } else {
          av = float4{a[e], a[e + 1], a[e + 2], a[e + 3]};
          if (p + 0 < lim) xv.x = xp[0];
          if (p + 1 < lim) xv.y = xp[1];
          if (p + 2 < lim) xv.z = xp[2];
          if (p + 3 < lim) xv.w = xp[3];
        }
        zv.x = one(av.x, xv.x, p + 0 < lim); zv.y = one(av.y, xv.y, p + 1 < lim);
        zv.z = one(av.z, xv.z, p + 2 < lim); zv.w = one(av.w, xv.w, p + 3 < lim);
        *reinterpret_cast<float4*>(z + e) = zv;
      }
    } else {
      for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const size_t e = row * inner + p;
        const bool obs = p < lim;
        const float xv = obs ? X[e % nX] : 0.f;
        const float zv = 1.f / (1.f + expf(-a[e]));
        const float t = __fadd_rn(__fmul_rn(logf(zv), xv), __fmul_rn(logf(1.f - zv), 1.f - xv));
        acc = obs ? __fadd_rn(acc, t) : acc;
        z[e] = zv;
      }
    }
  }
  float in1[1] = {acc}, out1[1];
  wave_sum_multi<1>(in1, out1);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = out1[0];
  __syncthreads();
  if (threadIdx.x == 0) part[row * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// ga = d/da: k_loglik_rowsum_bwd followed by k_act_bwd (sigmoid), same expressions in the same order
// MASK: ga = 0 on padded elements, whose X and z are not read (<false> is the kernel as it was)
template <bool MASK>
__global__ void k_sigmoid_loglik_bwd(const float* __restrict__ X, const float* __restrict__ z, const float* __restrict__ grow,
                                     float* __restrict__ ga, size_t n, size_t inner, size_t nX, const int* __restrict__ n_obs, int T,
                                     size_t frame) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    if constexpr (MASK) {
      const size_t ex = e % nX;
      if (ex % inner >= obs_limit(n_obs, ex / inner, T, frame)) { ga[e] = 0.f; continue; }
    }
    const float xv = X[e % nX], zv = z[e];
    const float gz = grow[e / inner] * (xv / zv - (1.f - xv) / (1.f - zv));
    ga[e] = gz * zv * (1.f - zv);
  }
}

// out[0..3] = {loss, -mean lhood, mean kl, kl_u} (create_model.py:61-73) from the likelihood partial sums (nl_values of them over
// nl_rows rows), the encoder's packed (mu | logvar) rows hs (and hv for second-order models; KL of a factorised Gaussian is additive)
// and the inducing posterior (Um, packed Us: svpy.py:144-175, k_svgp_kl in gp_misc.hip).  ONE workgroup, fixed-order reductions.
// sum of squares of a long vector in kElboParts fixed slices (the packed Us of a big inducing set: 2.1 M entries at M = 512, D = 16
// took one workgroup 0.87 ms)
constexpr int kElboParts = 256;
__global__ __launch_bounds__(256) void k_sumsq_parts(const float* __restrict__ v, size_t n, float* __restrict__ part) {
  __shared__ float red[4];
  const size_t chunk = (n + kElboParts - 1) / kElboParts, e0 = blockIdx.x * chunk, e1 = e0 + chunk < n ? e0 + chunk : n;
  float acc = 0.f;
  for (size_t e = e0 + threadIdx.x; e < e1; e += 256) acc = fmaf(v[e], v[e], acc);
  float in1[1] = {acc}, out1[1];
  wave_sum_multi<1>(in1, out1);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = out1[0];
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(1024) void k_elbo_all_fwd(const float* __restrict__ lpart, int nl_rows, int nl_values, const float* __restrict__ hs,
                                                        const float* __restrict__ hv, int N, int q, int M, int Do,
                                                        const float* __restrict__ Um, const float* __restrict__ Us, float nobs,
                                                        float* __restrict__ out, const float* __restrict__ usq_part,
                                                        const float* __restrict__ kls = nullptr, int nks = 0,
                                                        const float* __restrict__ klv = nullptr, int nkv = 0) {
  __shared__ float red[16][3];
  const size_t P = (size_t)M * (M + 1) / 2;
  float u = 0.f, a = 0.f, b = 0.f;
  // one workgroup walks 30 000 + 16 000 values: eight independent loads per thread in flight instead of one per dependent add
  auto strided = [&](const float* __restrict__ p, size_t n, bool square) {
    const size_t bd = blockDim.x;
    float sacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    size_t e = threadIdx.x;
    for (; e + 7 * bd < n; e += 8 * bd) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[e + k * bd];
#pragma unroll
      for (int k = 0; k < 8; ++k) sacc[k] = square ? fmaf(v[k], v[k], sacc[k]) : sacc[k] + v[k];
    }
    for (; e < n; e += bd) sacc[0] = square ? fmaf(p[e], p[e], sacc[0]) : sacc[0] + p[e];
    return ((sacc[0] + sacc[1]) + (sacc[2] + sacc[3])) + ((sacc[4] + sacc[5]) + (sacc[6] + sacc[7]));
  };
  if (usq_part) {                                    // ||Us||_F^2 arrives as kElboParts partial sums
    for (int e = threadIdx.x; e < kElboParts; e += blockDim.x) u += usq_part[e];
  } else {
    u = strided(Us, P * Do, true);
  }
  for (int e = threadIdx.x; e < M * Do; e += blockDim.x) {
    const int m = e / Do, d = e % Do;
    const float l = Us[(size_t)d * P + (size_t)m * (m + 1) / 2 + m];
    const float v = Um[e];
    u += v * v - logf(l * l);
  }
  a = strided(lpart, (size_t)nl_values, false);
  // hs == nullptr: the KL terms arrive summed per workgroup of k_reparam_kl_fwd (kls / klv)
  if (nks > 0) b += strided(kls, (size_t)nks, false);
  if (nkv > 0) b += strided(klv, (size_t)nkv, false);
  for (int e = threadIdx.x; hs && e < N * q; e += blockDim.x) {
    const int n = e / q, d = e % q;
    {
      const float m = hs[(size_t)n * 2 * q + d], sg = expf(0.5f * hs[(size_t)n * 2 * q + q + d]);
      const float vr = sg * sg;
      b += 0.5f * (vr + m * m - 1.f - logf(vr));
    }
    if (hv) {
      const float m = hv[(size_t)n * 2 * q + d], sg = expf(0.5f * hv[(size_t)n * 2 * q + q + d]);
      const float vr = sg * sg;
      b += 0.5f * (vr + m * m - 1.f - logf(vr));
    }
  }
  const float in3[3] = {u, a, b};
  float out3[3];
  wave_sum_multi<3>(in3, out3);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = out3[0]; red[threadIdx.x >> 6][1] = out3[1]; red[threadIdx.x >> 6][2] = out3[2]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[3] = {0.f, 0.f, 0.f};
    for (int w = 0; w < 16; ++w) { t[0] += red[w][0]; t[1] += red[w][1]; t[2] += red[w][2]; }
    const float ku = 0.5f * (t[0] - (float)M * (float)Do);
    const float lh = t[1] / (float)nl_rows, kr = t[2] / (float)N;
    out[0] = -(lh * nobs - kr * nobs - ku);
    out[1] = -lh;
    out[2] = kr;
    out[3] = ku;
  }
}
// g0..g3: gradients w.r.t. the four outputs (device scalars, NULL = 0) -> likelihood rows, packed encoder rows, Um, Us
__global__ void k_elbo_all_bwd(const float* __restrict__ g0p, const float* __restrict__ g1p, const float* __restrict__ g2p,
                               const float* __restrict__ g3p, int nl_rows, const float* __restrict__ hs, const float* __restrict__ hv, int N,
                               int q, int M, int Do, const float* __restrict__ Um, const float* __restrict__ Us, float nobs,
                               float* __restrict__ glrow, float* __restrict__ ghs, float* __restrict__ ghv, float* __restrict__ dUm,
                               float* __restrict__ dUs) {
  const size_t P = (size_t)M * (M + 1) / 2;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float g0 = g0p ? *g0p : 0.f, g1 = g1p ? *g1p : 0.f, g2 = g2p ? *g2p : 0.f, g3 = g3p ? *g3p : 0.f;
  if (e < (size_t)nl_rows) glrow[e] = (-g0 * nobs - g1) / (float)nl_rows;
  if (e < (size_t)N * q) {
    const float gk = (g0 * nobs + g2) / (float)N;
    const int n = (int)(e / q), d = (int)(e % q);
    const size_t im = (size_t)n * 2 * q + d, il = im + q;
    ghs[im] = gk * hs[im];
    ghs[il] = gk * 0.5f * (expf(hs[il]) - 1.f);
    if (hv) {
      ghv[im] = gk * hv[im];
      ghv[il] = gk * 0.5f * (expf(hv[il]) - 1.f);
    }
  }
  const float g = g0 + g3;
  if (e < (size_t)M * Do) dUm[e] = g * Um[e];
  if (e < P * Do) {
    const size_t k = e % P;
    int n = (int)((sqrtf(8.f * (float)k + 1.f) - 1.f) * 0.5f);
    while ((size_t)(n + 1) * (n + 2) / 2 <= k) ++n;
    while ((size_t)n * (n + 1) / 2 > k) --n;
    const bool diag = (k - (size_t)n * (n + 1) / 2) == (size_t)n;
    const float v = Us[e];
    dUs[e] = g * (diag ? v - 1.f / v : v);
  }
}

// k_elbo_all_bwd and k_sigmoid_loglik_bwd in ONE launch: every likelihood row receives the same gradient (-g0 nobs - g1) / rows, so the
// logit gradients need no row-gradient tensor in between -- blocks [0, nb_small) do the (N,q)- and (M,D)-sized outputs, the rest the logits.
// MASK (the *_len entry points): ga = 0 on padded elements, whose X and z are not read; everything else is untouched, and <false>
// is the kernel as it was (inner, n_obs, T, frame are not read).
template <bool MASK>
__global__ void k_elbo_loglik_bwd(const float* __restrict__ g0p, const float* __restrict__ g1p, const float* __restrict__ g2p,
                                  const float* __restrict__ g3p, int nl_rows, const float* __restrict__ hs, const float* __restrict__ hv, int N,
                                  int q, int M, int Do, const float* __restrict__ Um, const float* __restrict__ Us, float nobs,
                                  float* __restrict__ glrow, float* __restrict__ ghs, float* __restrict__ ghv, float* __restrict__ dUm,
                                  float* __restrict__ dUs, int nb_small, const float* __restrict__ X, const float* __restrict__ z,
                                  float* __restrict__ ga, size_t n, size_t nX, float* __restrict__ gkls, int nks,
                                  float* __restrict__ gklv, int nkv, size_t inner, const int* __restrict__ n_obs, int T, size_t frame) {
  const float g0 = g0p ? *g0p : 0.f, g1 = g1p ? *g1p : 0.f, g2 = g2p ? *g2p : 0.f, g3 = g3p ? *g3p : 0.f;
  if ((int)blockIdx.x < nb_small) {
    const size_t P = (size_t)M * (M + 1) / 2;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)nl_rows) glrow[e] = (-g0 * nobs - g1) / (float)nl_rows;
    if (e < (size_t)nks) gkls[e] = (g0 * nobs + g2) / (float)N;         // hs == nullptr: d loss / d (KL partial sum), the same for all
    if (e < (size_t)nkv) gklv[e] = (g0 * nobs + g2) / (float)N;
    if (hs && e < (size_t)N * q) {
      const float gk = (g0 * nobs + g2) / (float)N;
      const int nn = (int)(e / q), d = (int)(e % q);
      const size_t im = (size_t)nn * 2 * q + d, il = im + q;
      ghs[im] = gk * hs[im];
      ghs[il] = gk * 0.5f * (expf(hs[il]) - 1.f);
      if (hv) {
        ghv[im] = gk * hv[im];
        ghv[il] = gk * 0.5f * (expf(hv[il]) - 1.f);
      }
    }
    const float g = g0 + g3;
    if (e < (size_t)M * Do) dUm[e] = g * Um[e];
    if (e < P * Do) {
      const size_t k = e % P;
      int r = (int)((sqrtf(8.f * (float)k + 1.f) - 1.f) * 0.5f);
      while ((size_t)(r + 1) * (r + 2) / 2 <= k) ++r;
      while ((size_t)r * (r + 1) / 2 > k) --r;
      const bool diag = (k - (size_t)r * (r + 1) / 2) == (size_t)r;
      const float v = Us[e];
      dUs[e] = g * (diag ? v - 1.f / v : v);
    }
    return;
  }
  const float gl = (-g0 * nobs - g1) / (float)nl_rows;
  const size_t nb = gridDim.x - nb_small;
  for (size_t e = ((size_t)blockIdx.x - nb_small) * blockDim.x + threadIdx.x; e < n; e += nb * blockDim.x) {
    if constexpr (MASK) {
      const size_t ex = e % nX;
      if (ex % inner >= obs_limit(n_obs, ex / inner, T, frame)) { ga[e] = 0.f; continue; }
    }
    const float xv = X[e % nX], zv = z[e];
    const float gz = gl * (xv / zv - (1.f - xv) / (1.f - zv));
    ga[e] = gz * zv * (1.f - zv);
  }
}

// ---- the importance-weighted bound: K initial-state draws per sequence, shared by the L function draws ---------------------------------
// Rows of the likelihood are ordered (l, k, n) -- X is broadcast by row % N -- and lw (K,N) = log p(z0) - log q(z0 | x) comes from
// k_reparam_draws_fwd.  a[l,k,n] = sum_s lpart[row][s] + lw[k,n];  iw[l,n] = logsumexp_k a - log K;  the weighting is over z0 only, the
// mean over the function draws stays outside the log.  One wavefront owns a group (l, n), lane k its draw (K <= 64): the maximum over
// the draws is subtracted before any exp (a group's a spans thousands of nats), so the largest weight is exactly 1 and a weight that
// underflows is exactly 0.  Fixed summation orders, no atomics.
__device__ __forceinline__ float wave_max64(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}
// lane k of the calling wavefront -> w = exp(a - max_k a) (0 on lanes >= K), wave-uniform top = max_k a, s1 = sum_k w, s2 = sum_k w^2.
// Every caller goes through this one function, so the weights of the forward, of both backward forms and of the logit blocks agree bit
// for bit.
__device__ __forceinline__ void iw_group(const float* __restrict__ lpart, int nsplit, const float* __restrict__ lw, int K, int N, int l,
                                         int n, float& a, float& top, float& w, float& s1, float& s2) {
  const int lane = threadIdx.x & 63;
  a = -INFINITY;
  if (lane < K) {
    const float* p = lpart + ((size_t)((size_t)l * K + lane) * N + n) * nsplit;
    float acc = 0.f;
    for (int s = 0; s < nsplit; ++s) acc = __fadd_rn(acc, p[s]);
    a = __fadd_rn(acc, lw[(size_t)lane * N + n]);
  }
  top = wave_max64(a);
  w = lane < K ? expf(__fsub_rn(a, top)) : 0.f;
  const float in2[2] = {w, __fmul_rn(w, w)};
  float out2[2];
  wave_sum_multi<2>(in2, out2);
  s1 = out2[0];
  s2 = out2[1];
}
// the gradient every likelihood row's softmax weight is scaled by: d loss / d iw[l,n] = (-g0 nobs - g1) / (L N)
__device__ __forceinline__ float iw_row_scale(const float* g0p, const float* g1p, float nobs, int L, int N) {
  const float g0 = g0p ? *g0p : 0.f, g1 = g1p ? *g1p : 0.f;
  return __fdiv_rn(__fmaf_rn(-g0, nobs, -g1), (float)((size_t)L * N));
}
// out[0..4] = {loss = -(nobs mean iw - kl_u), -mean iw, -mean lw (the Monte-Carlo KL(q(z0) || p), for the log line), kl_u, mean ess},
// ess[l,n] = (sum_k w)^2 / sum_k w^2.  ONE workgroup of 16 wavefronts: wavefront v takes the groups v, v + 16, ... in that order, lane 0
// of every wavefront leaves its sums, thread 0 adds the 16 in order.  KL(q(u) || p(u)) as in k_elbo_all_fwd.
__global__ __launch_bounds__(1024) void k_elbo_iw_fwd(const float* __restrict__ lpart, int nsplit, const float* __restrict__ lw, int L, int K,
                                                       int N, int M, int Do, const float* __restrict__ Um, const float* __restrict__ Us,
                                                       float nobs, float* __restrict__ out, const float* __restrict__ usq_part) {
  __shared__ float red[16][4];
  const size_t P = (size_t)M * (M + 1) / 2;
  const int wv = threadIdx.x >> 6;
  float u = 0.f, b = 0.f;
  if (usq_part) {
    for (int e = threadIdx.x; e < kElboParts; e += blockDim.x) u += usq_part[e];
  } else {
    for (size_t e = threadIdx.x; e < P * Do; e += blockDim.x) u = fmaf(Us[e], Us[e], u);
  }
  for (int e = threadIdx.x; e < M * Do; e += blockDim.x) {
    const int m = e / Do, d = e % Do;
    const float l = Us[(size_t)d * P + (size_t)m * (m + 1) / 2 + m];
    const float v = Um[e];
    u += v * v - logf(l * l);
  }
  for (int e = threadIdx.x; e < K * N; e += blockDim.x) b += lw[e];
  const float in2[2] = {u, b};
  float out2[2];
  wave_sum_multi<2>(in2, out2);
  float siw = 0.f, sess = 0.f;
  const float logK = logf((float)K);
  for (int g = wv; g < L * N; g += 16) {
    float a, top, w, s1, s2;
    iw_group(lpart, nsplit, lw, K, N, g / N, g % N, a, top, w, s1, s2);
    siw += top + logf(s1) - logK;
    sess += s1 * s1 / s2;
  }
  if ((threadIdx.x & 63) == 0) { red[wv][0] = out2[0]; red[wv][1] = out2[1]; red[wv][2] = siw; red[wv][3] = sess; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < 16; ++v) { t[0] += red[v][0]; t[1] += red[v][1]; t[2] += red[v][2]; t[3] += red[v][3]; }
    const float ku = 0.5f * (t[0] - (float)M * (float)Do);
    const float groups = (float)((size_t)L * N), iw = t[2] / groups;
    out[0] = -(iw * nobs - ku);
    out[1] = -iw;
    out[2] = -(t[1] / (float)((size_t)K * N));
    out[3] = ku;
    out[4] = t[3] / groups;
  }
}
// g0..g4: gradients w.r.t. the five outputs (device scalars, NULL = 0; the ess output is a diagnostic and carries NO gradient: g4 is
// accepted and not read) -> grow[row] = softmax_k(a)[l,k,n] (-g0 nobs - g1) / (L N), glw[k,n] = sum_l grow[(l,k,n)] - g2 / (K N),
// dUm, dUs as in k_elbo_all_bwd.  Blocks [0, nb_small): wavefront n' takes sequence n' and walks l = 0 .. L-1 in order (lane k sums its
// glw in a register); the same threads do the elementwise (M,Do)- and packed-Us-sized outputs.
// LL (gpode_elbo_iw_bwd_ll): the blocks behind them do the logits, block (row, c) the elements [c kIwSpan, (c+1) kIwSpan) of its row.
// Rows do NOT share one gradient here, so every wavefront of a logit block recomputes its row's weight from the K nsplit partial sums of
// its group through iw_group -- K nsplit loads (out of the L2) against up to kIwSpan / 4 elements of work per wavefront, no row-gradient
// tensor staged between blocks and so no ordering between blocks of one launch -- and ga is k_sigmoid_loglik_bwd's expression.
constexpr int kIwSpan = 2048;
template <bool LL>
__global__ __launch_bounds__(256) void k_elbo_iw_bwd(const float* __restrict__ g0p, const float* __restrict__ g1p, const float* __restrict__ g2p,
                                                      const float* __restrict__ g3p, const float* __restrict__ lpart, int nsplit,
                                                      const float* __restrict__ lw, int L, int K, int N, int M, int Do,
                                                      const float* __restrict__ Um, const float* __restrict__ Us, float nobs,
                                                      float* __restrict__ grow, float* __restrict__ glw, float* __restrict__ dUm,
                                                      float* __restrict__ dUs, int nb_small, const float* __restrict__ X,
                                                      const float* __restrict__ z, float* __restrict__ ga, size_t inner, size_t nX, int cpr) {
  const float c = iw_row_scale(g0p, g1p, nobs, L, N);
  const int lane = threadIdx.x & 63;
  if (!LL || (int)blockIdx.x < nb_small) {
    const float g0 = g0p ? *g0p : 0.f, g2 = g2p ? *g2p : 0.f, g3 = g3p ? *g3p : 0.f;
    const size_t P = (size_t)M * (M + 1) / 2;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = e >> 6;                         // this wavefront's sequence (wave-uniform)
    if (n < (size_t)N) {
      float acc = 0.f;
      for (int l = 0; l < L; ++l) {
        float a, top, w, s1, s2;
        iw_group(lpart, nsplit, lw, K, N, l, (int)n, a, top, w, s1, s2);
        const float gr = __fmul_rn(__fdiv_rn(w, s1), c);
        if (lane < K) grow[((size_t)l * K + lane) * N + n] = gr;
        acc = __fadd_rn(acc, gr);
      }
      if (lane < K) glw[(size_t)lane * N + n] = __fsub_rn(acc, __fdiv_rn(g2, (float)((size_t)K * N)));
    }
    const float g = g0 + g3;
    if (e < (size_t)M * Do) dUm[e] = g * Um[e];
    if (e < P * Do) {
      const size_t k = e % P;
      int r = (int)((sqrtf(8.f * (float)k + 1.f) - 1.f) * 0.5f);
      while ((size_t)(r + 1) * (r + 2) / 2 <= k) ++r;
      while ((size_t)r * (r + 1) / 2 > k) --r;
      const bool diag = (k - (size_t)r * (r + 1) / 2) == (size_t)r;
      const float v = Us[e];
      dUs[e] = g * (diag ? v - 1.f / v : v);
    }
    return;
  }
  if constexpr (LL) {
    const size_t bl = (size_t)blockIdx.x - nb_small, row = bl / cpr, p0 = (bl % cpr) * (size_t)kIwSpan;
    const size_t p1 = p0 + kIwSpan < inner ? p0 + kIwSpan : inner;
    const int n = (int)(row % N), k = (int)((row / N) % K), l = (int)(row / ((size_t)N * K));
    float a, top, w, s1, s2;
    iw_group(lpart, nsplit, lw, K, N, l, n, a, top, w, s1, s2);
    const float gl = __shfl(__fmul_rn(__fdiv_rn(w, s1), c), k, 64);
    for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
      const size_t e = row * inner + p;
      const float xv = X[e % nX], zv = z[e];
      const float gz = gl * (xv / zv - (1.f - xv) / (1.f - zv));
      ga[e] = gz * zv * (1.f - zv);
    }
  }
}

int sigmoid_loglik_splits(size_t rows, size_t inner) {
  if (rows == 0 || inner == 0) return 1;             // nothing to split (and no division by rows)
  size_t ns = (1024 + rows - 1) / rows, cap = (inner + 1023) / 1024;
  if (ns > cap) ns = cap;
  if (ns > 64) ns = 64;
  return ns < 1 ? 1 : (int)ns;
}
// the slice of a row one workgroup of the forward sums: a multiple of 4 elements; an odd one sends the kernel down its scalar path
static size_t loglik_chunk(size_t inner, int nsplit, bool aligned) {
  size_t chunk = (inner + nsplit - 1) / nsplit;
  chunk = (chunk + 3) & ~(size_t)3;
  return aligned ? chunk : chunk | 1;
}
int sigmoid_loglik_fwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, const float* a, float* z, float* part,
                       int nsplit, hipStream_t st) {
  if (nsplit < 1 || r.rows > 65535) return set_error("%s: nsplit >= 1, rows <= 65535", who);
  if (ragged) if (const char* why = len_refusal(r.inner, r.nX, m)) return set_error("%s: %s", who, why);
  if ((r.rows * r.inner) % r.nX != 0) return set_error("%s: X must tile the rows", who);
  const size_t chunk = loglik_chunk(r.inner, nsplit, aligned16(r.X, a, z));   // ragged: the kernel loads element-wise where frame % 4 != 0
  const dim3 grid(nsplit, (unsigned)r.rows);
  if (ragged) hipLaunchKernelGGL(k_sigmoid_loglik_fwd<true>, grid, 256, 0, st, r.X, a, z, part, r.inner, r.nX, chunk, m.n_obs, m.T, m.frame);
  else hipLaunchKernelGGL(k_sigmoid_loglik_fwd<false>, grid, 256, 0, st, r.X, a, z, part, r.inner, r.nX, chunk, (const int*)nullptr, 0, (size_t)0);
  return check_launch(ragged ? "sigmoid_loglik_fwd_len" : "sigmoid_loglik_fwd");
}
int sigmoid_loglik_bwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, const float* grow, float* ga, hipStream_t st) {
  const size_t n = r.rows * r.inner;
  if (!ragged) {
    hipLaunchKernelGGL(k_sigmoid_loglik_bwd<false>, ew_grid(n), 256, 0, st, r.X, r.z, grow, ga, n, r.inner, r.nX, (const int*)nullptr, 0, (size_t)0);
    return check_launch("sigmoid_loglik_bwd");
  }
  if (const char* why = len_refusal(r.inner, r.nX, m)) return set_error("%s: %s", who, why);
  if ((r.rows * r.inner) % r.nX != 0) return set_error("%s: X must tile the rows", who);
  hipLaunchKernelGGL(k_sigmoid_loglik_bwd<true>, ew_grid(n), 256, 0, st, r.X, r.z, grow, ga, n, r.inner, r.nX, m.n_obs, m.T, m.frame);
  return check_launch("sigmoid_loglik_bwd_len");
}

// ---- ragged minibatches with the padding taken out in front of the decoder (the *_pk entry points and the frame gather) -----------------
// c[n] = clamp(n_obs[n], 0, T), off = exclusive prefix sum of c (N + 1 entries, off[N] = P), src[j] = n T + t for compact image j of a
// draw: the compact batch is (L P, ...), ordered (l, n, t) -- the padded order with the padded frames removed.
// out[(l P + j), 0..q) = zt[l, src[j], 0..q): rows of 12-64 bytes at a stride of ld floats, one lane per element (launch-bound)
__global__ void k_gather_frames_fwd(const float* __restrict__ zt, int ld, int q, const int* __restrict__ src, size_t NT, int P,
                                    float* __restrict__ out, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / q, l = r / P;
    out[e] = zt[(l * NT + src[r - l * P]) * ld + (e - r * q)];
  }
}
// the adjoint as a gather over gzt (L,N,T,ld): every element is written once -- observed rows, columns < q: the element of gout;
// padded rows and columns >= q: zero.  No pre-fill, no atomics.
__global__ void k_gather_frames_bwd(const float* __restrict__ gout, int ld, int q, const int* __restrict__ off, int N, int T, int P,
                                    float* __restrict__ gzt, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / ld, s = r / T, l = s / N;
    const int col = (int)(e - r * ld), t = (int)(r - s * T), nn = (int)(s - l * N);
    const int o0 = off[nn], c = off[nn + 1] - o0;
    gzt[e] = (col < q && t < c) ? gout[(l * P + o0 + t) * q + col] : 0.f;
  }
}
int gather_frames_fwd(const float* zt, int ld, int q, const int* src, int L, int N, int T, int P, float* out, hipStream_t st) {
  const size_t n = (size_t)L * P * q;
  hipLaunchKernelGGL(k_gather_frames_fwd, ew_grid(n), 256, 0, st, zt, ld, q, src, (size_t)N * T, P, out, n);
  return check_launch("gather_frames_fwd");
}
int gather_frames_bwd(const float* gout, int ld, int q, const int* off, int L, int N, int T, int P, float* gzt, hipStream_t st) {
  const size_t n = (size_t)L * N * T * ld;
  hipLaunchKernelGGL(k_gather_frames_bwd, ew_grid(n), 256, 0, st, gout, ld, q, off, N, T, P, gzt, n);
  return check_launch("gather_frames_bwd");
}

// k_sigmoid_loglik_fwd over compact logits: row (l, n) is the c[n] frame contiguous logits at (l P + off[n]) frame, its targets the
// leading c[n] frames of X + n T frame -- a padded target is never addressed.  The slices are the twin's (chunk from inner = T frame), a
// slice beyond its row's length writes exactly 0; element-to-thread assignment and the roundings of a term are those of
// k_sigmoid_loglik_fwd<true>, so with c[n] = T for all n z and part have the twin's bits.  frame % 4 == 0 (the launcher refuses others):
// rows, frames and slices start on 16-byte boundaries when the three pointers do (chunk % 4 == 0), else chunk is odd: the scalar path.
__global__ __launch_bounds__(256) void k_sigmoid_loglik_fwd_pk(const float* __restrict__ X, const float* __restrict__ a, float* __restrict__ z,
                                                                float* __restrict__ part, const int* __restrict__ off, int N, int T,
                                                                size_t frame, size_t chunk) {
  __shared__ float red[4];
  const size_t row = blockIdx.y, l = row / N, nn = row - l * N;
  const int o0 = off[nn], c = off[nn + 1] - o0, P = off[N];
  const size_t len = (size_t)(c < 0 ? 0 : (c > T ? T : c)) * frame;
  const size_t p0 = (size_t)blockIdx.x * chunk, p1 = p0 + chunk < len ? p0 + chunk : len;
  const size_t base = (l * P + o0) * frame;
  const float* __restrict__ ar = a + base;
  const float* __restrict__ xr = X + nn * T * frame;
  float* __restrict__ zr = z + base;
  float acc = 0.f;
  if ((chunk & 3) == 0) {
    auto one = [&](float av, float xv) {
      const float zv = 1.f / (1.f + expf(-av));
      acc = __fadd_rn(acc, __fmaf_rn(logf(zv), xv, __fmul_rn(logf(1.f - zv), 1.f - xv)));
      return zv;
    };
    for (size_t p = p0 + 4 * threadIdx.x; p < p1; p += 1024) {
      const float4 av = *reinterpret_cast<const float4*>(ar + p), xv = *reinterpret_cast<const float4*>(xr + p);
      float4 zv;
      zv.x = one(av.x, xv.x); zv.y = one(av.y, xv.y); zv.z = one(av.z, xv.z); zv.w = one(av.w, xv.w);
      *reinterpret_cast<float4*>(zr + p) = zv;
    }
  } else {
    for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
      const float xv = xr[p];
      const float zv = 1.f / (1.f + expf(-ar[p]));
      acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(logf(zv), xv), __fmul_rn(logf(1.f - zv), 1.f - xv)));
      zr[p] = zv;
    }
  }
  float in1[1] = {acc}, out1[1];
  wave_sum_multi<1>(in1, out1);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = out1[0];
  __syncthreads();
  if (threadIdx.x == 0) part[row * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// ga over the compact elements, k_sigmoid_loglik_bwd's expression: element e -> image e / frame = l P + j -> src[j] = n T + t -> its target
// at src[j] frame + e % frame and the row gradient grow[l N + n].  V4: four elements of one frame per lane (frame % 4 == 0, 16-byte pointers)
template <bool V4>
__global__ void k_sigmoid_loglik_bwd_pk(const float* __restrict__ X, const float* __restrict__ z, const float* __restrict__ grow,
                                        float* __restrict__ ga, const int* __restrict__ src, size_t n, int N, int T, int P, size_t frame) {
  auto one = [](float xv, float zv, float g) {
    const float gz = g * (xv / zv - (1.f - xv) / (1.f - zv));
    return gz * zv * (1.f - zv);
  };
  constexpr size_t W = V4 ? 4 : 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / W; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = W * i, img = e / frame, l = img / P;
    const int s = src[img - l * P];
    const float g = grow[l * N + s / T];
    const float* __restrict__ xp = X + (size_t)s * frame + (e - img * frame);
    if constexpr (V4) {
      const float4 xv = *reinterpret_cast<const float4*>(xp), zv = *reinterpret_cast<const float4*>(z + e);
      float4 o;
      o.x = one(xv.x, zv.x, g); o.y = one(xv.y, zv.y, g); o.z = one(xv.z, zv.z, g); o.w = one(xv.w, zv.w, g);
      *reinterpret_cast<float4*>(ga + e) = o;
    } else {
      ga[e] = one(xp[0], z[e], g);
    }
  }
}
// what the *_pk launchers refuse, with nothing written
static const char* pk_refusal(const LogLikRows& r, const PackedFrames& pk) {
  if (pk.index == nullptr) return "the frame index is NULL";
  if (pk.T < 1 || pk.frame < 1 || (pk.frame & 3) != 0) return "T >= 1 and frame a positive multiple of 4";
  const size_t inner = (size_t)pk.T * pk.frame;
  if (r.nX < inner || r.nX % inner != 0) return "X must hold a whole number of sequences (nX a multiple of T * frame)";
  if (r.rows == 0 || r.rows % (r.nX / inner) != 0) return "rows must be a multiple of the number of sequences";
  return nullptr;
}
int sigmoid_loglik_fwd_pk(const LogLikRows& r, const PackedFrames& pk, const float* a, float* z, float* part, int nsplit, hipStream_t st) {
  if (nsplit < 1 || r.rows > 65535) return set_error("gpode_sigmoid_loglik_fwd_pk: nsplit >= 1, rows <= 65535");
  if (const char* why = pk_refusal(r, pk)) return set_error("gpode_sigmoid_loglik_fwd_pk: %s", why);
  const size_t inner = (size_t)pk.T * pk.frame;
  const size_t chunk = loglik_chunk(inner, nsplit, aligned16(r.X, a, z));   // the slices are the padded twin's
  hipLaunchKernelGGL(k_sigmoid_loglik_fwd_pk, dim3(nsplit, (unsigned)r.rows), 256, 0, st, r.X, a, z, part, pk.index, (int)(r.nX / inner), pk.T,
                     pk.frame, chunk);
  return check_launch("sigmoid_loglik_fwd_pk");
}
int sigmoid_loglik_bwd_pk(const LogLikRows& r, const PackedFrames& pk, const float* grow, float* ga, hipStream_t st) {
  if (const char* why = pk_refusal(r, pk)) return set_error("gpode_sigmoid_loglik_bwd_pk: %s", why);
  const size_t N = r.nX / ((size_t)pk.T * pk.frame);
  if (pk.P < 1 || (size_t)pk.P > N * pk.T) return set_error("gpode_sigmoid_loglik_bwd_pk: 1 <= P <= N * T");
  const size_t n = r.rows / N * pk.P * pk.frame;
  if (aligned16(r.X, r.z, ga)) {
    hipLaunchKernelGGL(k_sigmoid_loglik_bwd_pk<true>, ew_grid(n / 4), 256, 0, st, r.X, r.z, grow, ga, pk.index, n, (int)N, pk.T, pk.P, pk.frame);
  } else {
    hipLaunchKernelGGL(k_sigmoid_loglik_bwd_pk<false>, ew_grid(n), 256, 0, st, r.X, r.z, grow, ga, pk.index, n, (int)N, pk.T, pk.P, pk.frame);
  }
  return check_launch("sigmoid_loglik_bwd_pk");
}

// The latent term's form (ElboKl): heads read q, values run the kernels with q = 1 and the heads' pointers null.
static int elbo_q(const ElboShape& s, const ElboKl& kl) { return kl.hs ? s.q : 1; }
// blocks of 256 threads that cover the largest of the small operands PRESENT: Us, the rows' gradients, Um, and the heads (N, q) or the
// KL values' gradients (nks, nkv)
static int elbo_small_blocks(int nl_rows, const ElboShape& s, const ElboKl& kl) {
  size_t ns = (size_t)s.M * (s.M + 1) / 2 * s.Do;
  if ((size_t)nl_rows > ns) ns = nl_rows;
  if ((size_t)s.M * s.Do > ns) ns = (size_t)s.M * s.Do;
  if (kl.hs) { if ((size_t)s.N * s.q > ns) ns = (size_t)s.N * s.q; }
  else { if ((size_t)kl.nks > ns) ns = kl.nks; if ((size_t)kl.nkv > ns) ns = kl.nkv; }
  return (int)((ns + 255) / 256);
}
int elbo_all_fwd(const float* lpart, int nl_rows, int nl_values, const ElboShape& s, const ElboKl& kl, float* out, hipStream_t st) {
  // out: 4 results + kElboParts floats of scratch
  const size_t nus = (size_t)s.M * (s.M + 1) / 2 * s.Do;
  const float* usq = nullptr;
  if (nus > ((size_t)1 << 16)) {
    hipLaunchKernelGGL(k_sumsq_parts, kElboParts, 256, 0, st, s.Us, nus, out + 4);
    usq = out + 4;
  }
  hipLaunchKernelGGL(k_elbo_all_fwd, 1, 1024, 0, st, lpart, nl_rows, nl_values, kl.hs, kl.hv, s.N, elbo_q(s, kl), s.M, s.Do, s.Um, s.Us, s.nobs, out,
                     usq, kl.kls, kl.nks, kl.klv, kl.nkv);
  if (kl.hs) return check_launch(usq ? "elbo_all_fwd (Us in parts)" : "elbo_all_fwd");
  return check_launch(usq ? "elbo_all_fwd_kl (Us in parts)" : "elbo_all_fwd_kl");
}
int elbo_all_bwd(const ElboSeeds& g, int nl_rows, const ElboShape& s, const ElboKl& kl, const ElboGrads& o, hipStream_t st) {
  hipLaunchKernelGGL(k_elbo_all_bwd, (unsigned)elbo_small_blocks(nl_rows, s, kl), 256, 0, st, g.g0, g.g1, g.g2, g.g3, nl_rows, kl.hs, kl.hv, s.N, s.q,
                     s.M, s.Do, s.Um, s.Us, s.nobs, o.glrow, kl.ghs, kl.ghv, o.dUm, o.dUs);
  return check_launch("elbo_all_bwd");
}

// the ELBO's backward and the likelihood's over the logits in one launch: the small operands' blocks first, then the logits'
int elbo_loglik_bwd(const char* who, bool ragged, const ElboSeeds& g, int nl_rows, const ElboShape& s, const ElboKl& kl, const ElboGrads& o,
                    const ElboLogits& lg, const FrameMask& m, hipStream_t st) {
  if (ragged) if (const char* why = len_refusal((size_t)(m.T > 0 ? m.T : 0) * m.frame, lg.nX, m)) return set_error("%s: %s", who, why);
  const int nb_small = elbo_small_blocks(nl_rows, s, kl);
  const unsigned grid = (unsigned)(nb_small + ew_grid(lg.n));
  const size_t inner = ragged ? (size_t)m.T * m.frame : 0;
  auto kern = ragged ? k_elbo_loglik_bwd<true> : k_elbo_loglik_bwd<false>;
  hipLaunchKernelGGL(kern, grid, 256, 0, st, g.g0, g.g1, g.g2, g.g3, nl_rows, kl.hs, kl.hv, s.N, elbo_q(s, kl), s.M, s.Do, s.Um, s.Us, s.nobs,
                     o.glrow, kl.ghs, kl.ghv, o.dUm, o.dUs, nb_small, lg.X, lg.z, lg.ga, lg.n, lg.nX, kl.gkls, kl.nks, kl.gklv, kl.nkv, inner,
                     ragged ? m.n_obs : nullptr, ragged ? m.T : 0, ragged ? m.frame : (size_t)0);
  if (kl.hs) return check_launch(ragged ? "elbo_loglik_bwd_len" : "elbo_loglik_bwd");
  return check_launch(ragged ? "elbo_loglik_bwd_kl_len" : "elbo_loglik_bwd_kl");
}

int reparam_kl_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, float* klpart, int N, int q, hipStream_t st) {
  hipLaunchKernelGGL(k_reparam_kl_fwd, (N * q + 255) / 256, 256, 0, st, mu, logvar, ld, eps, z, klpart, N, q);
  return check_launch("reparam_kl_fwd");
}
int reparam_kl_bwd(const float* gz, const float* gklpart, const float* mu, const float* logvar, int ld, const float* eps, float* gmu,
                   float* glogvar, int ldg, int N, int q, hipStream_t st) {
  hipLaunchKernelGGL(k_reparam_kl_bwd, (N * q + 255) / 256, 256, 0, st, gz, gklpart, mu, logvar, ld, eps, gmu, glogvar, ldg, N, q);
  return check_launch("reparam_kl_bwd");
}
int reparam_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int N, int q, hipStream_t st) {
  hipLaunchKernelGGL(k_reparam_fwd, (N * q + 255) / 256, 256, 0, st, mu, logvar, ld, eps, z, N, q);
  return check_launch("reparam_fwd");
}
int reparam_draws_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int ldz, float* lw, int accumulate, int L, int N,
                      int q, hipStream_t st) {
  const int rows = L * N;
  hipLaunchKernelGGL(k_reparam_draws_fwd, (rows + 255) / 256, 256, 0, st, mu, logvar, ld, eps, z, ldz, lw, accumulate, rows, N, q);
  return check_launch("reparam_draws_fwd");
}
int reparam_draws_bwd(const float* gz, int ldgz, const float* glw, const float* mu, const float* logvar, int ld, const float* eps, float* gmu,
                      float* glogvar, int ldg, int K, int N, int q, hipStream_t st) {
  hipLaunchKernelGGL(k_reparam_draws_bwd, (N * q + 255) / 256, 256, 0, st, gz, ldgz, glw, mu, logvar, ld, eps, gmu, glogvar, ldg, K, N, q);
  return check_launch("reparam_draws_bwd");
}
// what the four importance-weighted entry points refuse alike (nullptr: fine)
static const char* iw_refusal(const IwDraws& iw, const ElboShape& s) {
  if (iw.K < 1 || iw.K > 64) return "1 <= K <= 64 (one lane of a wavefront per draw)";
  if (iw.L < 1 || s.N < 1 || s.M < 1 || s.Do < 1) return "L, N, M, Do >= 1";
  if (iw.nsplit < 1) return "nsplit >= 1";
  if (iw.rows > 65535) return "rows <= 65535 (the grid of gpode_sigmoid_loglik_fwd)";
  if ((long long)iw.rows != (long long)iw.L * iw.K * s.N) return "rows = L * K * N";
  return nullptr;
}
int elbo_iw_fwd(const IwDraws& iw, const ElboShape& s, float* out, hipStream_t st) {
  if (const char* why = iw_refusal(iw, s)) return set_error("gpode_elbo_iw_fwd: %s", why);
  // out: 5 results + kElboParts floats of scratch
  const size_t nus = (size_t)s.M * (s.M + 1) / 2 * s.Do;
  const float* usq = nullptr;
  if (nus > ((size_t)1 << 16)) {
    hipLaunchKernelGGL(k_sumsq_parts, kElboParts, 256, 0, st, s.Us, nus, out + 5);
    usq = out + 5;
  }
  hipLaunchKernelGGL(k_elbo_iw_fwd, 1, 1024, 0, st, iw.lpart, iw.nsplit, iw.lw, iw.L, iw.K, s.N, s.M, s.Do, s.Um, s.Us, s.nobs, out, usq);
  return check_launch(usq ? "elbo_iw_fwd (Us in parts)" : "elbo_iw_fwd");
}
static int iw_small_blocks(const ElboShape& s) {
  size_t ns = (size_t)s.M * (s.M + 1) / 2 * s.Do;
  if ((size_t)s.N * 64 > ns) ns = (size_t)s.N * 64;      // one wavefront per sequence
  if ((size_t)s.M * s.Do > ns) ns = (size_t)s.M * s.Do;
  return (int)((ns + 255) / 256);
}
int elbo_iw_bwd(const char* who, bool ll, const ElboSeeds& g, const IwDraws& iw, const ElboShape& s, const ElboGrads& o, float* glw,
                const ElboLogits& lg, hipStream_t st) {
  if (const char* why = iw_refusal(iw, s)) return set_error("%s: %s", who, why);
  const int nb_small = iw_small_blocks(s);
  if (!ll) {
    hipLaunchKernelGGL(k_elbo_iw_bwd<false>, (unsigned)nb_small, 256, 0, st, g.g0, g.g1, g.g2, g.g3, iw.lpart, iw.nsplit, iw.lw, iw.L, iw.K, s.N, s.M,
                       s.Do, s.Um, s.Us, s.nobs, o.glrow, glw, o.dUm, o.dUs, nb_small, (const float*)nullptr, (const float*)nullptr, (float*)nullptr,
                       (size_t)0, (size_t)0, 0);
    return check_launch("elbo_iw_bwd");
  }
  const size_t n = lg.n, rows = (size_t)iw.rows;
  if (n == 0 || lg.nX == 0 || n % rows != 0 || n % lg.nX != 0) return set_error("%s: the logits must be whole rows and X must tile them", who);
  const size_t inner = n / rows, cpr = (inner + kIwSpan - 1) / kIwSpan;
  if (cpr * rows > 0x7fffffffu - 65536u) return set_error("%s: too many logits for one launch", who);
  hipLaunchKernelGGL(k_elbo_iw_bwd<true>, (unsigned)(nb_small + cpr * iw.rows), 256, 0, st, g.g0, g.g1, g.g2, g.g3, iw.lpart, iw.nsplit, iw.lw, iw.L,
                     iw.K, s.N, s.M, s.Do, s.Um, s.Us, s.nobs, o.glrow, glw, o.dUm, o.dUs, nb_small, lg.X, lg.z, lg.ga, inner, lg.nX, (int)cpr);
  return check_launch("elbo_iw_loglik_bwd");
}
int reparam_bwd(const float* gz, const float* logvar, int ld, const float* eps, float* gmu, float* glogvar, int ldg, int N, int q,
                hipStream_t st) {
  hipLaunchKernelGGL(k_reparam_bwd, (N * q + 255) / 256, 256, 0, st, gz, logvar, ld, eps, gmu, glogvar, ldg, N, q);
  return check_launch("reparam_bwd");
}
int normal_kl_fwd(const float* mu, const float* logvar, int ld, float* klrow, int N, int q, hipStream_t st) {
  hipLaunchKernelGGL(k_normal_kl_fwd, (N + 255) / 256, 256, 0, st, mu, logvar, ld, klrow, N, q);
  return check_launch("normal_kl_fwd");
}
int normal_kl_bwd(const float* grow, const float* mu, const float* logvar, int ld, float* gmu, float* glogvar, int ldg, int N, int q,
                  hipStream_t st) {
  hipLaunchKernelGGL(k_normal_kl_bwd, (N * q + 255) / 256, 256, 0, st, grow, mu, logvar, ld, gmu, glogvar, ldg, N, q);
  return check_launch("normal_kl_bwd");
}
int elbo_fwd(const float* lhood, int nl, const float* klrow, int nk, const float* kl_u, float nobs, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_elbo_fwd, 1, 256, 0, st, lhood, nl, klrow, nk, kl_u, nobs, out);
  return check_launch("elbo_fwd");
}
int elbo_bwd(const float* gout, int nl, int nk, float nobs, float* glhood, float* gklrow, float* gklu, hipStream_t st) {
  const int n = nl > nk ? nl : nk;
  hipLaunchKernelGGL(k_elbo_bwd, (n + 255) / 256, 256, 0, st, gout, nl, nk, nobs, glhood, gklrow, gklu);
  return check_launch("elbo_bwd");
}

}  // namespace gp
