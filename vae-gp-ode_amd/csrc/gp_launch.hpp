// gp_launch.hpp -- host-side helpers shared by the launchers (error slot, launch checks).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <unordered_map>

namespace gp {

char* error_slot();  // thread-local 512-byte buffer (capi.hip)
const char** last_launch_slot();  // thread-local: the tag of the launcher that ran last (capi.hip, gpode_last_launch)

inline int set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(error_slot(), 512, fmt, ap);
  va_end(ap);
  return 1;
}

inline int check_launch(const char* what) {
  *last_launch_slot() = what;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error("%s: launch failed: %s", what, hipGetErrorString(e));
  return 0;
}

// A GPODE_* switch that is on when set to "1".  Call sites keep the answer in a function-local static: read once per process.
inline bool env_flag(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '1';
}

// the float4 / b128 paths need 16-byte aligned operands; absent operands (nullptr) count as aligned
template <class... T> inline bool aligned16(const T*... p) {
  return ((uintptr_t{0} | ... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// Raise a kernel's dynamic-LDS limit above the 64 KB default.  The attribute is set once per (kernel, size) and
// remembered: hipFuncSetAttribute is not a stream operation (it is refused while the stream is being captured into
// a graph), and the first eager run of a step has already set every attribute its replay needs.
inline int set_max_lds(const void* kern, size_t bytes) {
  if (bytes <= 64 * 1024) return 0;
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> done;
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find(kern);
  if (it != done.end() && it->second >= bytes) return 0;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return set_error("hipFuncSetAttribute(max dynamic LDS=%zu): %s", bytes, hipGetErrorString(e));
  done[kern] = bytes;
  return 0;
}

// grid of an elementwise kernel with a grid-stride loop: one 256-thread block per 256 elements, at most 8192 of them
inline int ew_grid(size_t n) { size_t g = (n + 255) / 256; return (int)(g < 8192 ? (g ? g : 1) : 8192); }

// Compute units of the current device: the persistent kernels launch one (or two) workgroup(s) per CU.  Queried once (the first
// eager run of a step, never inside a capture); clamped to 256 because the split-sum scratch buffers are sized for that.
inline int num_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      return 256;
    return v < 256 ? v : 256;
  }();
  return n;
}

// Monte-Carlo draws batched into ONE launch (the reference loops `for l in range(L)` over whole flow calls, odegpvae.py:41-43):
// blockIdx.y = draw.  Strides in floats of the operands that differ per draw -- 0 = shared by all draws (the inducing locations
// handed to the prior-only rhs, the initial states z0 of a rollout).  Which operand each stride belongs to: the row operations'
// declarations below, rollout_fwd_draws (gp_forward.hip), rollout_bwd_draws (gp_backward.hip).
// ts: floats between the time grids of consecutive TRAJECTORIES (not draws: a grid belongs to the sequence), 0 = one (T,) grid shared
// by all of them, T = one row of a dense (N,T) block each.  Read by the fixed-grid rollout and its reverse sweep only.
// sub: equal solver steps per output interval [ts[t], ts[t+1]] (1 ... kMaxSubsteps), read by the same two; the record of an interval
// is then `sub` row blocks (T-1, sub, NS, D), and nothing between the output times reaches zt.
static const int kMaxSubsteps = 64;
struct Draws {
  int nd = 1;
  size_t pack = 0, in = 0, out = 0, in2 = 0, out2 = 0;
  size_t ts = 0;
  int sub = 1;
};

// One argument struct per rollout operation: capi.hip checks the arguments and fills it by member name, the launcher next to the
// kernel turns it into what the kernel takes (the strides between draws, the record's row count: rollout_fwd_draws, rollout_bwd_draws, adapt_fwd_arg).
// Operands are dense, [L,] the draw axis: z0 ([L,] N,Di) (z0_per_draw: one slab per draw, else shared), ts (T,) or (N,T)
// (ts_per_traj), zt / gzt (L,N,T,Di), gz0 (L,N,Di); the fixed-grid record xstage (L,N,T-1,substeps,NS,Di), astage the same in Do.
struct RolloutFwdArgs {
  int M, S; const float* pack; const float* z0; const float* ts; int N, T;
  float* zt; float* xstage; bool z0_per_draw, ts_per_traj; int substeps;
};
// slab (L, nchunk, pack_floats), gpack (L, pack_floats): the fused sweep's parameter sums (rollout_bwd_pgrad); null / 0 for the plain one
struct RolloutBwdArgs {
  int M, S; const float* pack; const float* xstage; const float* gzt; const float* ts; int N, T;
  float* gz0; float* astage; bool ts_per_traj; int substeps; float* slab; int nchunk; float* gpack;
};
// dopri5, landing and dense alike: the record is xstage (L,N,K,6|7,Di), hstep (L,N,K), index (L,N,T-1) (landing: iend, dense: istep)
// and, dense only, theta (L,N,T-1); counts (L,N,4)
struct AdaptFwdArgs {
  int M, S; const float* pack; const float* z0; const float* ts; int N, T, K; float rtol, atol;
  float* zt; float* xstage; float* hstep; int* index; float* theta; int* counts; bool z0_per_draw, ts_per_traj;
};
struct AdaptBwdArgs {
  int M, S; const float* pack; const float* xstage; const float* hstep; const int* index; const float* theta; const float* gzt;
  int N, T, K; float* gz0; float* astage;
};

// The tangent-linear (forward-mode) operations (gp_tangent.hip): K tangent columns per row, one wavefront per (row, column).
// x ([L,] R,Di) (x_per_draw), v ([L,] R,K,Di) with the leading layout of x, null: the identity directions (K == Di);
// f (L,R,Do), may be null; jv (L,R,K,Do)
static const int kMaxTangents = 64;
struct RhsJvpArgs {
  int M, S; const float* pack; const float* x; const float* v; int R, K; float* f; float* jv; int mode; bool x_per_draw;
};
// z0 ([L,] N,Di), v0 ([L,] N,K,Di) with the leading layout of z0, null: the identity; zt (L,N,T,Di), may be null; vt (L,N,T,K,Di)
struct RolloutJvpArgs {
  int M, S; const float* pack; const float* z0; const float* v0; int K; const float* ts; int N, T;
  float* zt; float* vt; bool z0_per_draw, ts_per_traj; int substeps;
};

// entry points implemented across the .hip files
int rhs_jvp(int kernel, int Di, int Do, const RhsJvpArgs& a, int nd, hipStream_t st);
int rollout_jvp(int kernel, int order, int method, int Di, int Do, const RolloutJvpArgs& a, int nd, hipStream_t st);
int dims_supported(int kernel, int Di, int Do);
// the row operations take their Draws as it is:
//   rhs_fwd: in = x, out = f      rhs_vjp: in = x, in2 = a, out = gx      param_grad: in = xr, in2 = ar, out = gpack
int rhs_fwd(int kernel, int Di, int Do, int M, int S, const float* pack, const float* x, int N, float* f, int mode, hipStream_t st,
            Draws dw = Draws{});
int rollout_fwd(int kernel, int order, int method, int Di, int Do, const RolloutFwdArgs& a, int nd, hipStream_t st);
int rollout_bwd(int kernel, int order, int method, int Di, int Do, const RolloutBwdArgs& a, int nd, hipStream_t st);
int rollout_bwd_pgrad_chunks(int kernel, int order, int method, int Di, int Do, int M, int S, int N);
int rollout_bwd_pgrad(int kernel, int order, int method, int Di, int Do, const RolloutBwdArgs& a, int nd, hipStream_t st);
// adaptive Dormand-Prince rollout and its reverse sweep (gp_adaptive.hip).  dense: steps cut at ts[T-1] only, interior outputs
// interpolated (record: 7 rows per step, istep, theta)
int rollout_adaptive_fwd(int kernel, int order, int Di, int Do, const AdaptFwdArgs& a, bool dense, int nd, hipStream_t st);
int rollout_adaptive_bwd(int kernel, int order, int Di, int Do, const AdaptBwdArgs& a, bool dense, int nd, hipStream_t st);
int rhs_vjp(int kernel, int Di, int Do, int M, int S, const float* pack, const float* x, const float* a, int R, float* gx,
            int prior_only, hipStream_t st, Draws dw = Draws{});
int param_grad(int kernel, int Di, int Do, int M, int S, const float* pack, const float* xr, const float* ar, int R,
               float* slab, int nchunk, float* gpack, int accumulate, int prior_only, hipStream_t st, Draws dw = Draws{});
int cache_sizes(int kernel, int Di, int Do, int M, int S, size_t* pack_floats, size_t* ws_floats, int nd = 1);
int cache_build_fwd(int kernel, int Di, int Do, int M, int S, int nd,
                    const float* raw_ell, const float* raw_var, const float* Z, const float* Um, const float* Us_packed,
                    const float* eps_u, const float* rff_w, const float* rff_eps, const float* rff_u,
                    float* pack, float* ws, float* ell, float* var, float* omega, float* phase, float* u,
                    float* Lu, float* nu, float* u_prior, hipStream_t st);

size_t kern_scratch_floats(int kernel, int Di, int Do, int M, int S);
int kern_cache(int kernel, int Di, int Do, int S, const float* raw_ell, const float* raw_var, const float* rff_w, const float* rff_eps,
               const float* rff_u, float* pack, float* omega, float* phase, hipStream_t st);
int compute_nu_ws(int kernel, int Di, int Do, int M, size_t* ws_floats);
int compute_nu(int kernel, int Di, int Do, int M, const float* Ku, const float* u_prior, const float* u, float* nu, float* ws, hipStream_t st);
int f_update(int kernel, int Di, int Do, int M, const float* raw_ell, const float* raw_var, const float* x2, const float* nu,
             const float* x, int N, float* out, float* pack, hipStream_t st);
int kernel_matrix(int kernel, int Di, int Do, const float* raw_ell, const float* raw_var, const float* X, int N,
                  const float* X2, int M2, float* out, hipStream_t st);
int conditional_ws(int Di, int Do, int M, int N, size_t* ws_floats);
int conditional(int Di, int Do, int M, int N, const float* raw_ell, const float* raw_var, const float* Z, const float* Um,
                const float* Us_packed, int us_rank1, const float* x, int full_cov, float* mean, float* var, float* ws, hipStream_t st);
int conditional_df_ws(int D, int M, int N, size_t* ws_floats);
int conditional_df(int D, int M, int N, const float* raw_ell, const float* raw_var, const float* Z, const float* Um,
                   const float* Us_packed, const float* x, int cov_mode, float* mean, float* var, float* ws, hipStream_t st);
int svgp_kl_fwd(int M, int Do, const float* Um, const float* Us, float* kl, hipStream_t st);
int noise_fill(float* out, long long n_normal, long long n_uniform, unsigned long long seed, unsigned long long* state, hipStream_t st);
int svgp_kl_bwd(int M, int Do, const float* Um, const float* Us, const float* g, float* dUm, float* dUs, hipStream_t st);

void set_backward_solves(int mode);
int get_backward_solves();
int cache_bwd_sizes(int kernel, int Di, int Do, int M, int S, int nd, size_t* bws_floats);
int cache_build_bwd(int kernel, int Di, int Do, int M, int S, int nd, const float* raw_ell, const float* raw_var, const float* Z,
                    const float* eps_u, const float* pack, const float* ws, float* gpack, float* bws,
                    float* g_raw_ell, float* g_raw_var, float* g_Z, float* g_Um, float* g_Us, int prepared, hipStream_t st);
int cache_bwd_prepare(int kernel, int Di, int Do, int M, int S, int nd, const float* ws, float* bws, hipStream_t st);

// conv VAE blocks, the loss stage and the evaluation epilogue: one argument struct per operation, as the rollouts above.
// capi.hip checks the pointers and the sizes and fills the structs by member name; grids, chunks and LDS sizes are computed beside the
// kernel that is launched.  `who`: the export the error texts start with; `ragged`: the export takes a frame count per sequence.
// The convolution as the exports describe it, x (B,Ci,H,W) -> y (B,Co,Ho,Wo); the direct kernels' ConvDims is made from it (vae_conv.hip)
struct ConvGeom { int B, Ci, H, W, Co, K, S, P, Ho, Wo; };
int conv2d_fwd(const float* x, const float* w, const float* bias, float* y, const ConvGeom& g, hipStream_t st, size_t xbs = 0);
size_t convT_fwd_stats_scratch(int Co_out);
int convT_fwd_stats(const float* x, const float* x_bn, const float* w, const float* bias, float* y, const ConvGeom& g, const float* gamma,
                    const float* beta, float* save_mean, float* save_invstd, float* running_mean, float* running_var, long long* nbt,
                    float momentum, float eps, float* table, float* scratch, int slot, hipStream_t st);
int conv2d_bwd_data(const float* gy, const float* w, const float* bias, float* gx, const ConvGeom& g, const float* gy_bn, hipStream_t st);
size_t conv_wgrad_scratch(int B, int Ci, int Co, int K);
int conv2d_bwd_weight(const float* x, const float* gy, float* gw, float* gbias, float* scratch, const ConvGeom& g, const float* gy_bn,
                      hipStream_t st, size_t xbs = 0);
size_t bn_scratch(int B, int C);
int bn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_invstd,
           float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, int B, int C, int HW,
           int relu, float* scratch, hipStream_t st);
int bn_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
           float* gx, float* ggamma, float* gbeta, float* gx_chansum, int B, int C, int HW, int relu, float* scratch, hipStream_t st);
int bn_stats(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd, float* running_mean,
             float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table, int B, int C, int HW,
             float* scratch, hipStream_t st);
int bn_moments(const float* x, float* mom, int B, int C, int HW, float* scratch, hipStream_t st);
int bn_finalize(const float* gathered, int W, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table, int C,
                hipStream_t st);
int bn_apply(const float* x, const float* table, float* y, int B, int C, int HW, int relu, hipStream_t st);
// decnn.10's input gradient fused with the BatchNorm + ReLU backward in front of it (vae_conv_tiled.hip)
int dec10_bn_scratch_floats();
int dec10_bn_bwd_sums(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* mean,
                      const float* invstd, float* sums, int B, float* scratch, hipStream_t st, float* gw = nullptr, float* wscratch = nullptr, float* gbias = nullptr);
int dec10_bn_wgrad_scratch_floats();
int dec10_bn_bwd_apply(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* mean,
                       const float* invstd, const float* gathered, const float* wts, int W, float count_all, float* gc, float* ggamma,
                       float* gbeta, float* gc_chansum, int B, float* scratch, hipStream_t st);
// final reductions of per-workgroup partials, recorded between defer_reductions(1) / (0) and run together by flush_reductions
// (vae_norm.hip); outside such a bracket reduce_job launches at once
struct RedJob { const float* part; float* out; int nsplit, n, kind, a, b, c; };
int reduce_job(const RedJob& job, hipStream_t st);
int reduce_jobs(const RedJob* jobs, int nj, hipStream_t st);
void defer_reductions(int mode);
int flush_reductions(hipStream_t st);
int bn_bwd_sums(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                float* sums, int B, int C, int HW, int relu, float* scratch, hipStream_t st);
int bn_bwd_apply(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                 const float* gathered, const float* wts, int W, float count, float* gx, float* ggamma, float* gbeta, float* gx_chansum, int B, int C, int HW, int relu,
                 float* scratch, hipStream_t st);
int bn_eval(const float* x, const float* gy, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
            float eps, float* out, int B, int C, int HW, int relu, hipStream_t st);
int bn_eval_table(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* table, int C,
                  hipStream_t st);
// decnn.10 of a frozen decoder fused with the predictive statistics over the draws (vae_conv_tiled.hip): c (Lc,F,16,32,32), X (F/Th,T_obs,
// 28,28); ell (L_total,F) with ll, n_obs (F/Th) when ragged -- k_fwd_predict<ll, ragged>
struct PredictArgs {
  const float* c; const float* table; const float* w; const float* bias; const float* X; int Lc, F, Th, T_obs, done;
  float* pred_mean; float* pred_m2; float* se_state; float* ell; int L_total; const int* n_obs;
};
int dec10_predict(const char* who, bool ll, bool ragged, const PredictArgs& a, hipStream_t st);
// ... with a log-weight per (draw, sequence): logw (L_total,N), F = N Th; wstate (F,2) = {ref, W}, wse (F); n_obs (N) or null --
// k_fwd_predict_w
struct PredictWArgs {
  const float* c; const float* table; const float* w; const float* bias; const float* X; int Lc, F, Th, T_obs, done;
  const float* logw; int L_total, N; float* wstate; float* pred_mean; float* pred_m2; float* wse; const int* n_obs;
};
int dec10_predict_w(const char* who, const PredictWArgs& a, hipStream_t st);
int chan_sum(const float* v, float* out, int B, int C, int HW, float* scratch, hipStream_t st);
int act_fwd(const float* x, float* y, size_t n, int mode, hipStream_t st);
int act_bwd(const float* y, const float* gy, float* gx, size_t n, int mode, hipStream_t st);
int linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, hipStream_t st);
int linear_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out, float* scratch, hipStream_t st);
size_t linear_bwd_scratch(int B, int In, int Out);
int linear_relu_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, hipStream_t st);
int linear_relu_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out, hipStream_t st);
int loglik_fwd(const float* X, const float* z, float* ll, size_t n, size_t nX, hipStream_t st);
int loglik_bwd(const float* X, const float* z, const float* g, float* gz, size_t n, size_t nX, hipStream_t st);
// Ragged minibatches: sequence n owns the frames t < n_obs[n] of its T padded ones, `frame` elements each.  A null n_obs means every
// frame: what the kernels' <false> instantiations get.  An export that takes counts (`ragged`) refuses a null one.
struct FrameMask { const int* n_obs = nullptr; int T = 0; size_t frame = 0; };
// `rows` rows (draw, sequence) of `inner` elements; the targets X (nX elements) repeat over the draws.  z: the probabilities an operation
// reads (the sigmoid forward writes them and takes them with its outputs)
struct LogLikRows { const float* X; const float* z; size_t rows, inner, nX; };
int loglik_rowsum_fwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, float* out, hipStream_t st);
int loglik_rowsum_bwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, const float* grow, float* gz, hipStream_t st);
int sigmoid_loglik_splits(size_t rows, size_t inner);
int sigmoid_loglik_fwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, const float* a, float* z, float* part,
                       int nsplit, hipStream_t st);
int sigmoid_loglik_bwd(const char* who, bool ragged, const LogLikRows& r, const FrameMask& m, const float* grow, float* ga, hipStream_t st);
// ragged minibatches with the padding taken out in front of the decoder: the frame gather and the likelihood over compact logits.
// index: off (exclusive prefix sum of the clamped counts, N + 1 entries, P = off[N]) for the forward, src (src[j] = n T + t of compact
// image j, P entries) for the backward, which alone reads P; r.inner is not read (a row has off[n + 1] - off[n] frames)
struct PackedFrames { const int* index; int P, T; size_t frame; };
int gather_frames_fwd(const float* zt, int ld, int q, const int* src, int L, int N, int T, int P, float* out, hipStream_t st);
int gather_frames_bwd(const float* gout, int ld, int q, const int* off, int L, int N, int T, int P, float* gzt, hipStream_t st);
int sigmoid_loglik_fwd_pk(const LogLikRows& r, const PackedFrames& pk, const float* a, float* z, float* part, int nsplit, hipStream_t st);
int sigmoid_loglik_bwd_pk(const LogLikRows& r, const PackedFrames& pk, const float* grow, float* ga, hipStream_t st);
int reparam_kl_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, float* klpart, int N, int q, hipStream_t st);
int reparam_kl_bwd(const float* gz, const float* gklpart, const float* mu, const float* logvar, int ld, const float* eps, float* gmu,
                   float* glogvar, int ldg, int N, int q, hipStream_t st);
int reparam_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int N, int q, hipStream_t st);
int reparam_draws_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int ldz, float* lw, int accumulate, int L, int N,
                      int q, hipStream_t st);
int reparam_draws_bwd(const float* gz, int ldgz, const float* glw, const float* mu, const float* logvar, int ld, const float* eps, float* gmu,
                      float* glogvar, int ldg, int K, int N, int q, hipStream_t st);
// The ELBO assembled in one launch and its backward (vae_loss.hip).  N sequences, q latent dimensions, the inducing posterior Um (M,Do) /
// Us (packed factors), nobs = the data-set size the likelihood is scaled to
struct ElboShape { int N, q, M, Do; const float* Um; const float* Us; float nobs; };
// the upstream gradients of the four outputs (loss, nll, kl, kl_u); a null one counts as zero
struct ElboSeeds { const float* g0; const float* g1; const float* g2; const float* g3; };
// The latent KL term comes in one of two forms.  heads: the encoder's mean / log-variance hs, hv (N,q) and their gradients (hs set).
// values: KL partials computed upstream, kls (nks) and klv (nkv), and their gradients (hs null; q is not read).
struct ElboKl {
  const float* hs = nullptr; const float* hv = nullptr; float* ghs = nullptr; float* ghv = nullptr;
  const float* kls = nullptr; const float* klv = nullptr; float* gkls = nullptr; float* gklv = nullptr; int nks = 0, nkv = 0;
};
struct ElboGrads { float* glrow; float* dUm; float* dUs; };   // the likelihood's row gradients (nl_rows) and the inducing posterior's
// the decoder's logits for the fused backward: ga (n) = d loss / d logits from the probabilities z and the targets X (nX, repeating)
struct ElboLogits { const float* X; const float* z; float* ga; size_t n, nX; };
int elbo_all_fwd(const float* lpart, int nl_rows, int nl_values, const ElboShape& s, const ElboKl& kl, float* out, hipStream_t st);
int elbo_all_bwd(const ElboSeeds& g, int nl_rows, const ElboShape& s, const ElboKl& kl, const ElboGrads& o, hipStream_t st);
int elbo_loglik_bwd(const char* who, bool ragged, const ElboSeeds& g, int nl_rows, const ElboShape& s, const ElboKl& kl, const ElboGrads& o,
                    const ElboLogits& lg, const FrameMask& m, hipStream_t st);
// the importance-weighted bound over K initial-state draws per sequence: lpart (rows, nsplit) likelihood partials, lw (L,K,N) log-weights
struct IwDraws { const float* lpart; int rows, nsplit; const float* lw; int L, K; };
int elbo_iw_fwd(const IwDraws& iw, const ElboShape& s, float* out, hipStream_t st);
// o.glrow: the rows' gradients; ll: the likelihood's backward over the logits in the same launch (lg is not read without it)
int elbo_iw_bwd(const char* who, bool ll, const ElboSeeds& g, const IwDraws& iw, const ElboShape& s, const ElboGrads& o, float* glw,
                const ElboLogits& lg, hipStream_t st);
int reparam_bwd(const float* gz, const float* logvar, int ld, const float* eps, float* gmu, float* glogvar, int ldg, int N, int q, hipStream_t st);
int normal_kl_fwd(const float* mu, const float* logvar, int ld, float* klrow, int N, int q, hipStream_t st);
int normal_kl_bwd(const float* grow, const float* mu, const float* logvar, int ld, float* gmu, float* glogvar, int ldg, int N, int q, hipStream_t st);
int elbo_fwd(const float* lhood, int nl, const float* klrow, int nk, const float* kl_u, float nobs, float* out, hipStream_t st);
int elbo_bwd(const float* gout, int nl, int nk, float nobs, float* glhood, float* gklrow, float* gklu, hipStream_t st);
int gather_multi(const float* const* grads, const long long* offs, int ntensors, long long total, float* flat, hipStream_t st);
int adam_multi(float* const* params, const float* const* grads, float* const* m1, float* const* m2, const long long* offs,
               int ntensors, long long total, float lr, float beta1, float beta2, float eps, int step, int* step_dev, hipStream_t st);

// big factors (np a multiple of 128, >= 1024) take the panelled / matrix-core kernels; GPODE_SMALL_FACTOR_KERNELS=1 keeps the
// 32-tile kernels for every size (an A/B switch for tests and profiling, same results up to summation order)
inline bool big_factor(int np) {
  static const bool off = env_flag("GPODE_SMALL_FACTOR_KERNELS");
  return !off && np % 128 == 0 && np >= 1024;
}

}  // namespace gp
