/* gpode.h -- C ABI of the MI355X-native GP-ODE hot path (libgpode_hip.so).
 *
 * Drop-in boundary for the reference's Python operator API
 * (/root/reference/experiments/model/core/{svpy,kernels,flow}.py).  The reference has no FFI
 * layer of its own; each entry point below names the reference method it replaces, and
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated otherwise;
 *  - the library never allocates, frees or retains caller memory; scratch is passed in (`ws`);
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *  - return value 0 = ok, non-zero = error (message via gpode_last_error()); the Python host
 *    raises RuntimeError on non-zero;
 *  - all randomness enters as explicit tensors: eps_u (M,Do), rff_w (S,Do) [DF (2S,Do)],
 *    rff_eps (Di,S,Do), rff_u (1,S,Do) in [0,1).
 *
 *  kernel: 0 = RBF dimwise  (kernels.py:29-195),  1 = divergence-free (kernels.py:201-393, Di==Do)
 *  order : 1 | 2            (flow.py:27-45)
 *  method: 0 = euler, 1 = rk4 (torchdiffeq fixed-grid 3/8 rule; flow.py:76-85), 2 = midpoint (y1 = y + dt f(y + dt/2 f(y))),
 *          3 = dopri5 (adaptive Dormand-Prince 5(4)) -- the gpode_rollout_adaptive_* entry points only; the fixed-grid ones refuse it
 */
#ifndef GPODE_H
#define GPODE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPODE_KERNEL_RBF 0
#define GPODE_KERNEL_DF 1
#define GPODE_METHOD_EULER 0
#define GPODE_METHOD_RK4 1
#define GPODE_METHOD_MIDPOINT 2
#define GPODE_METHOD_DOPRI5 3

/* Library / build identification. */
const char* gpode_version(void);
const char* gpode_last_error(void);
/* Tag of the launcher that ran last on the calling thread ("" before the first): which kernel a dispatching entry point chose,
 * e.g. "conv_v2_dec7_fwd_bn_stats" (second convolution engine) or "convT_fwd_mfma_stats" (first).  For tests and diagnosis. */
const char* gpode_last_launch(void);
/* 1 if (kernel,Di,Do) has a compiled specialisation. */
int gpode_supported(int kernel, int Di, int Do);

/* Sizes (in floats) of the packed per-draw cache consumed by rhs/rollout, and of the scratch
 * workspace gpode_cache_build_fwd needs. */
int gpode_cache_sizes(int kernel, int Di, int Do, int M, int S, size_t* pack_floats, size_t* ws_floats);

/* SVGP_Layer.build_cache (svpy.py:103-121): kern.build_cache (kernels.py:126-137 / :305-316),
 * sample_inducing (svpy.py:88-101), kern.K(Z) (kernels.py:98-110 / :289-303), kern.rff_forward(Z),
 * kern.compute_nu (kernels.py:155-172 / :376-387).
 * Inputs are the raw optvars of the state_dict and the noise.  `pack` receives the lane-major cache
 * used by the kernels below.  The remaining outputs mirror the attributes the reference caches on
 * `kern` and may be NULL: ell (Do,Di), var (Do), omega (Di,S,Do), phase (1,S,Do), u (M,Do),
 * Lu (RBF: (Do,M,M); DF: (M*D,M*D)), nu (RBF: (Do,M); DF: (M*D)), u_prior (M,Do). */
int gpode_cache_build_fwd(int kernel, int Di, int Do, int M, int S,
                          const float* raw_ell, const float* raw_var, const float* Z,
                          const float* Um, const float* Us_packed,
                          const float* eps_u, const float* rff_w, const float* rff_eps, const float* rff_u,
                          float* pack, float* ws,
                          float* ell, float* var, float* omega, float* phase, float* u,
                          float* Lu, float* nu, float* u_prior, void* stream);

/* SVGP_Layer.forward (svpy.py:123-142): f(x) = rff_forward(x) + f_update(x, Z).
 * x (N,Di) -> f (N,Do).  mode: 0 = prior + update, 1 = prior only, 2 = update only. */
int gpode_rhs_fwd(int kernel, int Di, int Do, int M, int S, const float* pack,
                  const float* x, int N, float* f, int mode, void* stream);

/* Flow.forward (flow.py:68-86) given a built cache: z0 (N,D), ts (T) -> zt (N,T,D),
 * D = Di = order*Do.  One fixed-grid step per output interval (the `_ns` entry points below take several).
 * xstage (nullable): (N, T-1, NS, D) receives the input of every RHS evaluation (NS = 1 euler, 4 rk4);
 * pass it when gradients are needed -- gpode_rollout_bwd walks it backwards. */
int gpode_rollout_fwd(int kernel, int order, int method, int Di, int Do, int M, int S,
                      const float* pack, const float* z0, const float* ts, int N, int T,
                      float* zt, float* xstage, void* stream);

/* Gradient of a scalar loss through Flow.forward = what loss.backward() computes through the unrolled
 * solver in the reference (main.py:209-210, use_adjoint=False).
 *   gzt (N,T,D) = dL/dzt  ->  gz0 (N,D) = dL/dz0  and  astage (N,T-1,NS,Do) = dL/df at every RHS evaluation. */
int gpode_rollout_bwd(int kernel, int order, int method, int Di, int Do, int M, int S,
                      const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                      float* gz0, float* astage, void* stream);

/* gx (R,Di) = J_f(x)^T a for rows x (R,Di), a (R,Do): autograd of SVGP_Layer.forward w.r.t. its input. */
int gpode_rhs_vjp(int kernel, int Di, int Do, int M, int S, const float* pack,
                  const float* x, const float* a, int R, float* gx, void* stream);

/* Parameter gradient of sum_r <a_r, f(x_r)> in PACK LAYOUT (same indexing as `pack`: d/d of every record
 * field and of the uniform tail); rows x (R,Di), a (R,Do).  slab: nchunk * pack_floats floats of scratch.
 * accumulate != 0 adds into gpack.  Deterministic (fixed-order two-stage sum, no float atomics). */
int gpode_param_grad(int kernel, int Di, int Do, int M, int S, const float* pack,
                     const float* x, const float* a, int R, float* slab, int nchunk, float* gpack, int accumulate,
                     void* stream);

/* Backward of gpode_cache_build_fwd: what autograd does behind SVGP_Layer.build_cache in the reference
 * (nu = L^-T(u - L^-1 f_prior(Z)), cholesky, K(Z), omega = eps/ell, softplus ...).
 *   gpack : in/out, pack-layout gradient from gpode_param_grad (the f_prior(Z) path is added to it);
 *   ws    : the workspace the forward of THIS draw wrote;  bws: gpode_cache_bwd_sizes() floats of scratch;
 *   outputs: gradients w.r.t. the five raw parameter tensors, in their state_dict layouts;
 *   prepared: bit 0 -- bws went through gpode_cache_bwd_prepare (below); bit 1 -- g_Um / g_Us already HOLD a gradient (that of
 *   KL(q(u)||p(u)), svpy.py:144-175, which reaches the same two parameters) and the flow's is ADDED to it: what autograd's
 *   accumulation of the two paths would do in one more launch each. */
int gpode_cache_bwd_sizes(int kernel, int Di, int Do, int M, int S, size_t* bws_floats);
int gpode_cache_build_bwd(int kernel, int Di, int Do, int M, int S,
                          const float* raw_ell, const float* raw_var, const float* Z, const float* eps_u,
                          const float* pack, const float* ws, float* gpack, float* bws,
                          float* g_raw_ell, float* g_raw_var, float* g_Z, float* g_Um, float* g_Us, int prepared, void* stream);
/* The gradient-independent part of the above (L^-1 from the factor in ws, written into bws).  Optional: call it any time
 * after gpode_cache_build_fwd -- e.g. on a side stream while the decoder runs -- and pass prepared = 1 with the same bws. */
int gpode_cache_bwd_prepare(int kernel, int Di, int Do, int M, int S, const float* ws, float* bws, void* stream);

/* ---- Monte-Carlo draws batched into one call ------------------------------------------------------------------------------
 * ODEGPVAE.sample_trajectories (odegpvae.py:37-45) loops `for l in range(L)` over whole flow calls -- L cache builds, L solver
 * loops, L autograd graphs -- and the training loop runs half of all epochs at L = 5 (main.py:200).  K_uu + jitter I and its
 * Cholesky factor depend on the parameters only (kernels.py:163 / :384), so the `_n` forms below build ONE factor for all
 * `ndraws` function draws (their right-hand sides f_prior_l(Z) are solved as a block), integrate the L * N trajectories in ONE
 * launch (the launch's second grid dimension is the draw: its own pack, the shared initial states) and run ONE Cholesky
 * backward on the summed adjoint (that VJP is linear).  Layouts: every per-draw operand gains a LEADING draw axis --
 *   eps_u (L,M,Do), rff_w (L,S|2S,Do), rff_eps (L,Di,S,Do), rff_u (L,1,S,Do); pack (L, pack_floats); omega / phase / u / nu /
 *   u_prior (L, ...); zt (L,N,T,D), xstage (L,N,T-1,NS,D), gzt, gz0 (L,N,D), astage; x / a of gpode_param_grad_n (L,R,.),
 *   slab (L, nchunk, pack_floats), gpack (L, pack_floats) --
 * while z0 (N,D), ts, the raw parameters, ell, var, Lu and the factor inside `ws` are shared.  gpode_cache_build_bwd_n returns the
 * parameter gradients SUMMED over the draws (what autograd accumulates over the reference's loop).  ws / bws sizes depend on
 * ndraws (gpode_cache_sizes_n, gpode_cache_bwd_sizes_n); pack_floats does not.  ndraws = 1 is the un-suffixed entry point. */
int gpode_cache_sizes_n(int kernel, int Di, int Do, int M, int S, int ndraws, size_t* pack_floats, size_t* ws_floats);
int gpode_cache_build_fwd_n(int kernel, int Di, int Do, int M, int S, int ndraws,
                            const float* raw_ell, const float* raw_var, const float* Z,
                            const float* Um, const float* Us_packed,
                            const float* eps_u, const float* rff_w, const float* rff_eps, const float* rff_u,
                            float* pack, float* ws,
                            float* ell, float* var, float* omega, float* phase, float* u,
                            float* Lu, float* nu, float* u_prior, void* stream);
int gpode_rollout_fwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                        const float* pack, const float* z0, const float* ts, int N, int T,
                        float* zt, float* xstage, void* stream);
int gpode_rollout_bwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                        const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                        float* gz0, float* astage, void* stream);
/* Adaptive rollout (method = GPODE_METHOD_DOPRI5): Dormand-Prince 5(4) with one step-size controller per trajectory, steps landing
 * on the output times ts (strictly increasing), tolerances rtol / atol on the RMS norm over the state.  K = accepted steps a
 * trajectory may take (the capacity of its record).
 *   zt     (L,N,T,D)      the states at ts; NaN from the first output a failed trajectory did not reach
 *   counts (L,N,4) int32  accepted steps, rejected steps, status (0 ok, 1 budget K exhausted, 2 step size underflow,
 *                         3 ts not increasing), evaluations of f (= 1 + 6 (accepted + rejected))
 * and, when gradients are needed (xstage != NULL; with xstage == NULL nothing but zt and counts is written):
 *   xstage (L,N,K,6,D)    the six stage inputs of every accepted step, consecutively     } zero past a trajectory's
 *   hstep  (L,N,K)        the accepted step sizes                                        } count of accepted steps
 *   iend   (L,N,T-1) int32  accepted steps taken when output t+1 was reached (non-decreasing)
 * gpode_rollout_adaptive_bwd_n walks the record backwards (step sizes constant; rejected steps and the error estimate carry no
 * gradient): gzt (L,N,T,D) -> gz0 (L,N,D), astage (L,N,K,6,Do) = dL/df at every recorded evaluation, zero past the count -- so
 * gpode_param_grad_n runs over all K * 6 rows of (xstage, astage) unchanged.  No fused parameter-gradient form
 * (gpode_rollout_bwd_pgrad_chunks returns 0 for this method). */
int gpode_rollout_adaptive_fwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                 const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                                 float* zt, float* xstage, float* hstep, int* iend, int* counts, void* stream);
int gpode_rollout_adaptive_bwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                 const float* pack, const float* xstage, const float* hstep, const int* iend, const float* gzt,
                                 int N, int T, int K, float* gz0, float* astage, void* stream);
/* The adaptive rollout with DENSE OUTPUT (flow.py:76-86 with torchdiffeq's free-stepping dopri5): the controller of
 * gpode_rollout_adaptive_fwd_n, but a step is cut only at the last output time ts[T-1] and the first step is capped by
 * ts[T-1] - ts[0]; the interior outputs are read off the 4th-order continuous extension of the pair (Shampine; Hairer, Noersett,
 * Wanner II.6), z(theta) = y_n + h sum_{j=1..7} w_j(theta) k_j, which costs no evaluation (counts as above).  The last output is the
 * end state of the last step.  Record, written when xstage != NULL, zero past a trajectory's count:
 *   xstage (L,N,K,7,D)      the six stage inputs of every accepted step and its end state (the input of the seventh slope)
 *   hstep  (L,N,K)          the accepted step sizes
 *   istep  (L,N,T-1) int32  1-based number of the accepted step that holds output t+1 (non-decreasing; several outputs may share
 *                           a step, a step may hold none); the count of accepted steps for outputs a failed trajectory did not reach
 *   theta  (L,N,T-1)        (ts[t+1] - t_n) / h inside that step, in (0, 1]; exactly 1 for the last output
 * gpode_rollout_dense_bwd_n (flow.py:76-86, the gradient of the above): gzt (L,N,T,D) -> gz0 (L,N,D), astage (L,N,K,7,Do) = dL/df at
 * every recorded evaluation; row 6 of a step is zero unless the step holds an output with theta < 1 (w_7(1) = 0), rows past the count
 * are zero -- gpode_param_grad_n runs over all K * 7 rows of (xstage, astage).  Deterministic, no atomics. */
int gpode_rollout_dense_fwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                              const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                              float* zt, float* xstage, float* hstep, int* istep, float* theta, int* counts, void* stream);
int gpode_rollout_dense_bwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                              const float* pack, const float* xstage, const float* hstep, const int* istep, const float* theta,
                              const float* gzt, int N, int T, int K, float* gz0, float* astage, void* stream);
/* The batched rollouts with an initial state PER DRAW (the joint samples (z0_l, f_l) of the importance-weighted marginal
 * likelihood, evaluate.predict_marginal): the arguments of the `_n` twin plus `z0_per_draw`, in front of `stream`.
 *   z0_per_draw = 0   z0 is (N,D), shared by all draws: the same launch, the same bits as the `_n` entry point
 *   z0_per_draw = 1   z0 is (ndraws,N,D), dense: draw l starts from slab l
 * Any other value is refused before anything is launched.  The reverse sweeps are the `_n` ones: gz0 is (L,N,D) already, and is
 * the gradient of the per-draw z0 as it stands (not summed over the draws). */
int gpode_rollout_fwd_nz(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* z0, const float* ts, int N, int T,
                         float* zt, float* xstage, int z0_per_draw, void* stream);
int gpode_rollout_adaptive_fwd_nz(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                  const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                                  float* zt, float* xstage, float* hstep, int* iend, int* counts, int z0_per_draw, void* stream);
int gpode_rollout_dense_fwd_nz(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                               float* zt, float* xstage, float* hstep, int* istep, float* theta, int* counts, int z0_per_draw,
                               void* stream);
/* The rollouts and the fixed-grid reverse sweeps with a time grid PER TRAJECTORY (sequences observed at their own times): the
 * arguments of the twin named plus `ts_per_traj`, directly in front of `stream`.
 *   gpode_rollout_fwd_nt           gpode_rollout_fwd_nz             gpode_rollout_bwd_nt         gpode_rollout_bwd_n
 *   gpode_rollout_adaptive_fwd_nt  gpode_rollout_adaptive_fwd_nz    gpode_rollout_bwd_pgrad_nt   gpode_rollout_bwd_pgrad_n
 *   gpode_rollout_dense_fwd_nt     gpode_rollout_dense_fwd_nz
 *   ts_per_traj = 0   ts is (T,), shared by all trajectories: the same launch, the same bits as the twin
 *   ts_per_traj = 1   ts is (N,T), dense: row n is the grid of trajectory n of EVERY draw -- a grid belongs to the sequence, not to
 *                     the function draw, so it has no draw axis
 * Any other value is refused before anything is launched (gpode_last_error() says so).  The route, and with it the tag
 * gpode_last_launch() returns, does not depend on the grid.  Every other operand keeps the layout of the twin; T is the same for all
 * trajectories (sequences with different numbers of observations are not covered).  The adaptive reverse sweeps read the recorded
 * step sizes and theta only, never ts: gpode_rollout_adaptive_bwd_n / gpode_rollout_dense_bwd_n serve either kind of grid.
 * Status 3 of the adaptive rollouts is per trajectory here: only the trajectory whose own row is not strictly increasing stops
 * (landing mode: at the first interval that is not; dense mode: before its first step) and turns NaN from the first output it did
 * not reach; every other trajectory of the launch is unaffected. */
int gpode_rollout_fwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* z0, const float* ts, int N, int T,
                         float* zt, float* xstage, int z0_per_draw, int ts_per_traj, void* stream);
int gpode_rollout_adaptive_fwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                  const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                                  float* zt, float* xstage, float* hstep, int* iend, int* counts, int z0_per_draw, int ts_per_traj,
                                  void* stream);
int gpode_rollout_dense_fwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                               float* zt, float* xstage, float* hstep, int* istep, float* theta, int* counts, int z0_per_draw,
                               int ts_per_traj, void* stream);
int gpode_rollout_bwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                         float* gz0, float* astage, int ts_per_traj, void* stream);
int gpode_rollout_bwd_pgrad_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                               float* gz0, float* astage, float* slab, int nchunk, float* gpack, int ts_per_traj, void* stream);
/* The fixed-grid rollout and its reverse sweeps with SUB-STEPS between the output times (the reference's --ts_dense_scale,
 * torchdiffeq's options=dict(step_size=...)): the arguments of the `_nt` twin plus `substeps`, directly in front of `stream`.
 *   gpode_rollout_fwd_ns  gpode_rollout_fwd_nt      gpode_rollout_bwd_ns  gpode_rollout_bwd_nt
 *   gpode_rollout_bwd_pgrad_ns  gpode_rollout_bwd_pgrad_nt
 * Every output interval [ts[t], ts[t+1]] of every trajectory is integrated in `substeps` equal steps of h = (ts[t+1] - ts[t]) /
 * substeps (one fp32 division per interval; the right-hand side is autonomous, so only h matters).  Outputs stay at ts: zt, gzt and
 * gz0 keep the twin's layout, and nothing between the output times is written to zt.  The record grows by the sub-step axis,
 *   xstage ([L,] N, T-1, substeps, NS, D)     astage ([L,] N, T-1, substeps, NS, Do)
 * contiguous -- the same bytes as ([L,] N, (T-1)*substeps, NS, .) -- so gpode_param_grad_n runs over all its rows unchanged, and
 * gpode_rollout_bwd_pgrad_chunks (which does not depend on the count) sizes the slab of the fused form as before.  The reverse
 * sweep walks intervals and sub-steps backwards; gzt[t] enters when the walk reaches the start of interval t.
 *   substeps = 1        the same launch, the same tag, the same bits as the twin
 *   substeps 1 ... 64   accepted; any other value is refused before anything is launched (gpode_last_error() names the entry
 *                       point) and nothing is written
 * method = GPODE_METHOD_DOPRI5 is refused as in the twins.  The route, and with it the tag gpode_last_launch() returns, does not
 * depend on substeps. */
/* For tests.  The rollout kernels exist in two instantiations: the one-step one, which the twins and substeps = 1 launch (the code they
 * always ran), and the sub-step one, which every other count launches.  on = 1 sends one-step launches through the sub-step
 * instantiation as well, so that a test can hold that instantiation to itself on a refined grid (two separately compiled kernels
 * need not round alike); on = 0 is the state the library starts in.  Any other value is refused.  Process-wide, not thread-safe. */
int gpode_test_substep_kernels(int on);
int gpode_rollout_fwd_ns(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* z0, const float* ts, int N, int T,
                         float* zt, float* xstage, int z0_per_draw, int ts_per_traj, int substeps, void* stream);
int gpode_rollout_bwd_ns(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                         float* gz0, float* astage, int ts_per_traj, int substeps, void* stream);
int gpode_rollout_bwd_pgrad_ns(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                               float* gz0, float* astage, float* slab, int nchunk, float* gpack, int ts_per_traj, int substeps,
                               void* stream);
/* Forward mode (tangent-linear): J_f(x) v of the sampled field, and the state-transition matrix Phi_t = d z_t / d z0 of the fixed-grid
 * rollout applied to K directions -- the exact derivative of the discrete step map gpode_rollout_fwd computes (the transpose of what
 * gpode_rollout_bwd applies).  One wavefront per (row, direction); records streamed from L2 (tags rhs_jvp_{rbf,df}_stream,
 * rollout_jvp_{rbf,df}_stream).  Shapes, L = ndraws:
 *   x  (R,Di), or (L,R,Di) with x_per_draw = 1        v  (R,K,Di) / (L,R,K,Di), the leading layout of x
 *   f  (L,R,Do), may be NULL                           jv (L,R,K,Do),   jv[l,r,k,:] = J_f(x[r]) v[r,k,:]
 *   z0 (N,Di), or (L,N,Di) with z0_per_draw = 1       v0 (N,K,Di) / (L,N,K,Di), the leading layout of z0
 *   zt (L,N,T,Di), may be NULL                         vt (L,N,T,K,Di), vt[l,n,t,k,:] = Phi_t v0[n,k,:], vt[.,.,0] = v0
 *   ts (T,), or (N,T) with ts_per_traj = 1;  substeps 1 ... 64 equal steps per output interval
 * v / v0 NULL: the identity directions; needs K == Di, and then Phi_t[i,k] = vt[...,t,k,i].  mode as gpode_rhs_fwd (0 full, 1 prior,
 * 2 update).  Refused before anything is launched, with nothing written and the reason in gpode_last_error(): a NULL pack, x, z0,
 * jv, vt or ts; K outside 1 ... 64, or K != Di with NULL directions; N, R or T < 1; substeps outside 1 ... 64; Di != order * Do; a
 * width that is not compiled; mode outside 0 ... 2; a method other than euler, midpoint or rk4 -- dopri5's steps depend on the
 * state through the controller, and the tangent of the accepted-step sequence is not built. */
int gpode_rhs_jvp(int kernel, int Di, int Do, int M, int S, int ndraws, const float* pack,
                  const float* x, int x_per_draw, const float* v, int R, int K,
                  float* f, float* jv, int mode, void* stream);
int gpode_rollout_jvp(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws, const float* pack,
                      const float* z0, int z0_per_draw, const float* v0, int K,
                      const float* ts, int ts_per_traj, int substeps, int N, int T,
                      float* zt, float* vt, void* stream);
/* gpode_rollout_bwd_n and gpode_param_grad_n in ONE pass: the reverse sweep visits every (stage input, adjoint) row anyway, so the
 * rows' parameter-gradient terms are accumulated on the way and come out as gpack (ndraws, pack_floats) -- what the two calls
 * produce together, with one launch and one pass over the rows less.  slab: ndraws * nchunk * pack_floats floats of scratch with
 * nchunk = gpode_rollout_bwd_pgrad_chunks(...) -- 0 means this shape has no fused form (streamed teams, second-order models,
 * midpoint rule): call the two entry points then.  gz0 / astage as gpode_rollout_bwd_n. */
int gpode_rollout_bwd_pgrad_chunks(int kernel, int order, int method, int Di, int Do, int M, int S, int N);
int gpode_rollout_bwd_pgrad_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                              const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                              float* gz0, float* astage, float* slab, int nchunk, float* gpack, void* stream);
int gpode_param_grad_n(int kernel, int Di, int Do, int M, int S, int ndraws, const float* pack,
                       const float* x, const float* a, int R, float* slab, int nchunk, float* gpack, int accumulate,
                       void* stream);
int gpode_cache_bwd_sizes_n(int kernel, int Di, int Do, int M, int S, int ndraws, size_t* bws_floats);
int gpode_cache_build_bwd_n(int kernel, int Di, int Do, int M, int S, int ndraws,
                            const float* raw_ell, const float* raw_var, const float* Z, const float* eps_u,
                            const float* pack, const float* ws, float* gpack, float* bws,
                            float* g_raw_ell, float* g_raw_var, float* g_Z, float* g_Um, float* g_Us, int prepared, void* stream);
int gpode_cache_bwd_prepare_n(int kernel, int Di, int Do, int M, int S, int ndraws, const float* ws, float* bws, void* stream);

/* Factorisation status of the last gpode_cache_build_fwd on `ws` (bit 0: K_uu + jitter I not positive
 * definite -- torch.linalg.cholesky raises there, kernels.py:163/:384).  Copies one int to the host and
 * synchronises `stream`. */
int gpode_cache_info(const float* ws, int* host_info, void* stream);
/* Conditioning estimate of the draw's factor(s): host_min_max[0] / [1] = the smallest / largest diagonal entry of L
 * (K_uu + jitter I = L L^T, kernels.py:163 / :384); their ratio squared bounds cond(K_uu) from below.  Synchronises `stream`. */
int gpode_cache_pivots(const float* ws, float* host_min_max, void* stream);
/* Route of gpode_cache_build_bwd through the factor (the autograd of kernels.py:163-171 / :384-386): 0 auto (triangular solves up
 * to 192 rows, an explicit triangular inverse beyond), 1 always triangular solves (up to 1216 rows; slower, and as accurate as
 * torch's fp32 solves on a numerically rank-deficient K_uu, where the explicit inverse is not), 2 never.  Process-wide. */
int gpode_set_backward_solves(int mode);

/* kern.K(X, X2) (kernels.py:98-110 / :289-303), no jitter.  X (N,Di), X2 (M2,Di).
 * RBF: out (Do,N,M2).  DF: out (N*D, M2*D), row (n,a), col (m,b). */
int gpode_kernel_matrix(int kernel, int Di, int Do, const float* raw_ell, const float* raw_var,
                        const float* X, int N, const float* X2, int M2, float* out, void* stream);

/* The kernel's own methods, for a caller that keeps its SVGP_Layer class and binds method by method -- the stages of
 * gpode_cache_build_fwd, cut where the reference cuts them:
 *   gpode_kern_cache   kern.build_cache(S, device) (kernels.py:126-137 / :305-316) with kern.sample_freq (kernels.py:112-124) inside:
 *                      omega (Di,S,Do) = rff_eps / ell^T, phase (1,S,Do) = 2 pi rff_u (either may be NULL), and in `pack` a
 *                      PRIOR-ONLY cache (no inducing records) that gpode_rhs_fwd(..., M = 0, ..., mode = 1) evaluates:
 *                      kern.rff_forward(x, S) (kernels.py:140-153 / :319-351) on exactly these Fourier features.
 *   gpode_compute_nu   kern.compute_nu(Ku, u_prior, inducing_val) (kernels.py:155-172 / :376-387): Cholesky of the CALLER's
 *                      Ku + 1e-5 I (RBF (Do,M,M); DF (M D, M D)) and nu = L^-T (u - L^-1 u_prior); u_prior, u (M,Do); nu RBF (Do,M,1),
 *                      DF (M D,1).  ws: gpode_compute_nu_ws floats; afterwards gpode_cache_info(ws) reports a non-positive-definite Ku.
 *   gpode_f_update     kern.f_update(x, x2) (kernels.py:174-181 / :390-393): out (N,Do) = K(x, x2) nu for the caller's nu and x2 (M,Di).
 * `pack` / `scratch`: gpode_kern_scratch(kernel, Di, Do, M, S) floats (M = 0 for gpode_kern_cache, S = 0 for gpode_f_update); 0 = no
 * specialisation. */
size_t gpode_kern_scratch(int kernel, int Di, int Do, int M, int S);
int gpode_kern_cache(int kernel, int Di, int Do, int S, const float* raw_ell, const float* raw_var, const float* rff_w,
                     const float* rff_eps, const float* rff_u, float* pack, float* omega, float* phase, void* stream);
int gpode_compute_nu_ws(int kernel, int Di, int Do, int M, size_t* ws_floats);
int gpode_compute_nu(int kernel, int Di, int Do, int M, const float* Ku, const float* u_prior, const float* u, float* nu, float* ws,
                     void* stream);
int gpode_f_update(int kernel, int Di, int Do, int M, const float* raw_ell, const float* raw_var, const float* x2, const float* nu,
                   const float* x, int N, float* out, float* scratch, void* stream);

/* SVGP_Layer.build_conditional (svpy.py:176-210), RBF kernel: q(f(x)) = N(m(x), Sigma(x)) at the rows of x (N,Di).
 * raw_ell (Do,Di), raw_var (Do), Z (M,Di), Um (M,Do) as in gpode_cache_build_fwd.  us_rank1 = 0: Us = the packed lower
 * triangle (Do, M(M+1)/2); us_rank1 = 1 (q_diag=True): Us = the constrained scale as (Do,M) columns s_d, and Us Us^T is the
 * rank-one s_d s_d^T the reference forms from its (M,1) column (svpy.py:194-195).
 * mean (N,Do).  full_cov = 0: var (N,Do) marginal variances; full_cov = 1: var (N,N,Do) (the layout `var.T` has in
 * svpy.py:210).  ws: gpode_conditional_ws floats of scratch (the caller allocates). */
int gpode_conditional_ws(int Di, int Do, int M, int N, size_t* ws_floats);
int gpode_conditional(int Di, int Do, int M, int N, const float* raw_ell, const float* raw_var, const float* Z,
                      const float* Um, const float* Us, int us_rank1, const float* x, int full_cov, float* mean,
                      float* var, float* ws, void* stream);

/* Posterior moments of the divergence-free layer, q(f(x)) = N(m(x), Sigma(x)) at the rows of x (N,D).  No reference line computes
 * it (svpy.py:176-210 assumes the RBF layout); this entry DEFINES it, from the sampling path (sample_inducing svpy.py:88-101,
 * compute_nu / f_update kernels.py:376-393).  With n = M D, rows and columns ordered (point, output) as kern.K orders them:
 *   L = chol(K(Z) + jitter I) (lower triangle read),  A = L^-1 K(Z,x) (n, N D),  a_j = column j = (query, b) of A viewed as (M,D),
 *   t_j[:, d] = Us_d^T a_j[:, d],   mean[query, b] = sum_{m,d} a_j[m,d] Um[m,d],
 *   cov[j, j'] = K(x,x)[j, j'] + sum_d t_j[:, d] . t_j'[:, d] - a_j . a_j'.
 * With per-entry lengthscales the DF matrix is not symmetric: K(Z,x) enters (as in f_update), not K(x,Z)^T, and K(x,x) is kern.K(x)
 * as it stands.  raw_ell (D,D), raw_var (D), Z (M,D), Um (M,D), Us_packed (D, M(M+1)/2) as in gpode_cache_build_fwd (q_diag: the
 * softplus'd scale on the packed diagonal, the q(u) that sample_inducing draws from).  mean (N,D).  cov_mode 0: var (N,D) marginal
 * variances; 1: var (N,D,D), the covariance of the D outputs at each query; 2: var (N D, N D), the full covariance in the layout
 * of kern.K(x).  D = 2 .. 16, M D <= 8192, (M + N) D <= 65408 (chunk the queries; every call refactors K(Z)).
 * ws: gpode_conditional_df_ws floats of scratch (at most 3 np^2 for np >= 64, np = the system rows (M + N) D rounded up to 32, to
 * 128 from 1024); every float the call reads it has written.  Its first word is the factorisation status (gpode_cache_info), as for
 * gpode_conditional.  gpode_last_launch(): "conditional_df: chain32" or "conditional_df: panel". */
int gpode_conditional_df_ws(int D, int M, int N, size_t* ws_floats);
int gpode_conditional_df(int D, int M, int N, const float* raw_ell, const float* raw_var, const float* Z, const float* Um,
                         const float* Us_packed, const float* x, int cov_mode, float* mean, float* var, float* ws,
                         void* stream);

/* SVGP_Layer.kl (svpy.py:144-175, q_diag=False): Um (M,Do), Us_packed (Do, M(M+1)/2) -> kl (1 float).
 * _bwd: g = d loss / d kl (1 float, device) -> dUm (M,Do), dUs (Do, M(M+1)/2). */
int gpode_svgp_kl_fwd(int M, int Do, const float* Um, const float* Us_packed, float* kl, void* stream);
int gpode_svgp_kl_bwd(int M, int Do, const float* Um, const float* Us_packed, const float* g,
                      float* dUm, float* dUs, void* stream);

/* ------------------------------------------------------------------------------------------------
 * conv VAE blocks (model/core/vae.py), NCHW fp32.  Conv geometry: x (B,Ci,H,W), w (Co,Ci,K,K), stride S,
 * padding P, y (B,Co,Ho,Wo).  nn.ConvTranspose2d(Cin_T,Cout_T) with weight (Cin_T,Cout_T,K,K) is the adjoint
 * of the convolution with Co=Cin_T, Ci=Cout_T on the SAME weight buffer:
 *   ConvTranspose2d forward   = gpode_conv2d_bwd_data(gy := its input, bias := its bias)
 *   ConvTranspose2d d/d input = gpode_conv2d_fwd(x := grad_output, bias := NULL)
 *   ConvTranspose2d d/d weight= gpode_conv2d_bwd_weight(x := grad_output, gy := its input)
 * Conv2d (vae.py:53-61) uses them under their own names. */
int gpode_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, int Co,
                     int K, int S, int P, int Ho, int Wo, void* stream);
int gpode_conv2d_bwd_data(const float* gy, const float* w, const float* bias, float* gx, int B, int Ci, int H, int W, int Co,
                          int K, int S, int P, int Ho, int Wo, void* stream);
/* The same with the BatchNorm + ReLU that precedes the ConvTranspose2d folded into its input staging: gy is the RAW output of the
 * previous layer, gy_bn its per-channel table {mean, invstd, gamma, beta} from gpode_bn_stats; the normalised activation is
 * never written to memory (vae.py:113-120: ConvTranspose2d -> BatchNorm2d -> ReLU -> ConvTranspose2d).  Matrix-core
 * specialisations only (decnn.1/4/7/10, cnn.6): other geometries return an error, and so does every call -- this one,
 * gpode_conv2d_bwd_weight_bn and gpode_convT_fwd_stats alike -- under GPODE_CONV_VALU=1 or with an operand (gy, gy_bn, w, gx) that
 * is not 16-byte aligned; nothing is written then.  Without a table and without statistics, such a call runs on the VALU / generic
 * kernels. */
int gpode_conv2d_bwd_data_bn(const float* gy, const float* gy_bn, const float* w, const float* bias, float* gx, int B, int Ci, int H,
                             int W, int Co, int K, int S, int P, int Ho, int Wo, void* stream);
/* gpode_conv2d_fwd / gpode_conv2d_bwd_weight on a BATCH-STRIDED input: image b starts x_batch_stride floats after image b - 1 and is
 * dense in itself -- the encoder reads frame 0 (or the first frames, order 2) of every sequence of the minibatch X (N,T,1,28,28) in place
 * (odegpvae.py:55-63: `X[:, 0]`), where torch would first copy the slice.  Generic kernels only (input channels not a multiple of 4). */
int gpode_conv2d_fwd_bs(const float* x, size_t x_batch_stride, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, int Co,
                        int K, int S, int P, int Ho, int Wo, void* stream);
int gpode_conv2d_bwd_weight_bs(const float* x, size_t x_batch_stride, const float* gy, float* gw, float* gbias, float* scratch, int B, int Ci,
                               int H, int W, int Co, int K, int S, int P, int Ho, int Wo, void* stream);
/* ConvTranspose2d forward (geometry arguments as gpode_conv2d_bwd_data: the convolution it is the adjoint of; x_bn = NULL or the
 * input's BatchNorm + ReLU table as above) that ALSO produces what the nn.BatchNorm2d in training mode BEHIND it needs (vae.py:107-120:
 * ConvTranspose2d -> BatchNorm2d): batch mean / invstd of the output y, the running-statistics update (momentum; unbiased variance;
 * num_batches_tracked += 1) and the {mean, invstd, gamma, beta} table for the next gpode_conv2d_bwd_data_bn.  The sums are taken while
 * y is stored and combined in a fixed order by the last workgroup to finish: no statistics pass over y, no separate table launch.
 *   gamma, beta (C = output channels): the BatchNorm's affine parameters;  running_mean / running_var / num_batches_tracked may be NULL;
 *   scratch: gpode_convT_fwd_stats_scratch(C) floats;  slot 0..63: launches that may run concurrently need different slots.
 * Matrix-core specialisations only (decnn.1/4/7); other geometries return an error. */
size_t gpode_convT_fwd_stats_scratch(int Cout);
int gpode_convT_fwd_stats(const float* x, const float* x_bn, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, int Co,
                          int K, int S, int P, int Ho, int Wo, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                          float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table,
                          float* scratch, int slot, void* stream);
size_t gpode_conv_wgrad_scratch(int B, int Ci, int Co, int K);
int gpode_conv2d_bwd_weight(const float* x, const float* gy, float* gw, float* gbias, float* scratch, int B, int Ci, int H, int W,
                            int Co, int K, int S, int P, int Ho, int Wo, void* stream);
int gpode_conv2d_bwd_weight_bn(const float* x, const float* gy, const float* gy_bn, float* gw, float* gbias, float* scratch, int B, int Ci,
                               int H, int W, int Co, int K, int S, int P, int Ho, int Wo, void* stream);
/* nn.BatchNorm2d in TRAINING mode (batch statistics), optional fused ReLU (vae.py:55-59,113-120).
 * running_* may be NULL (no update); num_batches_tracked (optional, DEVICE int64 scalar, the module buffer) is incremented.
 * gx_chansum (optional, C floats): per-channel sum of gx, i.e. the bias gradient of the
 * convolution that feeds this BatchNorm, produced while gx is written instead of by a separate pass.
 * gpode_bn_fwd and gpode_bn_stats refuse B * HW < 2 ("Expected more than 1 value per channel when training", as nn.BatchNorm2d:
 * the unbiased variance of one value does not exist) and write nothing; gpode_bn_moments accepts a one-element shard. */
size_t gpode_bn_scratch(int B, int C);
int gpode_bn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_invstd,
                 float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, int B, int C,
                 int HW, int relu, float* scratch, void* stream);
int gpode_bn_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                 const float* save_invstd, float* gx, float* ggamma, float* gbeta, float* gx_chansum, int B, int C, int HW,
                 int relu, float* scratch, void* stream);
/* Training-mode statistics WITHOUT the output pass: save_mean / save_invstd / running statistics / counter as gpode_bn_fwd, plus
 * table[C][4] = {mean, invstd, gamma, beta} for a consumer that applies the normalisation itself (gpode_conv2d_bwd_*_bn).
 * Backward: gpode_bn_bwd as usual (it needs x, not y). */
int gpode_bn_stats(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd, float* running_mean,
                   float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table, int B, int C, int HW,
                   float* scratch, void* stream);
/* BatchNorm across ranks (data parallelism): the reference's training-mode BatchNorm normalises with the statistics of
 * the WHOLE minibatch (vae.py:55,58,113,116,119).  The layer is split where the ranks exchange <= 2C+1 floats; the library does no
 * communication itself (the host all-gathers with RCCL):
 *   forward   gpode_bn_moments   this shard's per-channel {mean, M2 = sum (x - mean)^2} and its element count, moments[2C+1]
 *             (all-gather moments over the W ranks -> gathered[W][2C+1])
 *             gpode_bn_finalize  rank-ordered combination (Chan et al.), save_mean / save_invstd / running statistics / counter,
 *                                table[C][4] = {mean, invstd, gamma, beta}
 *             gpode_bn_apply     y = relu?(affine(x)) from the table -- or hand the table to gpode_conv2d_bwd_*_bn instead
 *   backward  gpode_bn_bwd_sums  this shard's {sum g, sum g xhat} (g = gy under the ReLU mask), sums[2C]
 *             (all-gather sums -> sums_gathered[W][2C])
 *             gpode_bn_bwd_apply gx with the centring terms sum_r weights[r] sums_gathered[r] / count_all, where weights[r] =
 *                                (rank r's share of the global batch) / (this rank's share) -- the data-parallel gradient average
 *                                weights every rank's loss by its share -- and count_all the global element count; ggamma / gbeta
 *                                stay this shard's sums.  Must be given the scratch gpode_bn_bwd_sums just used. */
int gpode_bn_moments(const float* x, float* moments, int B, int C, int HW, float* scratch, void* stream);
int gpode_bn_finalize(const float* gathered, int nranks, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                      float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table,
                      int C, void* stream);
int gpode_bn_apply(const float* x, const float* table, float* y, int B, int C, int HW, int relu, void* stream);
int gpode_bn_bwd_sums(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_invstd, float* sums, int B, int C, int HW, int relu, float* scratch, void* stream);
int gpode_bn_bwd_apply(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                       const float* save_invstd, const float* sums_gathered, const float* weights, int nranks, float count_all,
                       float* gx, float* ggamma, float* gbeta, float* gx_chansum, int B, int C, int HW, int relu, float* scratch,
                       void* stream);
/* Deferred final reductions.  The backward entry points that end in "sum the partials of nsplit workgroups" (gpode_conv2d_bwd_weight*,
 * gpode_bn_bwd, gpode_bn_bwd_apply, gpode_dec10_bn_bwd_apply, gpode_chan_sum) launch that last step themselves -- unless the call is
 * made between gpode_defer_reductions(1) and gpode_defer_reductions(0): then it is recorded (the caller keeps the scratch buffer alive)
 * and gpode_flush_reductions(stream) runs everything recorded so far in ONE launch; their outputs are valid after that.  This is what
 * autograd's end-of-backward hook of the host mirror does (10-15 launches of a few microseconds of work become one graph node).
 * mode 2 = drop what an aborted backward pass left behind, then as mode 1.  At most 24 pending jobs (further ones launch at once). */
void gpode_defer_reductions(int mode);
int gpode_flush_reductions(void* stream);
/* The decoder's last stage backward, fused: decnn.10 = ConvTranspose2d(16 -> 1, 5, stride 1, padding 2) on 28 x 28 (vae.py:121) fed by
 * ReLU(BatchNorm2d(16)) (vae.py:119-120).  The gradient w.r.t. the normalised activation (25 multiply-adds per element from one
 * 3 KB plane of gy) is recomputed inside both BatchNorm backward passes instead of being written once and read twice:
 *   gpode_dec10_bn_bwd_sums   this shard's {sum g, sum g xhat} (partials stay in scratch; sums[32] too unless NULL)
 *   gpode_dec10_bn_bwd_apply  gc = d loss / d c (c = the BatchNorm's input, B x 16 x 28 x 28), ggamma, gbeta, and the channel sums of gc
 *                             (gc_chansum, may be NULL).  sums_gathered == NULL: statistics of this rank alone; otherwise as
 *                             gpode_bn_bwd_apply.  Must be given the scratch gpode_dec10_bn_bwd_sums just used.
 * c: the BatchNorm input, gy: B x 1 x 28 x 28, w: decnn.10's weight [16][1][5][5]; scratch: gpode_dec10_bn_scratch_floats() floats.
 * Replaces gpode_conv2d_fwd (as the d/d input of decnn.10) + gpode_bn_bwd / gpode_bn_bwd_sums + gpode_bn_bwd_apply for this stage. */
/* gpode_dec10_bn_bwd_sums_wgrad: the sums pass that also produces decnn.10's WEIGHT gradient gw [16][1][5][5] (what
 * gpode_conv2d_bwd_weight_bn computes for this stage in a pass of its own over c) and, unless gbias is NULL, its BIAS gradient gbias[1] =
 * sum gy (gpode_chan_sum): both read c and the gy plane in the same lane layout.  wscratch: gpode_dec10_bn_wgrad_scratch_floats()
 * floats.  The final reductions of gw / gbias obey gpode_defer_reductions like the others. */
int gpode_dec10_bn_wgrad_scratch_floats(void);
int gpode_dec10_bn_bwd_sums_wgrad(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* save_mean,
                                  const float* save_invstd, float* sums, float* gw, float* gbias, int B, float* scratch, float* wscratch,
                                  void* stream);
int gpode_dec10_bn_scratch_floats(void);
int gpode_dec10_bn_bwd_sums(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, float* sums, int B, float* scratch, void* stream);
int gpode_dec10_bn_bwd_apply(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* save_mean,
                             const float* save_invstd, const float* sums_gathered, const float* weights, int nranks, float count_all,
                             float* gc, float* ggamma, float* gbeta, float* gc_chansum, int B, float* scratch, void* stream);
/* nn.BatchNorm2d in EVALUATION mode (running statistics; main.py:157-163 puts the pre-trained VAE in eval()).
 * gy == NULL: out = y = relu?(affine(x)); gy != NULL: out = d/dx (frozen layer: no affine gradients). */
int gpode_bn_eval(const float* x, const float* gy, const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, float* out, int B, int C, int HW, int relu, void* stream);
/* Evaluation-mode BatchNorm as a table: table[C][4] = {running_mean, rsqrtf(running_var + eps), gamma, beta}, the layout
 * gpode_bn_stats writes, so gpode_conv2d_bwd_data_bn runs a frozen decoder (the notebooks' `odegpvae.eval()`,
 * plots_dynamics.ipynb cell 13; create_plots.py:19-23) without materialising the normalised activations.  The inverse standard
 * deviation is formed as gpode_bn_eval forms it.  Reads the module's buffers and writes none of them. */
int gpode_bn_eval_table(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* table,
                        int C, void* stream);
/* The decoder's last stage on a frozen decoder fused with the posterior-predictive statistics (plots_dynamics.ipynb cell 13,
 * compute_mse_std: `Xrec = sigmoid(decnn.10(...))`, `se = (Xrec - X) ** 2`, `torch.mean(se)`, `torch.std(se)`; and the mean / variance
 * of Xrec over the draws).  c: raw decnn.7 output of Lc x F images of 16 x 28 x 28 floats laid out (draw, frame), F = N * Th frames;
 * table: decnn.8's {mean, invstd, gamma, beta}; w, bias: decnn.10; X: targets (N, T_obs, 1, 28, 28), frame n * Th + t has one iff
 * t < T_obs (T_obs <= Th).  State, updated in place, neither logits nor reconstructions are written:
 *   pred_mean, pred_m2 [F][784]  Welford mean / M2 of sigmoid(logit) over the draws (both may be NULL)
 *   se_state [F][3]              {count, mean, M2} of the squared error over draws and pixels of the frame
 *   done                         draws already folded into the state (0: the state is initialised, not read)
 * Deterministic: the draws of a frame are folded in order by one workgroup, so any split of the draws over launches gives the same
 * bits as one launch.  The F frame states are combined on the host in double precision (evaluate.merge_states). */
int gpode_dec10_predict(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                        int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, void* stream);
/* gpode_dec10_predict, which also leaves the held-out Bernoulli log-likelihood of every decoded image against its target -- the
 * likelihood of vae.py:136-153 (`log(z) * x + log(1 - z) * (1 - x)` summed over the pixels), the term create_model.py:52-53 averages
 * over draws and sequences.  With a = the logit of decnn.10 and x = the target as it is (not confined to [0,1]):
 *   ell[(done + l) * F + f] = sum_p  x * a - softplus(a),   softplus(a) = max(a, 0) + log1p(exp(-|a|)),
 * which equals the reference's expression in exact arithmetic (log z = a - softplus(a), log(1 - z) = -softplus(a)) and is finite for
 * every finite logit; the reference's float32 form is -inf / nan once 1 - z rounds to 0.  Frames without a target (t >= T_obs) get 0.
 * ell: [L_total][F], rows done .. done + Lc - 1 are written, every entry exactly once from one image only, so any split of the draws
 * over launches gives the same bits.  pred_mean, pred_m2 and se_state are updated to the same bits as by gpode_dec10_predict.
 * Refused, with nothing written: ell == NULL, done + Lc > L_total, every argument gpode_dec10_predict refuses, GPODE_CONV_VALU. */
int gpode_dec10_predict_ll(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                           int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, float* ell, int L_total, void* stream);
/* gpode_dec10_predict and gpode_dec10_predict_ll for ragged sequences: n_obs[N] (int32, device) is the frame count of every sequence,
 * X stays (N, T_obs, 1, 28, 28) with T_obs the padded width, and frame n * Th + t has a target iff t < min(T_obs, n_obs[n]).  A frame
 * without one is treated as a forecast frame t >= T_obs: count 0 in se_state, 0 in ell, and what its padded target holds is never
 * loaded; pred_mean / pred_m2 do not depend on n_obs.  Frames with a target get the twin's bits, n_obs[n] >= T_obs for all n gives the
 * twin's bits everywhere, and a split of the draws over launches gives the bits of one launch.  gpode_last_launch(): the twin's tag
 * + "_len".  Refused, with nothing written: n_obs == NULL and every argument the twin refuses. */
int gpode_dec10_predict_len(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                            int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, const int* n_obs, void* stream);
int gpode_dec10_predict_ll_len(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                               int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, float* ell, int L_total,
                               const int* n_obs, void* stream);
/* gpode_dec10_predict with a log-weight per (draw, sequence): the self-normalised importance-weighted predictive moments behind a
 * forecast conditioned on an observed prefix (evaluate.predict_conditional).  c, table, w, bias, X, Lc, F, Th, T_obs, done as
 * in gpode_dec10_predict; neither logits nor reconstructions are written.
 *   logw [L_total][N]            log-weight of draw l for sequence n (F = N * Th); rows done .. done + Lc - 1 are read.  -inf: weight 0.
 *                                A NaN is the caller's to refuse (the kernel does not look for one).
 *   wstate [F][2]                {ref, W}: the largest log-weight folded so far and W = sum_l exp(logw_l - ref)
 *   pred_mean, pred_m2 [F][784]  weighted mean and weighted M2 of sigmoid(logit) over the draws under the weights exp(logw_l - ref)
 *                                (West's update: W += u; d = x - mean; mean += (u / W) d; M2 += u d (x - mean)); the variance of the
 *                                weighted mixture is M2 / W
 *   wse [F]                      sum_l exp(logw_l - ref) mean_p (sigmoid(a_lp) - X_p)^2 for a frame with a target (wse / W is its
 *                                weighted per-image MSE), 0 for a frame without one, whose padded target is never loaded
 *   n_obs [N] or NULL            NULL: every frame t < T_obs has a target; otherwise as gpode_dec10_predict_len
 * A draw whose log-weight exceeds ref multiplies W, M2 and wse by exp(ref - logw) and moves ref (the mean is left alone); this happens
 * per draw, so any split of the draws over launches gives the bits of one launch.  A draw whose weight exp(logw - ref) underflows to 0
 * leaves the state bit for bit as it was.  done == 0: the state is initialised, not read.  All weights 0: W = 0, mean = M2 = 0.
 * gpode_last_launch(): the twin's tag + "_w".  Refused, with nothing written: logw == NULL, wstate == NULL, another null operand,
 * N < 1 or F != N * Th, done + Lc > L_total, every argument gpode_dec10_predict refuses, GPODE_CONV_VALU. */
int gpode_dec10_predict_w(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                          int T_obs, int done, const float* logw, int L_total, int N, float* wstate, float* pred_mean, float* pred_m2,
                          float* wse, const int* n_obs, void* stream);
/* out[c] = sum_{b,hw} v[b,c,hw] (bias gradients); scratch: gpode_bn_scratch(B,C) floats. */
int gpode_chan_sum(const float* v, float* out, int B, int C, int HW, float* scratch, void* stream);
/* mode 0: ReLU, 1: sigmoid (vae.py:60,121).  Backward takes the forward OUTPUT y. */
int gpode_act_fwd(const float* x, float* y, size_t n, int mode, void* stream);
int gpode_act_bwd(const float* y, const float* gy, float* gx, size_t n, int mode, void* stream);
/* nn.Linear (vae.py:64,107): x (B,In), w (Out,In).  scratch: gpode_linear_bwd_scratch(B, In, Out) floats, or NULL (the weight
 * gradient of a narrow, tall layer -- the decoder's fc at thousands of rows -- is then summed without row slabs, ~3x slower).
 * Each of gx, gw, gb may be NULL: that gradient is not computed, the others are (gb without gw included). */
int gpode_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, void* stream);
size_t gpode_linear_bwd_scratch(int B, int In, int Out);
int gpode_linear_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out,
                     float* scratch, void* stream);
/* nn.Linear on relu(x) with the ReLU folded into the layer (the encoder's Conv2d -> ReLU -> Flatten -> Linear, vae.py:58-61, 72-74): x is
 * the RAW convolution output (B, In); forward y = relu(x) W^T + b, backward gx = (x > 0) (gy W), gw = gy^T relu(x), gb = sum gy.  No
 * activation tensor and no ReLU launches in either direction.  Wide fan-in (In >= 128) only; other shapes return an error. */
int gpode_linear_relu_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, void* stream);
int gpode_linear_relu_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out,
                          void* stream);

/* Decoder.log_prob (vae.py:136-153): ll = log(z) X + log(1-z)(1-X), X broadcast over the leading L copies
 * (nX = numel(X)).  rowsum: the sum([2,3,4,5]) of create_model.py:52-53 fused, rows = L*N, inner = T*C*H*W. */
int gpode_loglik_fwd(const float* X, const float* z, float* ll, size_t n, size_t nX, void* stream);
int gpode_loglik_bwd(const float* X, const float* z, const float* g, float* gz, size_t n, size_t nX, void* stream);
int gpode_loglik_rowsum_fwd(const float* X, const float* z, float* out, size_t rows, size_t inner, size_t nX, void* stream);
int gpode_loglik_rowsum_bwd(const float* X, const float* z, const float* grow, float* gz, size_t rows, size_t inner, size_t nX,
                            void* stream);

/* The row sum and its adjoint for ragged sequences (the separate-kernel form of the *_len entries below, and their A/B reference): a row
 * is T frames of `frame` elements, sequence n = row % (nX / inner) owns the frames t < n_obs[n].  out[row] sums the observed terms only;
 * gz = 0 on padded elements, whose X and z are not read.  Refusals and tags as described below. */
int gpode_loglik_rowsum_fwd_len(const float* X, const float* z, float* out, size_t rows, size_t inner, size_t nX, const int* n_obs, int T,
                                size_t frame, void* stream);
int gpode_loglik_rowsum_bwd_len(const float* X, const float* z, const float* grow, float* gz, size_t rows, size_t inner, size_t nX,
                                const int* n_obs, int T, size_t frame, void* stream);

/* The last two stages of the training step's forward pass, fused (and their adjoints):
 *   gpode_sigmoid_loglik_fwd  z = sigmoid(a) (vae.py:84, the decoder's nn.Sigmoid) and the Bernoulli log-likelihood of X under z
 *                             (vae.py:136-153) summed per row as create_model.py:49 sums it; every row is cut into nsplit slices,
 *                             part[row][split] (gpode_sigmoid_loglik_splits(rows, inner) proposes nsplit).  X (nX floats) is broadcast
 *                             over the rows * inner / nX copies of it.  Same arithmetic as gpode_act_fwd + gpode_loglik_rowsum_fwd.
 *   gpode_sigmoid_loglik_bwd  ga = grow[row] * d/da, the chain gpode_loglik_rowsum_bwd -> gpode_act_bwd in one pass
 *   gpode_elbo_all_fwd        out[0..3] = {loss, -mean lhood, mean kl, kl_u} (out: 4 + 256 floats, the tail is scratch for the
 *                             sum over a big Us) (create_model.py:61-73) from the nl_values partial sums
 *                             of nl_rows likelihood rows, the encoder's rows hs = (mu | logvar), N x 2q (hv: the velocity half of a
 *                             second-order model, or NULL) -- KL(q(z0) || N(0, I)), create_model.py:47-49 -- and the inducing
 *                             posterior (Um M x Do, Us packed lower triangles Do x M(M+1)/2) -- KL(q(u) || N(0, I)), svpy.py:144-175
 *   gpode_elbo_all_bwd        gradients of the four outputs (device scalars, NULL = 0) -> glrow[nl_rows], ghs / ghv (N x 2q), dUm, dUs */
int gpode_sigmoid_loglik_splits(size_t rows, size_t inner);
int gpode_sigmoid_loglik_fwd(const float* X, const float* a, float* z, float* part, size_t rows, size_t inner, size_t nX, int nsplit,
                             void* stream);
int gpode_sigmoid_loglik_bwd(const float* X, const float* z, const float* grow, float* ga, size_t rows, size_t inner, size_t nX,
                             void* stream);
int gpode_elbo_all_fwd(const float* lpart, int nl_rows, int nl_values, const float* hs, const float* hv, int N, int q, int M, int Do,
                       const float* Um, const float* Us, float nobs, float* out, void* stream);
int gpode_elbo_all_bwd(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, const float* hs,
                       const float* hv, int N, int q, int M, int Do, const float* Um, const float* Us, float nobs, float* glrow, float* ghs,
                       float* ghv, float* dUm, float* dUs, void* stream);
/* gpode_elbo_all_bwd and gpode_sigmoid_loglik_bwd in one launch: every likelihood row receives the same gradient, so the gradient of the
 * decoder's logits (ga, n_logits values; X of nX values is broadcast over the Monte-Carlo copies) is produced together with the others. */
int gpode_elbo_all_bwd_ll(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, const float* hs,
                          const float* hv, int N, int q, int M, int Do, const float* Um, const float* Us, float nobs, float* glrow, float* ghs,
                          float* ghv, float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX,
                          void* stream);
/* Ragged minibatches: the loss stage with a frame count per sequence.  A ragged minibatch is a padded one -- X (N,T,...), n_obs[N]
 * (int32, device); rows are (draw, sequence), sequence n = row % N with N = nX / inner, frame t = p / frame for offset p inside the row
 * (`frame` = elements per frame, inner = T * frame), and frame t of sequence n is observed iff t < n_obs[n] (<= 0: none, >= T: all).
 * Each entry takes its twin's arguments plus n_obs, T and frame:
 *   gpode_sigmoid_loglik_fwd_len  z is written for every element with the twin's bits; part[row][split] sums the observed terms only
 *                                 (a row without a frame gives exactly 0).  The 16-byte path is taken only when frame % 4 == 0.
 *   gpode_sigmoid_loglik_bwd_len, gpode_elbo_all_bwd_ll_len, gpode_elbo_all_bwd_ll_kl_len
 *                                 ga = 0 on padded elements, whose X and z are not read; the twin's expression on observed ones; every
 *                                 other output of the two fused launches is the twin's, bit for bit.
 * The mask is a select, not a multiply: NaN or Inf in a padded target or logit reaches no sum and no gradient.  With n_obs[n] >= T for
 * all n every output has the twin's bits.  The KL terms have no mask: gpode_elbo_all_fwd / _fwd_kl serve both.  gpode_last_launch():
 * the twin's tag + "_len".  Refused, with nothing written: n_obs == NULL, inner != T * frame, nX % inner != 0, and what the twin refuses. */
int gpode_sigmoid_loglik_fwd_len(const float* X, const float* a, float* z, float* part, size_t rows, size_t inner, size_t nX, int nsplit,
                                 const int* n_obs, int T, size_t frame, void* stream);
int gpode_sigmoid_loglik_bwd_len(const float* X, const float* z, const float* grow, float* ga, size_t rows, size_t inner, size_t nX,
                                 const int* n_obs, int T, size_t frame, void* stream);
int gpode_elbo_all_bwd_ll_len(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, const float* hs,
                              const float* hv, int N, int q, int M, int Do, const float* Um, const float* Us, float nobs, float* glrow, float* ghs,
                              float* ghv, float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX,
                              const int* n_obs, int T, size_t frame, void* stream);
/* Ragged minibatches, compact route: the padded frames are taken out IN FRONT of the decoder, which then decodes the observed frames
 * only (what the *_len entries above mask out of the likelihood is here never decoded, and never enters a BatchNorm statistic).
 * The index (vae_ops.frame_index builds it on the host): c[n] = clamp(n_obs[n], 0, T); off[N + 1] (int32, device) the exclusive prefix
 * sum of c, off[N] = P; src[P] (int32, device), src[j] = n T + t for compact image j = off[n] + t, t < c[n].  The compact batch of L
 * draws is (L P, ...), ordered (l, n, t): the padded order with the padded frames removed; with full lengths it IS the padded batch.
 *   gpode_gather_frames_fwd      out[(l P + j), 0..q) = zt[l, src[j] / T, src[j] % T, 0..q) for zt (L,N,T,ld): replaces the position slice
 *                                + .contiguous() in front of Decoder.forward (odegpvae.py:18-35); ld >= q is the row stride of zt
 *                                (order * q), so the position slice of a second-order model is folded in.
 *   gpode_gather_frames_bwd      its adjoint written as a gather: EVERY element of gzt (L,N,T,ld) exactly once -- observed rows, columns
 *                                < q: the matching element of gout (L P, q); padded rows and columns >= q: zero.  No pre-fill, no atomics.
 *   gpode_sigmoid_loglik_fwd_pk  gpode_sigmoid_loglik_fwd over compact logits: rows are (draw, sequence), row (l, n) is the c[n] frame
 *                                contiguous logits at (l P + off[n]) frame, its targets the leading c[n] frames of X + n T frame (padded
 *                                targets are never addressed).  z is written for the L P frame compact elements; part is (rows, nsplit)
 *                                with the twin's slices (nsplit from gpode_sigmoid_loglik_splits(rows, T frame)); a slice beyond its
 *                                row's length, and so every slice of a row with c[n] = 0, is exactly 0.  With c[n] = T for all n, z and
 *                                part have the bits of gpode_sigmoid_loglik_fwd.  rows = L N with N = nX / (T frame).
 *   gpode_sigmoid_loglik_bwd_pk  gpode_sigmoid_loglik_bwd over the compact elements: ga[e] from z[e], the target at
 *                                src[j] frame + e % frame (image e / frame = l P + j) and grow[l N + src[j] / T].
 * gpode_elbo_all_fwd / _fwd_kl and gpode_elbo_all_bwd serve unchanged (nl_rows = L N).  gpode_last_launch(): "gather_frames_fwd",
 * "gather_frames_bwd", "sigmoid_loglik_fwd_pk", "sigmoid_loglik_bwd_pk".  Refused, with nothing written: a NULL index or operand,
 * q > ld, non-positive sizes, P > N T, frame % 4 != 0, nX no whole number of sequences, rows no multiple of N, and what the twins refuse. */
int gpode_gather_frames_fwd(const float* zt, int ld, int q, const int* src, int L, int N, int T, int P, float* out, void* stream);
int gpode_gather_frames_bwd(const float* gout, int ld, int q, const int* src, const int* off, int L, int N, int T, int P, float* gzt,
                            void* stream);
int gpode_sigmoid_loglik_fwd_pk(const float* X, const float* a, float* z, float* part, size_t rows, const int* off, int T, size_t frame,
                                size_t nX, int nsplit, void* stream);
int gpode_sigmoid_loglik_bwd_pk(const float* X, const float* z, const float* grow, float* ga, size_t rows, const int* src, int P, int T,
                                size_t frame, size_t nX, void* stream);
/* All device-side noise of a step in one launch (the reference draws on the host with numpy -- kernels.py:13-26,134-137,
 * svpy.py:12-27,94 -- and with torch.randn_like, vae.py:76; `--device_noise` / DeviceNoise draws here instead):
 *   out[0 .. n_normal) ~ N(0,1), out[n_normal .. n_normal + n_uniform) ~ U[0,1): Philox4x32-10 keyed by `seed`, counter = (element
 *   quad, draw number).  state: two 64-bit words in device memory {draw number, 0}; the kernel advances the draw number itself,
 *   so a captured launch yields fresh numbers at every replay and equal (seed, state) give equal numbers on every rank. */
int gpode_noise_fill(float* out, long long n_normal, long long n_uniform, unsigned long long seed, unsigned long long* state, void* stream);
/* ELBO glue on (N,q)-sized tensors (one launch each):
 *   mu / logvar are (N,q) with row stride ld (ld = 2q: the two halves of the encoder's fc output, vae.py:74), gradients
 *   are written with row stride ldg;
 *   reparameterisation z = mu + exp(logvar/2) eps (vae.py:75-78) and its backward;
 *   klrow[n] = sum_d KL(N(mu, exp(logvar/2)) || N(0,1)) (create_model.py:47-49, torch.distributions closed form) and its backward;
 *   out[4] = {loss = -(mean(lhood) nobs - mean(klrow) nobs - kl_u), -mean(lhood), mean(klrow), kl_u} (create_model.py:61-73);
 *   backward: gout[4] (gradients of the four outputs) -> glhood[nl], gklrow[nk], gklu[1]. */
/* The KL(q(z0) || N(0, I)) term riding with the reparameterisation (create_model.py:47-49 next to vae.py:75-78): gpode_reparam_kl_fwd
 * writes z and klpart[ceil(N q / 256)] = partial sums of the KL terms, which gpode_elbo_all_fwd_kl adds up in place of the packed
 * (mu | logvar) rows of gpode_elbo_all_fwd (klv / nkv: the velocity encoder's partials of a second-order model, or NULL / 0);
 * gpode_elbo_all_bwd_ll_kl returns the (uniform) gradient of every partial sum, and gpode_reparam_kl_bwd writes the gradients of
 * (mu, logvar) through z AND through the KL sum in one pass -- no second gradient tensor for autograd to add. */
int gpode_reparam_kl_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, float* klpart, int N, int q, void* stream);
int gpode_reparam_kl_bwd(const float* gz, const float* gklpart, const float* mu, const float* logvar, int ld, const float* eps, float* gmu,
                         float* glogvar, int ldg, int N, int q, void* stream);
int gpode_elbo_all_fwd_kl(const float* lpart, int nl_rows, int nl_values, const float* kls, int nks, const float* klv, int nkv, int N, int M,
                          int Do, const float* Um, const float* Us, float nobs, float* out, void* stream);
int gpode_elbo_all_bwd_ll_kl(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, int N, int M, int Do,
                             const float* Um, const float* Us, float nobs, float* glrow, float* gkls, int nks, float* gklv, int nkv,
                             float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX, void* stream);
/* gpode_elbo_all_bwd_ll_kl for ragged minibatches (see gpode_sigmoid_loglik_fwd_len) */
int gpode_elbo_all_bwd_ll_kl_len(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, int N, int M,
                                 int Do, const float* Um, const float* Us, float nobs, float* glrow, float* gkls, int nks, float* gklv, int nkv,
                                 float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX,
                                 const int* n_obs, int T, size_t frame, void* stream);
int gpode_reparam_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int N, int q, void* stream);
/* L reparameterised draws of one encoder distribution and their importance log-weights (forward only; evaluation):
 *   z[l,n,i]  = mu[n,i] + exp(logvar[n,i] / 2) eps[l,n,i]   -- the bits gpode_reparam_fwd gives for (mu, logvar, eps[l]) --
 *               written at z + (l N + n) ldz + i: ldz >= q, so the caller can point z at one half of an order-2 state
 *   lw[l,n] (+)= sum_i (eps^2 / 2 - z^2 / 2 + logvar / 2) = log N(z; 0, I) - log N(z; mu, sigma^2)   (the 2 pi terms cancel)
 * mu, logvar (N,q) with row stride ld; eps (L,N,q) dense; lw (L,N).  accumulate = 0 writes lw, 1 adds to it (the velocity
 * encoder's half of an order-2 state).  One lane per (l,n) row sums i = 0 .. q-1 in that order: no atomics, the same bits
 * every run. */
int gpode_reparam_draws_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int ldz, float* lw,
                            int accumulate, int L, int N, int q, void* stream);
/* The adjoint of gpode_reparam_draws_fwd (training on the importance-weighted bound below): gz (K,N,.) with row stride ldgz >= q -- one
 * half of an order-2 state gradient is read in place -- and glw (K,N); either may be NULL, meaning zero.  With sigma = exp(logvar / 2)
 * and z = mu + sigma eps:
 *   gmu[n,i]     = sum_k ( gz - glw z )
 *   glogvar[n,i] = sum_k ( gz sigma eps / 2 + glw (1/2 - z sigma eps / 2) )
 * written with row stride ldg.  One lane per (n,i) sums k = 0 .. K-1 in that order: no atomics, the same bits every run.
 * gpode_last_launch(): "reparam_draws_bwd".  Refused, with nothing written: a NULL mu, logvar, eps, gmu or glogvar, K outside 1..64,
 * N < 1, q < 1, a stride below q. */
int gpode_reparam_draws_bwd(const float* gz, int ldgz, const float* glw, const float* mu, const float* logvar, int ld, const float* eps,
                            float* gmu, float* glogvar, int ldg, int K, int N, int q, void* stream);
/* The importance-weighted bound over K initial-state draws per sequence, shared by the L function draws.  lpart (rows,
 * nsplit) are the partial sums of gpode_sigmoid_loglik_fwd[_len] over rows = L K N likelihood rows ordered (l,k,n) (X is broadcast by
 * row % N), lw (K,N) the log-weights of gpode_reparam_draws_fwd; Um, Us packed, M, Do, nobs as in gpode_elbo_all_fwd.  With
 * a[l,k,n] = sum_s lpart[(l,k,n)][s] + lw[k,n] and iw[l,n] = logsumexp_k a[l,k,n] - log K:
 *   gpode_elbo_iw_fwd     out[0..4] = {loss = -(nobs mean_{l,n} iw - kl_u), -mean iw, -mean_{k,n} lw (the Monte-Carlo KL(q(z0) || p)),
 *                         kl_u, mean_{l,n} ess}, ess = (sum_k w)^2 / sum_k w^2 with w = exp(a - max_k a); out: 5 + 256 floats, the tail is
 *                         scratch for the sum over a big Us.  One wavefront reduces a group (l,n), one lane per draw; the maximum over k is
 *                         subtracted before any exp.  gpode_last_launch(): "elbo_iw_fwd" [" (Us in parts)"].
 *   gpode_elbo_iw_bwd     seeds of the five outputs (device scalars, NULL = 0) -> grow[rows] = softmax_k(a)[l,k,n] (-g_loss nobs - g_nll)
 *                         / (L N), glw (K,N) = sum_l of the same - g_kl / (K N), dUm, dUs as gpode_elbo_all_bwd.  The ess output is a
 *                         diagnostic: g_ess is accepted and carries NO gradient.  A weight that underflows is exactly 0.  "elbo_iw_bwd".
 *   gpode_elbo_iw_bwd_ll  gpode_elbo_iw_bwd and gpode_sigmoid_loglik_bwd in one launch (every-frame route only): also
 *                         ga[e] = grow[row] (x/z - (1-x)/(1-z)) z (1-z) for the n_logits logits (whole rows; X of nX values broadcast);
 *                         every output has the bits of the two separate launches.  "elbo_iw_loglik_bwd".
 * Ragged minibatches run gpode_elbo_iw_bwd followed by gpode_sigmoid_loglik_bwd_len, which reads a gradient per row.  Fixed summation
 * orders, no atomics.  Refused, with nothing written: a NULL operand other than a seed, K outside 1..64, L, N, M or Do < 1, nsplit < 1,
 * rows != L K N, rows > 65535 (the grid of gpode_sigmoid_loglik_fwd), logits that are no whole rows or that X does not tile. */
int gpode_elbo_iw_fwd(const float* lpart, int rows, int nsplit, const float* lw, int L, int K, int N, int M, int Do, const float* Um,
                      const float* Us, float nobs, float* out, void* stream);
int gpode_elbo_iw_bwd(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, const float* g_ess, const float* lpart,
                      int rows, int nsplit, const float* lw, int L, int K, int N, int M, int Do, const float* Um, const float* Us, float nobs,
                      float* grow, float* glw, float* dUm, float* dUs, void* stream);
int gpode_elbo_iw_bwd_ll(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, const float* g_ess,
                         const float* lpart, int rows, int nsplit, const float* lw, int L, int K, int N, int M, int Do, const float* Um,
                         const float* Us, float nobs, float* grow, float* glw, float* dUm, float* dUs, const float* X, const float* z,
                         float* ga, size_t n_logits, size_t nX, void* stream);
int gpode_reparam_bwd(const float* gz, const float* logvar, int ld, const float* eps, float* gmu, float* glogvar, int ldg, int N, int q,
                      void* stream);
int gpode_normal_kl_fwd(const float* mu, const float* logvar, int ld, float* klrow, int N, int q, void* stream);
int gpode_normal_kl_bwd(const float* grow, const float* mu, const float* logvar, int ld, float* gmu, float* glogvar, int ldg, int N, int q,
                        void* stream);
int gpode_elbo_fwd(const float* lhood, int nl, const float* klrow, int nk, const float* kl_u, float nobs, float* out, void* stream);
int gpode_elbo_bwd(const float* gout, int nl, int nk, float nobs, float* glhood, float* gklrow, float* gklu, void* stream);

/* torch.optim.Adam step (main.py:194,211) over a whole parameter list in one launch.  params/grads/m1/m2:
 * DEVICE arrays of `ntensors` device pointers; offs: DEVICE array of element prefix offsets (offs[0]=0);
 * step: 1-based step count (bias correction).  step_dev (optional, DEVICE int[2] = {updates done so far, 0}): when non-NULL the
 * kernel uses step_dev[0] + 1 instead of `step` and advances step_dev[0] itself (the last workgroup to finish; step_dev[1] is its
 * ticket counter), so that a captured HIP graph of the training step replays with a live count and no separate counter launch. */
int gpode_adam_multi(void* params, void* grads, void* m1, void* m2, const long long* offs, int ntensors, long long total,
                     float lr, float beta1, float beta2, float eps, int step, int* step_dev, void* stream);

/* The data-parallel gradient bucket in one launch: flat[offs[t] + i] = grads[t][i] (same DEVICE tables as gpode_adam_multi).
 * What `loss.backward()` + DDP's bucket copy do in the reference's setting; the bucket is then all-reduced in place (RCCL)
 * and handed to gpode_adam_multi through a pointer table into it. */
int gpode_gather_multi(void* grads, const long long* offs, int ntensors, long long total, float* flat, void* stream);

#ifdef __cplusplus
}
#endif
#endif
