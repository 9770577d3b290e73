// capi.hip -- extern "C" surface of libgpode_hip.so (declared in include/gpode.h).
#include "../../include/gpode.h"
#include "gp_launch.hpp"

namespace gp {
char* error_slot() {
  static thread_local char buf[512] = {0};
  return buf;
}
const char** last_launch_slot() {
  static thread_local const char* tag = "";
  return &tag;
}
bool* force_substep_kernels() {
  static bool on = false;                            // gpode_test_substep_kernels
  return &on;
}
}  // namespace gp

extern "C" {

const char* gpode_version(void) { return "gpode-hip 0.1 (gfx950)"; }
const char* gpode_last_error(void) { return gp::error_slot(); }
const char* gpode_last_launch(void) { return *gp::last_launch_slot(); }
int gpode_supported(int kernel, int Di, int Do) { return gp::dims_supported(kernel, Di, Do); }

int gpode_cache_sizes(int kernel, int Di, int Do, int M, int S, size_t* pack_floats, size_t* ws_floats) {
  return gp::cache_sizes(kernel, Di, Do, M, S, pack_floats, ws_floats, 1);
}
int gpode_cache_sizes_n(int kernel, int Di, int Do, int M, int S, int ndraws, size_t* pack_floats, size_t* ws_floats) {
  return gp::cache_sizes(kernel, Di, Do, M, S, pack_floats, ws_floats, ndraws);
}

int gpode_cache_build_fwd_n(int kernel, int Di, int Do, int M, int S, int ndraws,
                            const float* raw_ell, const float* raw_var, const float* Z,
                            const float* Um, const float* Us_packed,
                            const float* eps_u, const float* rff_w, const float* rff_eps, const float* rff_u,
                            float* pack, float* ws,
                            float* ell, float* var, float* omega, float* phase, float* u,
                            float* Lu, float* nu, float* u_prior, void* stream) {
  if (!raw_ell || !raw_var || !Z || !Um || !Us_packed || !eps_u || !rff_w || !rff_eps || !rff_u || !pack || !ws)
    return gp::set_error("gpode_cache_build_fwd: null required pointer");
  return gp::cache_build_fwd(kernel, Di, Do, M, S, ndraws, raw_ell, raw_var, Z, Um, Us_packed, eps_u, rff_w, rff_eps, rff_u,
                             pack, ws, ell, var, omega, phase, u, Lu, nu, u_prior, (hipStream_t)stream);
}
int gpode_cache_build_fwd(int kernel, int Di, int Do, int M, int S,
                          const float* raw_ell, const float* raw_var, const float* Z,
                          const float* Um, const float* Us_packed,
                          const float* eps_u, const float* rff_w, const float* rff_eps, const float* rff_u,
                          float* pack, float* ws,
                          float* ell, float* var, float* omega, float* phase, float* u,
                          float* Lu, float* nu, float* u_prior, void* stream) {
  return gpode_cache_build_fwd_n(kernel, Di, Do, M, S, 1, raw_ell, raw_var, Z, Um, Us_packed, eps_u, rff_w, rff_eps, rff_u, pack, ws, ell, var,
                                 omega, phase, u, Lu, nu, u_prior, stream);
}

int gpode_cache_info(const float* ws, int* host_info, void* stream) {
  // copies the factorisation status word (bit 0: K_uu + jitter I not positive definite) to the host;
  // synchronises `stream`.
  hipError_t e = hipMemcpyAsync(host_info, ws, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return gp::set_error("gpode_cache_info: %s", hipGetErrorString(e));
  return 0;
}

int gpode_cache_pivots(const float* ws, float* host_min_max, void* stream) {
  // smallest and largest diagonal entry of the Cholesky factor(s) of this draw; synchronises `stream`
  hipError_t e = hipMemcpyAsync(host_min_max, ws + 1, 2 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return gp::set_error("gpode_cache_pivots: %s", hipGetErrorString(e));
  return 0;
}

int gpode_set_backward_solves(int mode) {
  if (mode < 0 || mode > 2) return gp::set_error("gpode_set_backward_solves: mode %d (0 auto, 1 always, 2 never)", mode);
  gp::set_backward_solves(mode);
  return 0;
}

int gpode_rhs_fwd(int kernel, int Di, int Do, int M, int S, const float* pack,
                  const float* x, int N, float* f, int mode, void* stream) {
  if (N < 0 || mode < 0 || mode > 2) return gp::set_error("gpode_rhs_fwd: N=%d mode=%d", N, mode);
  if (N == 0) return 0;                              // empty minibatch: nothing to do (empty tensors carry null pointers)
  if (!pack || !x || !f) return gp::set_error("gpode_rhs_fwd: null pointer");
  return gp::rhs_fwd(kernel, Di, Do, M, S, pack, x, N, f, mode, (hipStream_t)stream);
}

// ts_per_traj of the `_nt` entry points: 0 = ts (T,) shared by the trajectories, 1 = (N,T), row n for trajectory n of every draw
static int ts_flag_refused(const char* who, int ts_per_traj) {
  if (ts_per_traj == 0 || ts_per_traj == 1) return 0;
  return gp::set_error("%s: ts_per_traj=%d (0 one (T,) grid shared, 1 one row of (N,T) per trajectory)", who, ts_per_traj);
}
// z0_per_draw of the `_nz` entry points: 0 = z0 (N,D) shared by the draws, 1 = (ndraws,N,D)
static int z0_flag_refused(const char* who, int z0_per_draw) {
  if (z0_per_draw == 0 || z0_per_draw == 1) return 0;
  return gp::set_error("%s: z0_per_draw=%d (0 shared, 1 one (N,D) slab per draw)", who, z0_per_draw);
}
// substeps of the `_ns` entry points: equal solver steps per output interval, 1 (the twin's launch) ... gp::kMaxSubsteps
static int substeps_refused(const char* who, int substeps) {
  if (substeps >= 1 && substeps <= gp::kMaxSubsteps) return 0;
  return gp::set_error("%s: substeps=%d (1 ... %d steps per output interval)", who, substeps, gp::kMaxSubsteps);
}
static bool draws_ok(int ndraws) { return ndraws >= 1 && ndraws <= 65535; }   // the draws ride on gridDim.y

// The four checked operations under the gpode_rollout_* exports, which only name themselves (`who`, the entry point the error texts
// start with) and the flags their prototype lacks.  Each checks the arguments and fills the launcher's struct by member name; the
// strides and the record layout are the launcher's (gp_launch.hpp).
static int rollout_fwd_any(const char* who, int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                           const float* pack, const float* z0, const float* ts, int N, int T,
                           float* zt, float* xstage, int z0_per_draw, int ts_per_traj, int substeps, void* stream) {
  if (z0_flag_refused(who, z0_per_draw) || ts_flag_refused(who, ts_per_traj) || substeps_refused(who, substeps)) return 1;
  if (N < 0 || T < 1 || !draws_ok(ndraws)) return gp::set_error("%s: N=%d T=%d draws=%d", who, N, T, ndraws);
  if (N == 0) return 0;
  if (!pack || !z0 || !ts || !zt) return gp::set_error("%s: null pointer", who);
  const gp::RolloutFwdArgs a{.M = M, .S = S, .pack = pack, .z0 = z0, .ts = ts, .N = N, .T = T, .zt = zt, .xstage = xstage,
                             .z0_per_draw = z0_per_draw != 0, .ts_per_traj = ts_per_traj != 0, .substeps = substeps};
  return gp::rollout_fwd(kernel, order, method, Di, Do, a, ndraws, (hipStream_t)stream);
}
// slab / nchunk / gpack: the fused sweep with parameter sums (`pgrad`, which needs a step to sum over); null / 0 for the plain one
static int rollout_bwd_any(const char* who, bool pgrad, int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                           const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                           float* gz0, float* astage, float* slab, int nchunk, float* gpack, int ts_per_traj, int substeps,
                           void* stream) {
  if (ts_flag_refused(who, ts_per_traj) || substeps_refused(who, substeps)) return 1;
  if (N < (pgrad ? 1 : 0) || T < (pgrad ? 2 : 1) || !draws_ok(ndraws)) return gp::set_error("%s: N=%d T=%d draws=%d", who, N, T, ndraws);
  if (N == 0) return 0;
  if (!pack || !gzt || !ts || !gz0 || (T > 1 && (!xstage || !astage)) || (pgrad && (!slab || !gpack)))
    return gp::set_error("%s: null pointer", who);
  const gp::RolloutBwdArgs a{.M = M, .S = S, .pack = pack, .xstage = xstage, .gzt = gzt, .ts = ts, .N = N, .T = T, .gz0 = gz0,
                             .astage = astage, .ts_per_traj = ts_per_traj != 0, .substeps = substeps, .slab = slab, .nchunk = nchunk,
                             .gpack = gpack};
  return pgrad ? gp::rollout_bwd_pgrad(kernel, order, method, Di, Do, a, ndraws, (hipStream_t)stream)
               : gp::rollout_bwd(kernel, order, method, Di, Do, a, ndraws, (hipStream_t)stream);
}
// dopri5, landing (index = iend, theta unused) or dense (index = istep)
static int adaptive_fwd_any(const char* who, bool dense, int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                            const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                            float* zt, float* xstage, float* hstep, int* index, float* theta, int* counts, int z0_per_draw,
                            int ts_per_traj, void* stream) {
  if (ts_flag_refused(who, ts_per_traj) || z0_flag_refused(who, z0_per_draw)) return 1;
  if (method != GPODE_METHOD_DOPRI5) return gp::set_error("%s: method %d (3 dopri5)", who, method);
  if (N < 0 || T < 1 || K < 0 || !draws_ok(ndraws)) return gp::set_error("%s: N=%d T=%d K=%d draws=%d", who, N, T, K, ndraws);
  if (!(rtol >= 0.f) || !(atol >= 0.f) || !(rtol + atol > 0.f) || !(rtol + atol < 1e30f))
    return gp::set_error("%s: rtol=%g atol=%g (both >= 0, not both 0)", who, rtol, atol);
  if (N == 0) return 0;
  if (!pack || !z0 || !ts || !zt || !counts) return gp::set_error("%s: null pointer", who);
  if (xstage && T > 1 && (!index || (dense && !theta) || (K > 0 && !hstep)))
    return gp::set_error(dense ? "%s: xstage without hstep / istep / theta" : "%s: xstage without hstep / iend", who);
  const gp::AdaptFwdArgs a{.M = M, .S = S, .pack = pack, .z0 = z0, .ts = ts, .N = N, .T = T, .K = K, .rtol = rtol, .atol = atol,
                           .zt = zt, .xstage = xstage, .hstep = hstep, .index = index, .theta = theta, .counts = counts,
                           .z0_per_draw = z0_per_draw != 0, .ts_per_traj = ts_per_traj != 0};
  return gp::rollout_adaptive_fwd(kernel, order, Di, Do, a, dense, ndraws, (hipStream_t)stream);
}
static int adaptive_bwd_any(const char* who, bool dense, int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                            const float* pack, const float* xstage, const float* hstep, const int* index, const float* theta,
                            const float* gzt, int N, int T, int K, float* gz0, float* astage, void* stream) {
  if (method != GPODE_METHOD_DOPRI5) return gp::set_error("%s: method %d (3 dopri5)", who, method);
  if (N < 0 || T < 1 || K < 0 || !draws_ok(ndraws)) return gp::set_error("%s: N=%d T=%d K=%d draws=%d", who, N, T, K, ndraws);
  if (N == 0) return 0;
  if (!pack || !gzt || !gz0 || (T > 1 && (!index || (dense && !theta))) || (T > 1 && K > 0 && (!xstage || !hstep || !astage)))
    return gp::set_error("%s: null pointer", who);
  const gp::AdaptBwdArgs a{.M = M, .S = S, .pack = pack, .xstage = xstage, .hstep = hstep, .index = index, .theta = theta, .gzt = gzt,
                           .N = N, .T = T, .K = K, .gz0 = gz0, .astage = astage};
  return gp::rollout_adaptive_bwd(kernel, order, Di, Do, a, dense, ndraws, (hipStream_t)stream);
}

int gpode_test_substep_kernels(int on) {
  if (on != 0 && on != 1) return gp::set_error("gpode_test_substep_kernels: on=%d (0 or 1)", on);
  *gp::force_substep_kernels() = on != 0;
  return 0;
}
int gpode_rollout_bwd_pgrad_chunks(int kernel, int order, int method, int Di, int Do, int M, int S, int N) {
  return gp::rollout_bwd_pgrad_chunks(kernel, order, method, Di, Do, M, S, N);
}

// The exports: thin forwards.  An entry point without a flag passes the value its twin with the flag takes for "as before".
int gpode_rollout_fwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                        const float* pack, const float* z0, const float* ts, int N, int T,
                        float* zt, float* xstage, void* stream) {
  return rollout_fwd_any("gpode_rollout_fwd", kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, zt, xstage, 0, 0, 1, stream);
}
int gpode_rollout_fwd_nz(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* z0, const float* ts, int N, int T,
                         float* zt, float* xstage, int z0_per_draw, void* stream) {
  return rollout_fwd_any("gpode_rollout_fwd_nz", kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, zt, xstage, z0_per_draw,
                         0, 1, stream);
}
int gpode_rollout_fwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* z0, const float* ts, int N, int T,
                         float* zt, float* xstage, int z0_per_draw, int ts_per_traj, void* stream) {
  return rollout_fwd_any("gpode_rollout_fwd_nt", kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, zt, xstage, z0_per_draw,
                         ts_per_traj, 1, stream);
}
int gpode_rollout_fwd_ns(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* z0, const float* ts, int N, int T,
                         float* zt, float* xstage, int z0_per_draw, int ts_per_traj, int substeps, void* stream) {
  return rollout_fwd_any("gpode_rollout_fwd_ns", kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, zt, xstage, z0_per_draw,
                         ts_per_traj, substeps, stream);
}
int gpode_rollout_fwd(int kernel, int order, int method, int Di, int Do, int M, int S,
                      const float* pack, const float* z0, const float* ts, int N, int T,
                      float* zt, float* xstage, void* stream) {
  return gpode_rollout_fwd_n(kernel, order, method, Di, Do, M, S, 1, pack, z0, ts, N, T, zt, xstage, stream);
}

// Forward mode (gp_tangent.hip).  What the two share: the number of directions, and the widths -- checked here, so that every
// refusal comes before the first HIP call.
static int tangents_refused(const char* who, int kernel, int Di, int Do, int K, bool identity, long long rows) {
  if (identity && K != Di) return gp::set_error("%s: NULL directions are the identity and need K == Di (K=%d Di=%d)", who, K, Di);
  if (!gp::dims_supported(kernel, Di, Do)) return gp::set_error("%s: no specialisation for kernel=%d Di=%d Do=%d", who, kernel, Di, Do);
  if (rows * K > 0x7fffffffLL) return gp::set_error("%s: %lld rows x %d directions do not fit one launch", who, rows, K);
  return 0;
}
static int tangent_count_refused(const char* who, int K) {
  if (K >= 1 && K <= gp::kMaxTangents) return 0;
  return gp::set_error("%s: K=%d (1 ... %d tangent directions per row)", who, K, gp::kMaxTangents);
}

int gpode_rhs_jvp(int kernel, int Di, int Do, int M, int S, int ndraws, const float* pack,
                  const float* x, int x_per_draw, const float* v, int R, int K,
                  float* f, float* jv, int mode, void* stream) {
  static const char* const who = "gpode_rhs_jvp";
  if (mode < 0 || mode > 2) return gp::set_error("%s: mode=%d (0 full, 1 prior, 2 update)", who, mode);
  if (x_per_draw != 0 && x_per_draw != 1) return gp::set_error("%s: x_per_draw=%d (0 shared, 1 one (R,Di) slab per draw)", who, x_per_draw);
  if (R < 1 || !draws_ok(ndraws)) return gp::set_error("%s: R=%d draws=%d", who, R, ndraws);
  if (tangent_count_refused(who, K)) return 1;
  if (!pack || !x || !jv) return gp::set_error("%s: null pointer", who);
  if (tangents_refused(who, kernel, Di, Do, K, v == nullptr, R)) return 1;
  const gp::RhsJvpArgs a{.M = M, .S = S, .pack = pack, .x = x, .v = v, .R = R, .K = K, .f = f, .jv = jv, .mode = mode,
                         .x_per_draw = x_per_draw != 0};
  return gp::rhs_jvp(kernel, Di, Do, a, ndraws, (hipStream_t)stream);
}

int gpode_rollout_jvp(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws, const float* pack,
                      const float* z0, int z0_per_draw, const float* v0, int K,
                      const float* ts, int ts_per_traj, int substeps, int N, int T,
                      float* zt, float* vt, void* stream) {
  static const char* const who = "gpode_rollout_jvp";
  if (method == GPODE_METHOD_DOPRI5)
    return gp::set_error("%s: method 3 (dopri5): its steps depend on the state through the controller, and the tangent of the "
                         "accepted-step sequence is not built (0 euler, 1 rk4, 2 midpoint)", who);
  if (method < 0 || method > 2) return gp::set_error("%s: method %d (0 euler, 1 rk4, 2 midpoint)", who, method);
  if (z0_flag_refused(who, z0_per_draw) || ts_flag_refused(who, ts_per_traj) || substeps_refused(who, substeps)) return 1;
  if (N < 1 || T < 1 || !draws_ok(ndraws)) return gp::set_error("%s: N=%d T=%d draws=%d", who, N, T, ndraws);
  if (tangent_count_refused(who, K)) return 1;
  if (!pack || !z0 || !ts || !vt) return gp::set_error("%s: null pointer", who);
  if (tangents_refused(who, kernel, Di, Do, K, v0 == nullptr, N)) return 1;
  if (Di != order * Do || (order != 1 && order != 2))
    return gp::set_error("%s: order=%d needs Di == order*Do (Di=%d Do=%d)", who, order, Di, Do);
  const gp::RolloutJvpArgs a{.M = M, .S = S, .pack = pack, .z0 = z0, .v0 = v0, .K = K, .ts = ts, .N = N, .T = T, .zt = zt, .vt = vt,
                             .z0_per_draw = z0_per_draw != 0, .ts_per_traj = ts_per_traj != 0, .substeps = substeps};
  return gp::rollout_jvp(kernel, order, method, Di, Do, a, ndraws, (hipStream_t)stream);
}

int gpode_rollout_bwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                         float* gz0, float* astage, int ts_per_traj, void* stream) {
  return rollout_bwd_any("gpode_rollout_bwd", false, kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, gzt, ts, N, T, gz0, astage,
                         nullptr, 0, nullptr, ts_per_traj, 1, stream);
}
int gpode_rollout_bwd_ns(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                         const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                         float* gz0, float* astage, int ts_per_traj, int substeps, void* stream) {
  return rollout_bwd_any("gpode_rollout_bwd_ns", false, kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, gzt, ts, N, T, gz0, astage,
                         nullptr, 0, nullptr, ts_per_traj, substeps, stream);
}
int gpode_rollout_bwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                        const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                        float* gz0, float* astage, void* stream) {
  return gpode_rollout_bwd_nt(kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, gzt, ts, N, T, gz0, astage, 0, stream);
}
int gpode_rollout_bwd(int kernel, int order, int method, int Di, int Do, int M, int S,
                      const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                      float* gz0, float* astage, void* stream) {
  return gpode_rollout_bwd_n(kernel, order, method, Di, Do, M, S, 1, pack, xstage, gzt, ts, N, T, gz0, astage, stream);
}
int gpode_rollout_bwd_pgrad_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                               float* gz0, float* astage, float* slab, int nchunk, float* gpack, int ts_per_traj, void* stream) {
  return rollout_bwd_any("gpode_rollout_bwd_pgrad", true, kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, gzt, ts, N, T, gz0,
                         astage, slab, nchunk, gpack, ts_per_traj, 1, stream);
}
int gpode_rollout_bwd_pgrad_ns(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                               float* gz0, float* astage, float* slab, int nchunk, float* gpack, int ts_per_traj, int substeps,
                               void* stream) {
  return rollout_bwd_any("gpode_rollout_bwd_pgrad_ns", true, kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, gzt, ts, N, T, gz0,
                         astage, slab, nchunk, gpack, ts_per_traj, substeps, stream);
}
int gpode_rollout_bwd_pgrad_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                              const float* pack, const float* xstage, const float* gzt, const float* ts, int N, int T,
                              float* gz0, float* astage, float* slab, int nchunk, float* gpack, void* stream) {
  return gpode_rollout_bwd_pgrad_nt(kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, gzt, ts, N, T, gz0, astage, slab, nchunk,
                                    gpack, 0, stream);
}

int gpode_rollout_adaptive_fwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                 const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                                 float* zt, float* xstage, float* hstep, int* iend, int* counts, void* stream) {
  return adaptive_fwd_any("gpode_rollout_adaptive_fwd", false, kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, rtol, atol,
                          K, zt, xstage, hstep, iend, nullptr, counts, 0, 0, stream);
}
int gpode_rollout_adaptive_fwd_nz(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                  const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                                  float* zt, float* xstage, float* hstep, int* iend, int* counts, int z0_per_draw, void* stream) {
  return adaptive_fwd_any("gpode_rollout_adaptive_fwd_nz", false, kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, rtol,
                          atol, K, zt, xstage, hstep, iend, nullptr, counts, z0_per_draw, 0, stream);
}
int gpode_rollout_adaptive_fwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                  const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                                  float* zt, float* xstage, float* hstep, int* iend, int* counts, int z0_per_draw, int ts_per_traj,
                                  void* stream) {
  return adaptive_fwd_any("gpode_rollout_adaptive_fwd_nt", false, kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, rtol,
                          atol, K, zt, xstage, hstep, iend, nullptr, counts, z0_per_draw, ts_per_traj, stream);
}
int gpode_rollout_adaptive_bwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                                 const float* pack, const float* xstage, const float* hstep, const int* iend, const float* gzt,
                                 int N, int T, int K, float* gz0, float* astage, void* stream) {
  return adaptive_bwd_any("gpode_rollout_adaptive_bwd", false, kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, hstep, iend,
                          nullptr, gzt, N, T, K, gz0, astage, stream);
}
int gpode_rollout_dense_fwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                              const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                              float* zt, float* xstage, float* hstep, int* istep, float* theta, int* counts, void* stream) {
  return adaptive_fwd_any("gpode_rollout_dense_fwd", true, kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, rtol, atol, K, zt,
                          xstage, hstep, istep, theta, counts, 0, 0, stream);
}
int gpode_rollout_dense_fwd_nz(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                               float* zt, float* xstage, float* hstep, int* istep, float* theta, int* counts, int z0_per_draw,
                               void* stream) {
  return adaptive_fwd_any("gpode_rollout_dense_fwd_nz", true, kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, rtol, atol, K,
                          zt, xstage, hstep, istep, theta, counts, z0_per_draw, 0, stream);
}
int gpode_rollout_dense_fwd_nt(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                               const float* pack, const float* z0, const float* ts, int N, int T, float rtol, float atol, int K,
                               float* zt, float* xstage, float* hstep, int* istep, float* theta, int* counts, int z0_per_draw,
                               int ts_per_traj, void* stream) {
  return adaptive_fwd_any("gpode_rollout_dense_fwd_nt", true, kernel, order, method, Di, Do, M, S, ndraws, pack, z0, ts, N, T, rtol, atol, K,
                          zt, xstage, hstep, istep, theta, counts, z0_per_draw, ts_per_traj, stream);
}
int gpode_rollout_dense_bwd_n(int kernel, int order, int method, int Di, int Do, int M, int S, int ndraws,
                              const float* pack, const float* xstage, const float* hstep, const int* istep, const float* theta,
                              const float* gzt, int N, int T, int K, float* gz0, float* astage, void* stream) {
  return adaptive_bwd_any("gpode_rollout_dense_bwd", true, kernel, order, method, Di, Do, M, S, ndraws, pack, xstage, hstep, istep, theta,
                          gzt, N, T, K, gz0, astage, stream);
}

int gpode_rhs_vjp(int kernel, int Di, int Do, int M, int S, const float* pack,
                  const float* x, const float* a, int R, float* gx, void* stream) {
  if (!pack || !x || !a || !gx) return gp::set_error("gpode_rhs_vjp: null pointer");
  return gp::rhs_vjp(kernel, Di, Do, M, S, pack, x, a, R, gx, 0, (hipStream_t)stream);
}

int gpode_param_grad_n(int kernel, int Di, int Do, int M, int S, int ndraws, const float* pack,
                       const float* x, const float* a, int R, float* slab, int nchunk, float* gpack, int accumulate,
                       void* stream) {
  if (!pack || !x || !a || !slab || !gpack) return gp::set_error("gpode_param_grad: null pointer");
  if (ndraws < 1 || ndraws > 65535) return gp::set_error("gpode_param_grad: %d draws", ndraws);
  size_t pf = 0;
  if (gp::cache_sizes(kernel, Di, Do, M, S, &pf, nullptr)) return 1;
  gp::Draws d;
  d.nd = ndraws; d.pack = pf; d.in = (size_t)R * Di; d.in2 = (size_t)R * Do; d.out = pf;
  return gp::param_grad(kernel, Di, Do, M, S, pack, x, a, R, slab, nchunk, gpack, accumulate, 0, (hipStream_t)stream, d);
}
int gpode_param_grad(int kernel, int Di, int Do, int M, int S, const float* pack,
                     const float* x, const float* a, int R, float* slab, int nchunk, float* gpack, int accumulate,
                     void* stream) {
  return gpode_param_grad_n(kernel, Di, Do, M, S, 1, pack, x, a, R, slab, nchunk, gpack, accumulate, stream);
}

int gpode_kernel_matrix(int kernel, int Di, int Do, const float* raw_ell, const float* raw_var,
                        const float* X, int N, const float* X2, int M2, float* out, void* stream) {
  if (!raw_ell || !raw_var || !X || !X2 || !out) return gp::set_error("gpode_kernel_matrix: null pointer");
  return gp::kernel_matrix(kernel, Di, Do, raw_ell, raw_var, X, N, X2, M2, out, (hipStream_t)stream);
}

size_t gpode_kern_scratch(int kernel, int Di, int Do, int M, int S) {
  if (!gp::dims_supported(kernel, Di, Do) || M < 0 || S < 0) return 0;
  return gp::kern_scratch_floats(kernel, Di, Do, M, S);
}
int gpode_kern_cache(int kernel, int Di, int Do, int S, const float* raw_ell, const float* raw_var, const float* rff_w,
                     const float* rff_eps, const float* rff_u, float* pack, float* omega, float* phase, void* stream) {
  if (!raw_ell || !raw_var || !rff_w || !rff_eps || !rff_u || !pack) return gp::set_error("gpode_kern_cache: null pointer");
  return gp::kern_cache(kernel, Di, Do, S, raw_ell, raw_var, rff_w, rff_eps, rff_u, pack, omega, phase, (hipStream_t)stream);
}
int gpode_compute_nu_ws(int kernel, int Di, int Do, int M, size_t* ws_floats) {
  if (!ws_floats) return gp::set_error("gpode_compute_nu_ws: null pointer");
  return gp::compute_nu_ws(kernel, Di, Do, M, ws_floats);
}
int gpode_compute_nu(int kernel, int Di, int Do, int M, const float* Ku, const float* u_prior, const float* u, float* nu, float* ws,
                     void* stream) {
  if (!Ku || !u_prior || !u || !nu || !ws) return gp::set_error("gpode_compute_nu: null pointer");
  return gp::compute_nu(kernel, Di, Do, M, Ku, u_prior, u, nu, ws, (hipStream_t)stream);
}
int gpode_f_update(int kernel, int Di, int Do, int M, const float* raw_ell, const float* raw_var, const float* x2, const float* nu,
                   const float* x, int N, float* out, float* scratch, void* stream) {
  if (N < 0) return gp::set_error("gpode_f_update: N=%d", N);
  if (N == 0) return 0;
  if (!raw_ell || !raw_var || !x2 || !nu || !x || !out || !scratch) return gp::set_error("gpode_f_update: null pointer");
  return gp::f_update(kernel, Di, Do, M, raw_ell, raw_var, x2, nu, x, N, out, scratch, (hipStream_t)stream);
}

int gpode_conditional_ws(int Di, int Do, int M, int N, size_t* ws_floats) {
  if (!ws_floats) return gp::set_error("gpode_conditional_ws: null pointer");
  return gp::conditional_ws(Di, Do, M, N, ws_floats);
}

int gpode_conditional(int Di, int Do, int M, int N, const float* raw_ell, const float* raw_var, const float* Z, const float* Um,
                      const float* Us, int us_rank1, const float* x, int full_cov, float* mean, float* var, float* ws, void* stream) {
  if (!raw_ell || !raw_var || !Z || !Um || !Us || !x || !mean || !var || !ws) return gp::set_error("gpode_conditional: null pointer");
  return gp::conditional(Di, Do, M, N, raw_ell, raw_var, Z, Um, Us, us_rank1, x, full_cov, mean, var, ws, (hipStream_t)stream);
}

int gpode_conditional_df_ws(int D, int M, int N, size_t* ws_floats) {
  if (!ws_floats) return gp::set_error("gpode_conditional_df_ws: null pointer");
  return gp::conditional_df_ws(D, M, N, ws_floats);
}

int gpode_conditional_df(int D, int M, int N, const float* raw_ell, const float* raw_var, const float* Z, const float* Um,
                         const float* Us_packed, const float* x, int cov_mode, float* mean, float* var, float* ws, void* stream) {
  if (!raw_ell || !raw_var || !Z || !Um || !Us_packed || !x || !mean || !var || !ws) return gp::set_error("gpode_conditional_df: null pointer");
  return gp::conditional_df(D, M, N, raw_ell, raw_var, Z, Um, Us_packed, x, cov_mode, mean, var, ws, (hipStream_t)stream);
}

int gpode_svgp_kl_fwd(int M, int Do, const float* Um, const float* Us_packed, float* kl, void* stream) {
  if (!Um || !Us_packed || !kl) return gp::set_error("gpode_svgp_kl_fwd: null pointer");
  return gp::svgp_kl_fwd(M, Do, Um, Us_packed, kl, (hipStream_t)stream);
}

int gpode_svgp_kl_bwd(int M, int Do, const float* Um, const float* Us_packed, const float* g,
                      float* dUm, float* dUs, void* stream) {
  if (!Um || !Us_packed || !g || !dUm || !dUs) return gp::set_error("gpode_svgp_kl_bwd: null pointer");
  return gp::svgp_kl_bwd(M, Do, Um, Us_packed, g, dUm, dUs, (hipStream_t)stream);
}

int gpode_cache_bwd_sizes_n(int kernel, int Di, int Do, int M, int S, int ndraws, size_t* bws_floats) {
  if (!bws_floats) return gp::set_error("gpode_cache_bwd_sizes: null pointer");
  if (ndraws < 1) return gp::set_error("gpode_cache_bwd_sizes: %d draws", ndraws);
  return gp::cache_bwd_sizes(kernel, Di, Do, M, S, ndraws, bws_floats);
}
int gpode_cache_bwd_sizes(int kernel, int Di, int Do, int M, int S, size_t* bws_floats) {
  return gpode_cache_bwd_sizes_n(kernel, Di, Do, M, S, 1, bws_floats);
}

int gpode_cache_build_bwd_n(int kernel, int Di, int Do, int M, int S, int ndraws,
                            const float* raw_ell, const float* raw_var, const float* Z, const float* eps_u,
                            const float* pack, const float* ws, float* gpack, float* bws,
                            float* g_raw_ell, float* g_raw_var, float* g_Z, float* g_Um, float* g_Us, int prepared, void* stream) {
  if (!raw_ell || !raw_var || !Z || !eps_u || !pack || !ws || !gpack || !bws || !g_raw_ell || !g_raw_var || !g_Z || !g_Um || !g_Us)
    return gp::set_error("gpode_cache_build_bwd: null pointer");
  if (ndraws < 1 || ndraws > 65535) return gp::set_error("gpode_cache_build_bwd: %d draws", ndraws);
  return gp::cache_build_bwd(kernel, Di, Do, M, S, ndraws, raw_ell, raw_var, Z, eps_u, pack, ws, gpack, bws,
                             g_raw_ell, g_raw_var, g_Z, g_Um, g_Us, prepared, (hipStream_t)stream);
}
int gpode_cache_build_bwd(int kernel, int Di, int Do, int M, int S,
                          const float* raw_ell, const float* raw_var, const float* Z, const float* eps_u,
                          const float* pack, const float* ws, float* gpack, float* bws,
                          float* g_raw_ell, float* g_raw_var, float* g_Z, float* g_Um, float* g_Us, int prepared, void* stream) {
  return gpode_cache_build_bwd_n(kernel, Di, Do, M, S, 1, raw_ell, raw_var, Z, eps_u, pack, ws, gpack, bws, g_raw_ell, g_raw_var, g_Z, g_Um,
                                 g_Us, prepared, stream);
}
int gpode_cache_bwd_prepare_n(int kernel, int Di, int Do, int M, int S, int ndraws, const float* ws, float* bws, void* stream) {
  if (!ws || !bws) return gp::set_error("gpode_cache_bwd_prepare: null pointer");
  if (ndraws < 1) return gp::set_error("gpode_cache_bwd_prepare: %d draws", ndraws);
  return gp::cache_bwd_prepare(kernel, Di, Do, M, S, ndraws, ws, bws, (hipStream_t)stream);
}
int gpode_cache_bwd_prepare(int kernel, int Di, int Do, int M, int S, const float* ws, float* bws, void* stream) {
  return gpode_cache_bwd_prepare_n(kernel, Di, Do, M, S, 1, ws, bws, stream);
}

// ---- conv VAE blocks -----------------------------------------------------------------------
#define GP_ST ((hipStream_t)stream)
// the geometry arguments every convolution export names alike
#define GP_GEOM gp::ConvGeom{.B = B, .Ci = Ci, .H = H, .W = W, .Co = Co, .K = K, .S = S, .P = P, .Ho = Ho, .Wo = Wo}
int gpode_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, int Co,
                     int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!x || !w || !y) return gp::set_error("gpode_conv2d_fwd: null pointer");
  return gp::conv2d_fwd(x, w, bias, y, GP_GEOM, GP_ST);
}
int gpode_conv2d_bwd_data(const float* gy, const float* w, const float* bias, float* gx, int B, int Ci, int H, int W, int Co,
                          int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!gy || !w || !gx) return gp::set_error("gpode_conv2d_bwd_data: null pointer");
  return gp::conv2d_bwd_data(gy, w, bias, gx, GP_GEOM, nullptr, GP_ST);
}
int gpode_conv2d_bwd_data_bn(const float* gy, const float* gy_bn, const float* w, const float* bias, float* gx, int B, int Ci, int H,
                             int W, int Co, int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!gy || !gy_bn || !w || !gx) return gp::set_error("gpode_conv2d_bwd_data_bn: null pointer");
  return gp::conv2d_bwd_data(gy, w, bias, gx, GP_GEOM, gy_bn, GP_ST);
}
int gpode_conv2d_fwd_bs(const float* x, size_t x_batch_stride, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, int Co,
                        int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!x || !w || !y) return gp::set_error("gpode_conv2d_fwd_bs: null pointer");
  if (x_batch_stride < (size_t)Ci * H * W) return gp::set_error("gpode_conv2d_fwd_bs: images overlap");
  return gp::conv2d_fwd(x, w, bias, y, GP_GEOM, GP_ST, x_batch_stride);
}
int gpode_conv2d_bwd_weight_bs(const float* x, size_t x_batch_stride, const float* gy, float* gw, float* gbias, float* scratch, int B, int Ci,
                               int H, int W, int Co, int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!x || !gy || !gw || !scratch) return gp::set_error("gpode_conv2d_bwd_weight_bs: null pointer");
  if (x_batch_stride < (size_t)Ci * H * W) return gp::set_error("gpode_conv2d_bwd_weight_bs: images overlap");
  return gp::conv2d_bwd_weight(x, gy, gw, gbias, scratch, GP_GEOM, nullptr, GP_ST, x_batch_stride);
}
size_t gpode_convT_fwd_stats_scratch(int Cout) { return gp::convT_fwd_stats_scratch(Cout); }
int gpode_convT_fwd_stats(const float* x, const float* x_bn, const float* w, const float* bias, float* y, int B, int Ci, int H, int W, int Co,
                          int K, int S, int P, int Ho, int Wo, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                          float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table,
                          float* scratch, int slot, void* stream) {
  if (!x || !w || !y || !gamma || !beta || !save_mean || !save_invstd || !table || !scratch)
    return gp::set_error("gpode_convT_fwd_stats: null pointer");
  if ((running_mean == nullptr) != (running_var == nullptr)) return gp::set_error("gpode_convT_fwd_stats: running_mean and running_var go together");
  return gp::convT_fwd_stats(x, x_bn, w, bias, y, GP_GEOM, gamma, beta, save_mean, save_invstd, running_mean, running_var, num_batches_tracked,
                             momentum, eps, table, scratch, slot, GP_ST);
}
size_t gpode_conv_wgrad_scratch(int B, int Ci, int Co, int K) { return gp::conv_wgrad_scratch(B, Ci, Co, K); }
int gpode_conv2d_bwd_weight(const float* x, const float* gy, float* gw, float* gbias, float* scratch, int B, int Ci, int H, int W,
                            int Co, int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!x || !gy || !gw || !scratch) return gp::set_error("gpode_conv2d_bwd_weight: null pointer");
  return gp::conv2d_bwd_weight(x, gy, gw, gbias, scratch, GP_GEOM, nullptr, GP_ST);
}
int gpode_conv2d_bwd_weight_bn(const float* x, const float* gy, const float* gy_bn, float* gw, float* gbias, float* scratch, int B, int Ci,
                               int H, int W, int Co, int K, int S, int P, int Ho, int Wo, void* stream) {
  if (!x || !gy || !gy_bn || !gw || !scratch) return gp::set_error("gpode_conv2d_bwd_weight_bn: null pointer");
  return gp::conv2d_bwd_weight(x, gy, gw, gbias, scratch, GP_GEOM, gy_bn, GP_ST);
}
#undef GP_GEOM
size_t gpode_bn_scratch(int B, int C) { return gp::bn_scratch(B, C); }
int gpode_bn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_invstd,
                 float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, int B, int C,
                 int HW, int relu, float* scratch, void* stream) {
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !scratch) return gp::set_error("gpode_bn_fwd: null pointer");
  return gp::bn_fwd(x, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, momentum, eps, B, C, HW, relu,
                    scratch, GP_ST);
}
int gpode_bn_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                 const float* save_invstd, float* gx, float* ggamma, float* gbeta, float* gx_chansum, int B, int C, int HW,
                 int relu, float* scratch, void* stream) {
  if (!x || !gy || !gamma || !beta || !save_mean || !save_invstd || !gx || !ggamma || !gbeta || !scratch)
    return gp::set_error("gpode_bn_bwd: null pointer");
  return gp::bn_bwd(x, gy, gamma, beta, save_mean, save_invstd, gx, ggamma, gbeta, gx_chansum, B, C, HW, relu, scratch, GP_ST);
}
int gpode_bn_stats(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd, float* running_mean,
                   float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table, int B, int C, int HW,
                   float* scratch, void* stream) {
  if (!x || !gamma || !beta || !save_mean || !save_invstd || !table || !scratch) return gp::set_error("gpode_bn_stats: null pointer");
  return gp::bn_stats(x, gamma, beta, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, momentum, eps, table, B, C, HW,
                      scratch, GP_ST);
}
int gpode_bn_moments(const float* x, float* moments, int B, int C, int HW, float* scratch, void* stream) {
  if (!x || !moments || !scratch) return gp::set_error("gpode_bn_moments: null pointer");
  return gp::bn_moments(x, moments, B, C, HW, scratch, GP_ST);
}
int gpode_bn_finalize(const float* gathered, int nranks, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                      float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* table,
                      int C, void* stream) {
  if (!gathered || !gamma || !beta || !save_mean || !save_invstd || !table) return gp::set_error("gpode_bn_finalize: null pointer");
  return gp::bn_finalize(gathered, nranks, gamma, beta, save_mean, save_invstd, running_mean, running_var, num_batches_tracked, momentum, eps,
                         table, C, GP_ST);
}
int gpode_bn_apply(const float* x, const float* table, float* y, int B, int C, int HW, int relu, void* stream) {
  if (!x || !table || !y) return gp::set_error("gpode_bn_apply: null pointer");
  return gp::bn_apply(x, table, y, B, C, HW, relu, GP_ST);
}
int gpode_bn_bwd_sums(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_invstd, float* sums, int B, int C, int HW, int relu, float* scratch, void* stream) {
  if (!x || !gy || !gamma || !beta || !save_mean || !save_invstd || !sums || !scratch) return gp::set_error("gpode_bn_bwd_sums: null pointer");
  return gp::bn_bwd_sums(x, gy, gamma, beta, save_mean, save_invstd, sums, B, C, HW, relu, scratch, GP_ST);
}
int gpode_bn_bwd_apply(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                       const float* save_invstd, const float* sums_gathered, const float* weights, int nranks, float count_all,
                       float* gx, float* ggamma, float* gbeta, float* gx_chansum, int B, int C, int HW, int relu, float* scratch,
                       void* stream) {
  if (!x || !gy || !gamma || !beta || !save_mean || !save_invstd || !sums_gathered || !weights || !gx || !ggamma || !gbeta || !scratch)
    return gp::set_error("gpode_bn_bwd_apply: null pointer");
  return gp::bn_bwd_apply(x, gy, gamma, beta, save_mean, save_invstd, sums_gathered, weights, nranks, count_all, gx, ggamma, gbeta, gx_chansum, B, C, HW, relu,
                          scratch, GP_ST);
}
void gpode_defer_reductions(int mode) { gp::defer_reductions(mode); }
int gpode_flush_reductions(void* stream) { return gp::flush_reductions(GP_ST); }
int gpode_dec10_bn_scratch_floats(void) { return gp::dec10_bn_scratch_floats(); }
int gpode_dec10_bn_bwd_sums(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, float* sums, int B, float* scratch, void* stream) {
  if (!c || !gy || !w || !gamma || !beta || !save_mean || !save_invstd || !scratch) return gp::set_error("gpode_dec10_bn_bwd_sums: null pointer");
  if (B < 1) return gp::set_error("gpode_dec10_bn_bwd_sums: B >= 1");
  return gp::dec10_bn_bwd_sums(c, gy, w, gamma, beta, save_mean, save_invstd, sums, B, scratch, GP_ST);
}
int gpode_dec10_bn_wgrad_scratch_floats(void) { return gp::dec10_bn_wgrad_scratch_floats(); }
int gpode_dec10_bn_bwd_sums_wgrad(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* save_mean,
                                  const float* save_invstd, float* sums, float* gw, float* gbias, int B, float* scratch, float* wscratch,
                                  void* stream) {
  if (!c || !gy || !w || !gamma || !beta || !save_mean || !save_invstd || !scratch || !gw || !wscratch)
    return gp::set_error("gpode_dec10_bn_bwd_sums_wgrad: null pointer");
  if (B < 1) return gp::set_error("gpode_dec10_bn_bwd_sums_wgrad: B >= 1");
  return gp::dec10_bn_bwd_sums(c, gy, w, gamma, beta, save_mean, save_invstd, sums, B, scratch, GP_ST, gw, wscratch, gbias);
}
int gpode_dec10_bn_bwd_apply(const float* c, const float* gy, const float* w, const float* gamma, const float* beta, const float* save_mean,
                             const float* save_invstd, const float* sums_gathered, const float* weights, int nranks, float count_all,
                             float* gc, float* ggamma, float* gbeta, float* gc_chansum, int B, float* scratch, void* stream) {
  if (!c || !gy || !w || !gamma || !beta || !save_mean || !save_invstd || !gc || !ggamma || !gbeta || !scratch)
    return gp::set_error("gpode_dec10_bn_bwd_apply: null pointer");
  if (B < 1) return gp::set_error("gpode_dec10_bn_bwd_apply: B >= 1");
  return gp::dec10_bn_bwd_apply(c, gy, w, gamma, beta, save_mean, save_invstd, sums_gathered, weights, nranks, count_all, gc, ggamma, gbeta, gc_chansum,
                                B, scratch, GP_ST);
}
int gpode_bn_eval(const float* x, const float* gy, const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, float* out, int B, int C, int HW, int relu, void* stream) {
  if (!x || !gamma || !beta || !running_mean || !running_var || !out) return gp::set_error("gpode_bn_eval: null pointer");
  return gp::bn_eval(x, gy, gamma, beta, running_mean, running_var, eps, out, B, C, HW, relu, GP_ST);
}
int gpode_bn_eval_table(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* table,
                        int C, void* stream) {
  if (!gamma || !beta || !running_mean || !running_var || !table) return gp::set_error("gpode_bn_eval_table: null pointer");
  return gp::bn_eval_table(gamma, beta, running_mean, running_var, eps, table, C, GP_ST);
}
// The checked operation under the four gpode_dec10_predict* exports, which name themselves and the operands their prototype lacks
static int predict_any(const char* who, bool ll, bool ragged, const float* c, const float* table, const float* w, const float* bias,
                       const float* X, int Lc, int F, int Th, int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state,
                       float* ell, int L_total, const int* n_obs, void* stream) {
  if (!c || !table || !w || !X || !se_state) return gp::set_error("%s: null pointer", who);
  const gp::PredictArgs a{.c = c, .table = table, .w = w, .bias = bias, .X = X, .Lc = Lc, .F = F, .Th = Th, .T_obs = T_obs, .done = done,
                          .pred_mean = pred_mean, .pred_m2 = pred_m2, .se_state = se_state, .ell = ell, .L_total = L_total, .n_obs = n_obs};
  return gp::dec10_predict(who, ll, ragged, a, GP_ST);
}
int gpode_dec10_predict(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                        int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, void* stream) {
  return predict_any("gpode_dec10_predict", false, false, c, table, w, bias, X, Lc, F, Th, T_obs, done, pred_mean, pred_m2, se_state, nullptr, 0,
                     nullptr, stream);
}
int gpode_dec10_predict_ll(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                           int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, float* ell, int L_total, void* stream) {
  return predict_any("gpode_dec10_predict_ll", true, false, c, table, w, bias, X, Lc, F, Th, T_obs, done, pred_mean, pred_m2, se_state, ell,
                     L_total, nullptr, stream);
}
int gpode_dec10_predict_len(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                            int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, const int* n_obs, void* stream) {
  return predict_any("gpode_dec10_predict_len", false, true, c, table, w, bias, X, Lc, F, Th, T_obs, done, pred_mean, pred_m2, se_state, nullptr,
                     0, n_obs, stream);
}
int gpode_dec10_predict_ll_len(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                               int T_obs, int done, float* pred_mean, float* pred_m2, float* se_state, float* ell, int L_total,
                               const int* n_obs, void* stream) {
  return predict_any("gpode_dec10_predict_ll_len", true, true, c, table, w, bias, X, Lc, F, Th, T_obs, done, pred_mean, pred_m2, se_state, ell,
                     L_total, n_obs, stream);
}
int gpode_dec10_predict_w(const float* c, const float* table, const float* w, const float* bias, const float* X, int Lc, int F, int Th,
                          int T_obs, int done, const float* logw, int L_total, int N, float* wstate, float* pred_mean, float* pred_m2,
                          float* wse, const int* n_obs, void* stream) {
  const char* who = "gpode_dec10_predict_w";
  if (!c || !table || !w || !X || !pred_mean || !pred_m2 || !wse) return gp::set_error("%s: null pointer", who);
  if (!logw) return gp::set_error("%s: logw is NULL", who);
  if (!wstate) return gp::set_error("%s: wstate is NULL", who);
  const gp::PredictWArgs a{.c = c, .table = table, .w = w, .bias = bias, .X = X, .Lc = Lc, .F = F, .Th = Th, .T_obs = T_obs, .done = done,
                           .logw = logw, .L_total = L_total, .N = N, .wstate = wstate, .pred_mean = pred_mean, .pred_m2 = pred_m2,
                           .wse = wse, .n_obs = n_obs};
  return gp::dec10_predict_w(who, a, GP_ST);
}
int gpode_chan_sum(const float* v, float* out, int B, int C, int HW, float* scratch, void* stream) {
  if (!v || !out || !scratch) return gp::set_error("gpode_chan_sum: null pointer");
  return gp::chan_sum(v, out, B, C, HW, scratch, GP_ST);
}
int gpode_act_fwd(const float* x, float* y, size_t n, int mode, void* stream) { return gp::act_fwd(x, y, n, mode, GP_ST); }
int gpode_act_bwd(const float* y, const float* gy, float* gx, size_t n, int mode, void* stream) { return gp::act_bwd(y, gy, gx, n, mode, GP_ST); }
int gpode_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, void* stream) {
  if (!x || !w || !y) return gp::set_error("gpode_linear_fwd: null pointer");
  return gp::linear_fwd(x, w, bias, y, B, In, Out, GP_ST);
}
size_t gpode_linear_bwd_scratch(int B, int In, int Out) { return gp::linear_bwd_scratch(B, In, Out); }
int gpode_linear_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out,
                     float* scratch, void* stream) {
  if (!x || !w || !gy) return gp::set_error("gpode_linear_bwd: null pointer");
  return gp::linear_bwd(x, w, gy, gx, gw, gb, B, In, Out, scratch, GP_ST);
}
int gpode_linear_relu_fwd(const float* x, const float* w, const float* bias, float* y, int B, int In, int Out, void* stream) {
  if (!x || !w || !y) return gp::set_error("gpode_linear_relu_fwd: null pointer");
  return gp::linear_relu_fwd(x, w, bias, y, B, In, Out, GP_ST);
}
int gpode_linear_relu_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int B, int In, int Out,
                          void* stream) {
  if (!x || !w || !gy) return gp::set_error("gpode_linear_relu_bwd: null pointer");
  return gp::linear_relu_bwd(x, w, gy, gx, gw, gb, B, In, Out, GP_ST);
}
int gpode_loglik_fwd(const float* X, const float* z, float* ll, size_t n, size_t nX, void* stream) { return gp::loglik_fwd(X, z, ll, n, nX, GP_ST); }
int gpode_loglik_bwd(const float* X, const float* z, const float* g, float* gz, size_t n, size_t nX, void* stream) {
  return gp::loglik_bwd(X, z, g, gz, n, nX, GP_ST);
}
// The likelihood's row operations.  The twins without frame counts pass an empty mask; `ragged` says that the export takes counts, so a
// null n_obs is refused there and means "every frame" here.  The legacy rowsum pair checks nothing (its callers do).
static int rowsum_any(const char* who, bool ragged, bool bwd, const float* X, const float* z, const float* grow, float* out, size_t rows,
                      size_t inner, size_t nX, const int* n_obs, int T, size_t frame, void* stream) {
  if (ragged) {
    if (!X || !z || !out || (bwd && !grow)) return gp::set_error("%s: null pointer", who);
    if (!rows || !inner || !nX) return gp::set_error("%s: empty input", who);
  }
  const gp::LogLikRows r{.X = X, .z = z, .rows = rows, .inner = inner, .nX = nX};
  const gp::FrameMask m{.n_obs = n_obs, .T = T, .frame = frame};
  return bwd ? gp::loglik_rowsum_bwd(who, ragged, r, m, grow, out, GP_ST) : gp::loglik_rowsum_fwd(who, ragged, r, m, out, GP_ST);
}
int gpode_loglik_rowsum_fwd(const float* X, const float* z, float* out, size_t rows, size_t inner, size_t nX, void* stream) {
  return rowsum_any("gpode_loglik_rowsum_fwd", false, false, X, z, nullptr, out, rows, inner, nX, nullptr, 0, 0, stream);
}
int gpode_loglik_rowsum_bwd(const float* X, const float* z, const float* grow, float* gz, size_t rows, size_t inner, size_t nX,
                            void* stream) {
  return rowsum_any("gpode_loglik_rowsum_bwd", false, true, X, z, grow, gz, rows, inner, nX, nullptr, 0, 0, stream);
}
int gpode_loglik_rowsum_fwd_len(const float* X, const float* z, float* out, size_t rows, size_t inner, size_t nX, const int* n_obs, int T,
                                size_t frame, void* stream) {
  return rowsum_any("gpode_loglik_rowsum_fwd_len", true, false, X, z, nullptr, out, rows, inner, nX, n_obs, T, frame, stream);
}
int gpode_loglik_rowsum_bwd_len(const float* X, const float* z, const float* grow, float* gz, size_t rows, size_t inner, size_t nX,
                                const int* n_obs, int T, size_t frame, void* stream) {
  return rowsum_any("gpode_loglik_rowsum_bwd_len", true, true, X, z, grow, gz, rows, inner, nX, n_obs, T, frame, stream);
}
int gpode_noise_fill(float* out, long long n_normal, long long n_uniform, unsigned long long seed, unsigned long long* state, void* stream) {
  if (n_normal < 0 || n_uniform < 0) return gp::set_error("gpode_noise_fill: negative count");
  if (n_normal + n_uniform == 0) return 0;
  if (!out || !state) return gp::set_error("gpode_noise_fill: null pointer");
  return gp::noise_fill(out, n_normal, n_uniform, seed, state, GP_ST);
}
int gpode_reparam_kl_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, float* klpart, int N, int q, void* stream) {
  if (N == 0) return 0;
  if (!mu || !logvar || !eps || !z || !klpart || q < 1 || ld < q) return gp::set_error("gpode_reparam_kl_fwd: bad argument");
  return gp::reparam_kl_fwd(mu, logvar, ld, eps, z, klpart, N, q, GP_ST);
}
int gpode_reparam_kl_bwd(const float* gz, const float* gklpart, const float* mu, const float* logvar, int ld, const float* eps, float* gmu,
                         float* glogvar, int ldg, int N, int q, void* stream) {
  if (N == 0) return 0;
  if (!mu || !logvar || !eps || !gmu || !glogvar || q < 1 || ld < q || ldg < q) return gp::set_error("gpode_reparam_kl_bwd: bad argument");
  return gp::reparam_kl_bwd(gz, gklpart, mu, logvar, ld, eps, gmu, glogvar, ldg, N, q, GP_ST);
}
int gpode_reparam_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int N, int q, void* stream) {
  if (N == 0) return 0;
  if (!mu || !logvar || !eps || !z || q < 1 || ld < q) return gp::set_error("gpode_reparam_fwd: bad argument");
  return gp::reparam_fwd(mu, logvar, ld, eps, z, N, q, GP_ST);
}
int gpode_reparam_draws_fwd(const float* mu, const float* logvar, int ld, const float* eps, float* z, int ldz, float* lw, int accumulate,
                            int L, int N, int q, void* stream) {
  if (L < 0 || N < 0 || q < 1 || q > 16 || ld < q || ldz < q || (accumulate != 0 && accumulate != 1) || (long long)L * N > 0x7fffffffLL / 16)
    return gp::set_error("gpode_reparam_draws_fwd: bad argument (L=%d N=%d q=%d ld=%d ldz=%d accumulate=%d; q <= 16)", L, N, q, ld, ldz, accumulate);
  if (L == 0 || N == 0) return 0;
  if (!mu || !logvar || !eps || !z || !lw) return gp::set_error("gpode_reparam_draws_fwd: null pointer");
  return gp::reparam_draws_fwd(mu, logvar, ld, eps, z, ldz, lw, accumulate, L, N, q, GP_ST);
}
int gpode_reparam_draws_bwd(const float* gz, int ldgz, const float* glw, const float* mu, const float* logvar, int ld, const float* eps,
                            float* gmu, float* glogvar, int ldg, int K, int N, int q, void* stream) {
  if (K < 1 || K > 64 || N < 1 || q < 1 || ld < q || ldg < q || (gz && ldgz < q) || (long long)K * N > 0x7fffffffLL / 64)
    return gp::set_error("gpode_reparam_draws_bwd: bad argument (K=%d N=%d q=%d ld=%d ldg=%d ldgz=%d; 1 <= K <= 64)", K, N, q, ld, ldg, ldgz);
  if (!mu || !logvar || !eps || !gmu || !glogvar) return gp::set_error("gpode_reparam_draws_bwd: null pointer");
  return gp::reparam_draws_bwd(gz, ldgz, glw, mu, logvar, ld, eps, gmu, glogvar, ldg, K, N, q, GP_ST);
}
int gpode_elbo_iw_fwd(const float* lpart, int rows, int nsplit, const float* lw, int L, int K, int N, int M, int Do, const float* Um,
                      const float* Us, float nobs, float* out, void* stream) {
  if (!lpart || !lw || !Um || !Us || !out) return gp::set_error("gpode_elbo_iw_fwd: null pointer");
  return gp::elbo_iw_fwd({.lpart = lpart, .rows = rows, .nsplit = nsplit, .lw = lw, .L = L, .K = K},
                         {.N = N, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, out, GP_ST);
}
// g_ess is taken and not read: the ess output carries no gradient
int gpode_elbo_iw_bwd(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, const float* g_ess, const float* lpart,
                      int rows, int nsplit, const float* lw, int L, int K, int N, int M, int Do, const float* Um, const float* Us, float nobs,
                      float* grow, float* glw, float* dUm, float* dUs, void* stream) {
  (void)g_ess;
  if (!lpart || !lw || !Um || !Us || !grow || !glw || !dUm || !dUs) return gp::set_error("gpode_elbo_iw_bwd: null pointer");
  return gp::elbo_iw_bwd("gpode_elbo_iw_bwd", false, {.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu},
                         {.lpart = lpart, .rows = rows, .nsplit = nsplit, .lw = lw, .L = L, .K = K},
                         {.N = N, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.glrow = grow, .dUm = dUm, .dUs = dUs}, glw, {}, GP_ST);
}
int gpode_elbo_iw_bwd_ll(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, const float* g_ess,
                         const float* lpart, int rows, int nsplit, const float* lw, int L, int K, int N, int M, int Do, const float* Um,
                         const float* Us, float nobs, float* grow, float* glw, float* dUm, float* dUs, const float* X, const float* z,
                         float* ga, size_t n_logits, size_t nX, void* stream) {
  (void)g_ess;
  if (!lpart || !lw || !Um || !Us || !grow || !glw || !dUm || !dUs || !X || !z || !ga) return gp::set_error("gpode_elbo_iw_bwd_ll: null pointer");
  return gp::elbo_iw_bwd("gpode_elbo_iw_bwd_ll", true, {.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu},
                         {.lpart = lpart, .rows = rows, .nsplit = nsplit, .lw = lw, .L = L, .K = K},
                         {.N = N, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.glrow = grow, .dUm = dUm, .dUs = dUs}, glw,
                         {.X = X, .z = z, .ga = ga, .n = n_logits, .nX = nX}, GP_ST);
}
int gpode_reparam_bwd(const float* gz, const float* logvar, int ld, const float* eps, float* gmu, float* glogvar, int ldg, int N, int q,
                      void* stream) {
  if (N == 0) return 0;
  if (!gz || !logvar || !eps || !gmu || !glogvar || q < 1 || ld < q || ldg < q) return gp::set_error("gpode_reparam_bwd: bad argument");
  return gp::reparam_bwd(gz, logvar, ld, eps, gmu, glogvar, ldg, N, q, GP_ST);
}
int gpode_normal_kl_fwd(const float* mu, const float* logvar, int ld, float* klrow, int N, int q, void* stream) {
  if (N == 0) return 0;
  if (!mu || !logvar || !klrow || q < 1 || ld < q) return gp::set_error("gpode_normal_kl_fwd: bad argument");
  return gp::normal_kl_fwd(mu, logvar, ld, klrow, N, q, GP_ST);
}
int gpode_normal_kl_bwd(const float* grow, const float* mu, const float* logvar, int ld, float* gmu, float* glogvar, int ldg, int N, int q,
                        void* stream) {
  if (N == 0) return 0;
  if (!grow || !mu || !logvar || !gmu || !glogvar || q < 1 || ld < q || ldg < q) return gp::set_error("gpode_normal_kl_bwd: bad argument");
  return gp::normal_kl_bwd(grow, mu, logvar, ld, gmu, glogvar, ldg, N, q, GP_ST);
}
int gpode_sigmoid_loglik_splits(size_t rows, size_t inner) { return gp::sigmoid_loglik_splits(rows, inner); }
static int sigmoid_fwd_any(const char* who, bool ragged, const float* X, const float* a, float* z, float* part, size_t rows, size_t inner,
                           size_t nX, int nsplit, const int* n_obs, int T, size_t frame, void* stream) {
  if (!X || !a || !z || !part) return gp::set_error("%s: null pointer", who);
  if (!rows || !inner || !nX) return gp::set_error("%s: empty input", who);
  return gp::sigmoid_loglik_fwd(who, ragged, {.X = X, .z = nullptr, .rows = rows, .inner = inner, .nX = nX},
                                {.n_obs = n_obs, .T = T, .frame = frame}, a, z, part, nsplit, GP_ST);
}
static int sigmoid_bwd_any(const char* who, bool ragged, const float* X, const float* z, const float* grow, float* ga, size_t rows,
                           size_t inner, size_t nX, const int* n_obs, int T, size_t frame, void* stream) {
  if (!X || !z || !grow || !ga) return gp::set_error("%s: null pointer", who);
  if (!rows || !inner || !nX) return gp::set_error("%s: empty input", who);
  return gp::sigmoid_loglik_bwd(who, ragged, {.X = X, .z = z, .rows = rows, .inner = inner, .nX = nX}, {.n_obs = n_obs, .T = T, .frame = frame},
                                grow, ga, GP_ST);
}
int gpode_sigmoid_loglik_fwd(const float* X, const float* a, float* z, float* part, size_t rows, size_t inner, size_t nX, int nsplit,
                             void* stream) {
  return sigmoid_fwd_any("gpode_sigmoid_loglik_fwd", false, X, a, z, part, rows, inner, nX, nsplit, nullptr, 0, 0, stream);
}
int gpode_sigmoid_loglik_bwd(const float* X, const float* z, const float* grow, float* ga, size_t rows, size_t inner, size_t nX,
                             void* stream) {
  return sigmoid_bwd_any("gpode_sigmoid_loglik_bwd", false, X, z, grow, ga, rows, inner, nX, nullptr, 0, 0, stream);
}
int gpode_sigmoid_loglik_fwd_len(const float* X, const float* a, float* z, float* part, size_t rows, size_t inner, size_t nX, int nsplit,
                                 const int* n_obs, int T, size_t frame, void* stream) {
  return sigmoid_fwd_any("gpode_sigmoid_loglik_fwd_len", true, X, a, z, part, rows, inner, nX, nsplit, n_obs, T, frame, stream);
}
int gpode_sigmoid_loglik_bwd_len(const float* X, const float* z, const float* grow, float* ga, size_t rows, size_t inner, size_t nX,
                                 const int* n_obs, int T, size_t frame, void* stream) {
  return sigmoid_bwd_any("gpode_sigmoid_loglik_bwd_len", true, X, z, grow, ga, rows, inner, nX, n_obs, T, frame, stream);
}
int gpode_gather_frames_fwd(const float* zt, int ld, int q, const int* src, int L, int N, int T, int P, float* out, void* stream) {
  if (!zt || !out) return gp::set_error("gpode_gather_frames_fwd: null pointer");
  if (!src) return gp::set_error("gpode_gather_frames_fwd: the frame index is NULL");
  if (q < 1 || q > ld) return gp::set_error("gpode_gather_frames_fwd: 1 <= q <= ld");
  if (L < 1 || N < 1 || T < 1 || P < 1 || (long long)P > (long long)N * T) return gp::set_error("gpode_gather_frames_fwd: L, N, T >= 1 and 1 <= P <= N * T");
  return gp::gather_frames_fwd(zt, ld, q, src, L, N, T, P, out, GP_ST);
}
int gpode_gather_frames_bwd(const float* gout, int ld, int q, const int* src, const int* off, int L, int N, int T, int P, float* gzt,
                            void* stream) {
  if (!gout || !gzt) return gp::set_error("gpode_gather_frames_bwd: null pointer");
  if (!src || !off) return gp::set_error("gpode_gather_frames_bwd: the frame index is NULL");
  if (q < 1 || q > ld) return gp::set_error("gpode_gather_frames_bwd: 1 <= q <= ld");
  if (L < 1 || N < 1 || T < 1 || P < 1 || (long long)P > (long long)N * T) return gp::set_error("gpode_gather_frames_bwd: L, N, T >= 1 and 1 <= P <= N * T");
  return gp::gather_frames_bwd(gout, ld, q, off, L, N, T, P, gzt, GP_ST);
}
int gpode_sigmoid_loglik_fwd_pk(const float* X, const float* a, float* z, float* part, size_t rows, const int* off, int T, size_t frame,
                                size_t nX, int nsplit, void* stream) {
  if (!X || !a || !z || !part) return gp::set_error("gpode_sigmoid_loglik_fwd_pk: null pointer");
  if (!rows || !nX) return gp::set_error("gpode_sigmoid_loglik_fwd_pk: empty input");
  return gp::sigmoid_loglik_fwd_pk({.X = X, .z = nullptr, .rows = rows, .inner = 0, .nX = nX}, {.index = off, .P = 0, .T = T, .frame = frame}, a, z,
                                   part, nsplit, GP_ST);
}
int gpode_sigmoid_loglik_bwd_pk(const float* X, const float* z, const float* grow, float* ga, size_t rows, const int* src, int P, int T,
                                size_t frame, size_t nX, void* stream) {
  if (!X || !z || !grow || !ga) return gp::set_error("gpode_sigmoid_loglik_bwd_pk: null pointer");
  if (!rows || !nX) return gp::set_error("gpode_sigmoid_loglik_bwd_pk: empty input");
  return gp::sigmoid_loglik_bwd_pk({.X = X, .z = z, .rows = rows, .inner = 0, .nX = nX}, {.index = src, .P = P, .T = T, .frame = frame}, grow, ga,
                                   GP_ST);
}
// The ELBO in one launch.  The latent KL term arrives as the encoder's heads (hs, hv: gpode_elbo_all_fwd, _bwd, _bwd_ll[_len]) or as values
// computed upstream (kls, klv: the *_kl exports); gp::ElboKl holds either (`heads` says which the export requires).
static int elbo_fwd_any(const char* who, bool heads, const float* lpart, int nl_rows, int nl_values, const gp::ElboShape& s, const gp::ElboKl& kl,
                        float* out, void* stream) {
  if (!lpart || !(heads ? kl.hs : kl.kls) || !s.Um || !s.Us || !out || (kl.nkv > 0 && !kl.klv)) return gp::set_error("%s: null pointer", who);
  if (nl_rows < 1 || nl_values < nl_rows || s.N < 1 || s.q < 1 || s.M < 1 || s.Do < 1 || (!heads && kl.nks < 1) || kl.nkv < 0)
    return gp::set_error("%s: bad sizes", who);
  return gp::elbo_all_fwd(lpart, nl_rows, nl_values, s, kl, out, GP_ST);
}
int gpode_elbo_all_fwd(const float* lpart, int nl_rows, int nl_values, const float* hs, const float* hv, int N, int q, int M, int Do,
                       const float* Um, const float* Us, float nobs, float* out, void* stream) {
  return elbo_fwd_any("gpode_elbo_all_fwd", true, lpart, nl_rows, nl_values, {.N = N, .q = q, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs},
                      {.hs = hs, .hv = hv}, out, stream);
}
int gpode_elbo_all_fwd_kl(const float* lpart, int nl_rows, int nl_values, const float* kls, int nks, const float* klv, int nkv, int N, int M,
                          int Do, const float* Um, const float* Us, float nobs, float* out, void* stream) {
  return elbo_fwd_any("gpode_elbo_all_fwd_kl", false, lpart, nl_rows, nl_values, {.N = N, .q = 1, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs},
                      {.kls = kls, .klv = klv, .nks = nks, .nkv = nkv}, out, stream);
}
int gpode_elbo_all_bwd(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, const float* hs,
                       const float* hv, int N, int q, int M, int Do, const float* Um, const float* Us, float nobs, float* glrow, float* ghs,
                       float* ghv, float* dUm, float* dUs, void* stream) {
  if (!hs || !Um || !Us || !glrow || !ghs || !dUm || !dUs || (hv && !ghv)) return gp::set_error("gpode_elbo_all_bwd: null pointer");
  if (nl_rows < 1 || N < 1 || q < 1 || M < 1 || Do < 1) return gp::set_error("gpode_elbo_all_bwd: bad sizes");
  return gp::elbo_all_bwd({.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu}, nl_rows,
                          {.N = N, .q = q, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.hs = hs, .hv = hv, .ghs = ghs, .ghv = ghv},
                          {.glrow = glrow, .dUm = dUm, .dUs = dUs}, GP_ST);
}
// the fused backward, heads (`heads`: hs and ghs required, q >= 1) or values (gkls required, nks >= 1), with or without frame counts
static int elbo_bwd_ll_any(const char* who, bool heads, bool ragged, const gp::ElboSeeds& g, int nl_rows, const gp::ElboShape& s,
                           const gp::ElboKl& kl, const gp::ElboGrads& o, const gp::ElboLogits& lg, const gp::FrameMask& m, void* stream) {
  if (!s.Um || !s.Us || !o.glrow || !o.dUm || !o.dUs || !lg.X || !lg.z || !lg.ga ||
      (heads ? (!kl.hs || !kl.ghs || (kl.hv && !kl.ghv)) : (!kl.gkls || (kl.nkv > 0 && !kl.gklv))))
    return gp::set_error("%s: null pointer", who);
  if (nl_rows < 1 || s.N < 1 || s.q < 1 || s.M < 1 || s.Do < 1 || (!heads && (kl.nks < 1 || kl.nkv < 0)) || lg.n < 1 || lg.nX < 1 ||
      lg.n % lg.nX != 0)
    return gp::set_error("%s: bad sizes", who);
  return gp::elbo_loglik_bwd(who, ragged, g, nl_rows, s, kl, o, lg, m, GP_ST);
}
int gpode_elbo_all_bwd_ll(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, const float* hs,
                          const float* hv, int N, int q, int M, int Do, const float* Um, const float* Us, float nobs, float* glrow, float* ghs,
                          float* ghv, float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX,
                          void* stream) {
  return elbo_bwd_ll_any("gpode_elbo_all_bwd_ll", true, false, {.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu}, nl_rows,
                         {.N = N, .q = q, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.hs = hs, .hv = hv, .ghs = ghs, .ghv = ghv},
                         {.glrow = glrow, .dUm = dUm, .dUs = dUs}, {.X = X, .z = z, .ga = ga, .n = n_logits, .nX = nX}, {}, stream);
}
int gpode_elbo_all_bwd_ll_len(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, const float* hs,
                              const float* hv, int N, int q, int M, int Do, const float* Um, const float* Us, float nobs, float* glrow, float* ghs,
                              float* ghv, float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX,
                              const int* n_obs, int T, size_t frame, void* stream) {
  return elbo_bwd_ll_any("gpode_elbo_all_bwd_ll_len", true, true, {.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu}, nl_rows,
                         {.N = N, .q = q, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.hs = hs, .hv = hv, .ghs = ghs, .ghv = ghv},
                         {.glrow = glrow, .dUm = dUm, .dUs = dUs}, {.X = X, .z = z, .ga = ga, .n = n_logits, .nX = nX},
                         {.n_obs = n_obs, .T = T, .frame = frame}, stream);
}
int gpode_elbo_all_bwd_ll_kl(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, int N, int M, int Do,
                             const float* Um, const float* Us, float nobs, float* glrow, float* gkls, int nks, float* gklv, int nkv,
                             float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX, void* stream) {
  return elbo_bwd_ll_any("gpode_elbo_all_bwd_ll_kl", false, false, {.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu}, nl_rows,
                         {.N = N, .q = 1, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.gkls = gkls, .gklv = gklv, .nks = nks, .nkv = nkv},
                         {.glrow = glrow, .dUm = dUm, .dUs = dUs}, {.X = X, .z = z, .ga = ga, .n = n_logits, .nX = nX}, {}, stream);
}
int gpode_elbo_all_bwd_ll_kl_len(const float* g_loss, const float* g_nll, const float* g_kl, const float* g_klu, int nl_rows, int N, int M,
                                 int Do, const float* Um, const float* Us, float nobs, float* glrow, float* gkls, int nks, float* gklv, int nkv,
                                 float* dUm, float* dUs, const float* X, const float* z, float* ga, size_t n_logits, size_t nX,
                                 const int* n_obs, int T, size_t frame, void* stream) {
  return elbo_bwd_ll_any("gpode_elbo_all_bwd_ll_kl_len", false, true, {.g0 = g_loss, .g1 = g_nll, .g2 = g_kl, .g3 = g_klu}, nl_rows,
                         {.N = N, .q = 1, .M = M, .Do = Do, .Um = Um, .Us = Us, .nobs = nobs}, {.gkls = gkls, .gklv = gklv, .nks = nks, .nkv = nkv},
                         {.glrow = glrow, .dUm = dUm, .dUs = dUs}, {.X = X, .z = z, .ga = ga, .n = n_logits, .nX = nX},
                         {.n_obs = n_obs, .T = T, .frame = frame}, stream);
}
int gpode_elbo_fwd(const float* lhood, int nl, const float* klrow, int nk, const float* kl_u, float nobs, float* out, void* stream) {
  if (!lhood || !klrow || !kl_u || !out || nl < 1 || nk < 1) return gp::set_error("gpode_elbo_fwd: bad argument");
  return gp::elbo_fwd(lhood, nl, klrow, nk, kl_u, nobs, out, GP_ST);
}
int gpode_elbo_bwd(const float* gout, int nl, int nk, float nobs, float* glhood, float* gklrow, float* gklu, void* stream) {
  if (!gout || !glhood || !gklrow || !gklu || nl < 1 || nk < 1) return gp::set_error("gpode_elbo_bwd: bad argument");
  return gp::elbo_bwd(gout, nl, nk, nobs, glhood, gklrow, gklu, GP_ST);
}
int gpode_gather_multi(void* grads, const long long* offs, int ntensors, long long total, float* flat, void* stream) {
  if (!grads || !offs || !flat) return gp::set_error("gpode_gather_multi: null pointer");
  return gp::gather_multi((const float* const*)grads, offs, ntensors, total, flat, (hipStream_t)stream);
}

int gpode_adam_multi(void* params, void* grads, void* m1, void* m2, const long long* offs, int ntensors, long long total,
                     float lr, float beta1, float beta2, float eps, int step, int* step_dev, void* stream) {
  if (!params || !grads || !m1 || !m2 || !offs) return gp::set_error("gpode_adam_multi: null pointer");
  return gp::adam_multi((float* const*)params, (const float* const*)grads, (float* const*)m1, (float* const*)m2, offs, ntensors, total,
                        lr, beta1, beta2, eps, step, step_dev, GP_ST);
}
#undef GP_ST

}  // extern "C"
