// gp_adaptive.hip -- adaptive Dormand-Prince 5(4) rollout (forward) and its reverse sweep.
//
// Replaces torchdiffeq's `dopri5` behind Flow.forward (flow.py:49,68-86).  As in the fixed-grid rollout one wavefront (wave
// mapping) or one workgroup of four (team mapping) carries a trajectory from z0 to z_{T-1} in ONE launch; only the trip count
// is data-dependent.  Differences to torchdiffeq, by design:
//   * one controller PER TRAJECTORY (torchdiffeq couples the batch through one RMS norm): every trajectory meets its own tolerance;
//   * by default steps LAND on the output times (a step that would pass ts[t+1] is shortened to end on it; no dense output), so
//     zt[:, t] is a step end point and the reverse sweep needs no interpolant.  Results agree to the tolerances, not step by step.
//     The opt-in dense-output mode further down steps freely and interpolates, as torchdiffeq does.
//
// Controller (Hairer, Noersett, Wanner, Solving ODEs I, II.4-5)
//   err_i  = h sum_j e_j k_j,i                      (5th-order minus embedded 4th-order solution)
//   ratio  = sqrt(mean_i (err_i / (atol + rtol max(|y_i|, |ynew_i|)))^2),   accept iff ratio <= 1
//   h_new  = h clamp(0.9 ratio^(-1/5), 0.2, 10);  no growth on the step after a rejection
//   first step: h = min(100 h0, (0.01 / d1)^(1/5), ts[1] - ts[0]),  h0 = 0.01 d0 / d1,  d0 = |y0|, d1 = |f0| in the scaled RMS norm:
//               Hairer's estimate without its second-derivative probe, so that it costs no evaluation beyond f0 (= k1 of step one)
//   landing: inside an interval with `rem` left, a proposal with 1.01 h >= rem is replaced by rem (the 1 % stretch of Hairer's
//            DOPRI5 code: no sliver of a step is left over); after such a cut step the larger of the uncut proposal and the
//            controller's is carried into the next interval
//   failure: budget (K accepted steps recorded and more needed) -> status 1; step <= 16 eps max(|t|, |h|) -> status 2;
//            ts not increasing -> status 3.  The trajectory stops, its remaining outputs are NaN; others are unaffected.
//
// The seven slopes k_j are wave-uniform values.  They are kept in a wavefront-private row block of LDS (7 x 16 floats), not in
// registers: the stage loop then indexes them dynamically (ONE inlined evaluation of f instead of seven) and the kernel needs
// no more registers than the fixed-grid rk4 one, whose four slopes in registers are at the edge already at D = 16.
//
// Record (for the reverse sweep; all zero past the count): xstage (N,K,6,D) the six stage inputs of every ACCEPTED step (b7 = 0,
// so the seventh does not enter the step), hstep (N,K), iend (N,T-1) = accepted steps taken when output t+1 was reached.
//
// Dense-output mode (template parameter DENSE; gpode_rollout_dense_*): the controller above with `rem` the distance to the LAST
// output time -- the cut happens once, at ts[T-1], and the first step is capped by ts[T-1] - ts[0].  The interior outputs are read
// off the 4th-order continuous extension of the pair (Shampine; Hairer, Noersett, Wanner II.6, CONTD5), which costs no evaluation:
//   z(theta) = y_n + h sum_j w_j(theta) k_j,   theta = (t - t_n) / h in (0, 1],   j = 1..7 (k_7 = the FSAL slope at y_{n+1})
//   w_j(theta) = theta [b_j + (1 - theta) ((d_j1 - b_j) + theta ((2 b_j - d_j1 - d_j7) + (1 - theta) dp_d[j]))]
// Every output not yet written with ts[j] <= t_n + h belongs to the accepted step, and is formed before the step's seventh slope
// replaces row 0 of the slope block; the last output is the end state of the last step (theta = 1 exactly).  Time is an fp32 offset
// tn from ts[0] (the running sum of the accepted steps); theta and every loop condition derive from scalars.
// Record: xstage (N,K,7,D) (row 6 = y_{n+1}, where k_7 is evaluated), hstep (N,K), istep (N,T-1) = 1-based number of the accepted
// step that holds output t+1 (non-decreasing; a step may hold several outputs or none), theta (N,T-1).
#include "gp_rollout.hpp"

namespace gp {

// Dormand-Prince 5(4).  Row s: the weights of k_0 .. k_{s-1} in the input of stage s; row 6 is the 5th-order solution itself
// (FSAL: its slope is k_0 of the next step).  dp_e = 5th-order minus 4th-order weights.
__constant__ float dp_a[7][6] = {
    {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(1.0 / 5.0), 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(3.0 / 40.0), (float)(9.0 / 40.0), 0.f, 0.f, 0.f, 0.f},
    {(float)(44.0 / 45.0), (float)(-56.0 / 15.0), (float)(32.0 / 9.0), 0.f, 0.f, 0.f},
    {(float)(19372.0 / 6561.0), (float)(-25360.0 / 2187.0), (float)(64448.0 / 6561.0), (float)(-212.0 / 729.0), 0.f, 0.f},
    {(float)(9017.0 / 3168.0), (float)(-355.0 / 33.0), (float)(46732.0 / 5247.0), (float)(49.0 / 176.0), (float)(-5103.0 / 18656.0), 0.f},
    {(float)(35.0 / 384.0), 0.f, (float)(500.0 / 1113.0), (float)(125.0 / 192.0), (float)(-2187.0 / 6784.0), (float)(11.0 / 84.0)}};
__constant__ float dp_e[7] = {(float)(71.0 / 57600.0), 0.f, (float)(-71.0 / 16695.0), (float)(71.0 / 1920.0),
                              (float)(-17253.0 / 339200.0), (float)(22.0 / 525.0), (float)(-1.0 / 40.0)};

constexpr int KP = 16;                  // floats per slope row in LDS (D <= 16 for every compiled width)
// the quartic's free coefficient per slope (dense output)
__constant__ float dp_d[7] = {(float)(-12715105075.0 / 11282082432.0), 0.f, (float)(87487479700.0 / 32700410799.0),
                              (float)(-10690763975.0 / 1880347072.0), (float)(701980252875.0 / 199316789632.0),
                              (float)(-1453857185.0 / 822651844.0), (float)(69997945.0 / 29380423.0)};

constexpr int NREC = 6;                 // recorded stage inputs per accepted step (landing mode)
constexpr int NDEN = 7;                 // ... in dense mode: the end state, where the seventh slope is evaluated, is one of them

struct AdaptFwd {
  const float* pack; size_t pack_stride; int M, S;
  const float* z0; const float* ts; int N, T, K;
  float rtol, atol;
  float* zt; float* xstage; float* hstep; int* iend; int* counts;
};
struct AdaptBwd {
  const float* pack; size_t pack_stride; int M, S;
  const float* xstage; const float* hstep; const int* iend; const float* gzt; int N, T, K;
  float* gz0; float* astage;
};
// What the kernels take, filled from AdaptFwdArgs / AdaptBwdArgs (gp_launch.hpp) by adapt_fwd_arg and rollout_adaptive_bwd below.
// z0_stride: floats between the draws' initial states, 0 = one (N,D) block shared by all draws; it is the
// member after the mode's own pointers, so every other argument stays where it was.  ts_stride follows it: floats between the
// trajectories' time grids, 0 = the one (T,) grid all of them share, T = row n of a dense (N,T) block for trajectory n of every draw.
// The dense mode's kernels take one pointer more.
struct AdaptFwdLand : AdaptFwd { size_t z0_stride, ts_stride; };
struct AdaptFwdDense : AdaptFwd { float* theta; size_t z0_stride, ts_stride; };
struct AdaptBwdDense : AdaptBwd { const float* theta; };
template <bool DENSE> using AdaptFwdArg = std::conditional_t<DENSE, AdaptFwdDense, AdaptFwdLand>;
template <bool DENSE> using AdaptBwdArg = std::conditional_t<DENSE, AdaptBwdDense, AdaptBwd>;

// a value every lane holds identically -> a scalar: the controller's branches are then scalar branches, the same in every
// wavefront of a team (whose evaluations carry a workgroup barrier) because the slopes they derive from are bit-identical there
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <int DI> __device__ __forceinline__ void put_row(float* __restrict__ row, const float (&v)[DI]) {
#pragma unroll
  for (int d = 0; d < DI; ++d) row[d] = v[d];      // every lane writes the same value to the same address; it reads back its own
}

template <int DI> __device__ __forceinline__ float scaled_rms(const float (&v)[DI], const float (&a)[DI], const float (&b)[DI], float rtol, float atol) {
  float sq = 0.f;
#pragma unroll
  for (int d = 0; d < DI; ++d) {
    const float r = v[d] / (atol + rtol * fmaxf(fabsf(a[d]), fabsf(b[d])));
    sq = fmaf(r, r, sq);
  }
  return sqrtf(sq * (1.f / DI));
}

// weight of slope j (0-based) in the continuous extension at theta
__device__ __forceinline__ float dense_w(int j, float th) {
  const float b = j < 6 ? dp_a[6][j] : 0.f, d1 = j == 0 ? 1.f : 0.f, d7 = j == 6 ? 1.f : 0.f, om = 1.f - th;
  return th * (b + om * ((d1 - b) + th * ((2.f * b - d1 - d7) + om * dp_d[j])));
}

// One trajectory, start to end.  kst: this wavefront's 7 x KP floats of LDS.  wr: this wavefront writes the outputs (in a team all
// four compute the same values).  Pointers are the draw's; ts is the trajectory's own grid (a scalar pointer: ts_row).
// DENSE: one "interval" from ts[0] to ts[T-1]; the outputs inside it are interpolated when the step that holds them is accepted.
template <class EV, int DI, int DO, int ORDER, bool DENSE>
__device__ __forceinline__ void dopri5_trajectory(EV& ev, const AdaptFwd& a, const float* __restrict__ z0, float* __restrict__ zt,
                                                  float* __restrict__ xstage, float* __restrict__ hstep, int* __restrict__ iend,
                                                  float* __restrict__ theta, int* __restrict__ counts, int n, float* __restrict__ kst,
                                                  bool wr, int lane, const float* __restrict__ ts) {
  constexpr int NR = DENSE ? NDEN : NREC;
  const int T = a.T, K = a.K;
  const float rtol = a.rtol, atol = a.atol;
  const bool rec = xstage != nullptr && wr;
  float y[DI], xs[DI], kv[DI];
#pragma unroll
  for (int i = 0; i < DI; ++i) y[i] = z0[(size_t)n * DI + i];
  float* out = zt + (size_t)n * T * DI;
  float* xrec = rec ? xstage + (size_t)n * K * NR * DI : nullptr;
  float* hrec = rec ? hstep + (size_t)n * K : nullptr;
  int* irec = rec ? iend + (size_t)n * (T - 1) : nullptr;
  float* trec = DENSE && rec ? theta + (size_t)n * (T - 1) : nullptr;
  if (wr) store_state<DI>(out, y, lane);
  ode_rhs<EV, DI, DO, ORDER>(ev, y, kv);
  put_row<DI>(kst, kv);
  int nacc = 0, nrej = 0, status = 0, nfe = 1, t = 0;
  float h = 0.f, tn = 0.f;                           // tn (dense): time reached, as an offset from ts[0]
  int jout = 1;                                      // dense: the first output not yet written
  bool after_reject = false;
  if (T > 1) {
    const float d0 = scaled_rms<DI>(y, y, y, rtol, atol), d1 = scaled_rms<DI>(kv, y, y, rtol, atol);
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
    const float h1 = d1 <= 1e-15f ? fmaxf(1e-6f, h0 * 1e-3f) : powf(0.01f / d1, 0.2f);
    h = uni(fminf(fminf(100.f * h0, h1), ts[DENSE ? T - 1 : 1] - ts[0]));
  }
  if constexpr (DENSE) {
    for (int i = 0; i + 1 < T; ++i)
      if (!(ts[i + 1] - ts[i] > 0.f)) status = 3;
    if (status) t = T;                               // nothing is integrated
  }
  for (; t + 1 < T; ++t) {
    const float t0 = ts[t], t1 = ts[DENSE ? T - 1 : t + 1];
    const float dt = t1 - t0, tabs = fmaxf(fabsf(t0), fabsf(t1));
    if (!(dt > 0.f)) { status = 3; break; }
    float rem = dt;
    while (true) {
      if (nacc >= K) { status = 1; break; }
      const bool cut = 1.01f * h >= rem;
      const float hs = cut ? rem : h;
      if (!(hs > 16.f * 1.1920929e-7f * fmaxf(tabs, fabsf(hs)))) { status = 2; break; }   // also a NaN step
      if (rec) store_state<DI>(xrec + (size_t)(nacc * NR) * DI, y, lane);
      for (int s = 1; s < 7; ++s) {
        float acc[DI];
#pragma unroll
        for (int d = 0; d < DI; ++d) acc[d] = 0.f;
        for (int j = 0; j < s; ++j) {
          const float c = dp_a[s][j];
#pragma unroll
          for (int d = 0; d < DI; ++d) acc[d] = fmaf(c, kst[j * KP + d], acc[d]);
        }
#pragma unroll
        for (int d = 0; d < DI; ++d) xs[d] = fmaf(hs, acc[d], y[d]);
        if (rec && s < NR) store_state<DI>(xrec + (size_t)(nacc * NR + s) * DI, xs, lane);
        ode_rhs<EV, DI, DO, ORDER>(ev, xs, kv);
        put_row<DI>(kst + s * KP, kv);
      }
      nfe += 6;
      // xs = the 5th-order solution, kv = its slope
      float err[DI];
#pragma unroll
      for (int d = 0; d < DI; ++d) err[d] = 0.f;
      for (int j = 0; j < 7; ++j) {
        const float c = dp_e[j];
#pragma unroll
        for (int d = 0; d < DI; ++d) err[d] = fmaf(c, kst[j * KP + d], err[d]);
      }
#pragma unroll
      for (int d = 0; d < DI; ++d) err[d] *= hs;
      const float ratio = uni(scaled_rms<DI>(err, y, xs, rtol, atol));
      float fac = uni(fminf(fmaxf(0.9f * powf(ratio, -0.2f), 0.2f), 10.f));   // ratio 0 -> 10; NaN -> 0.2
      if (ratio <= 1.f) {
        if (after_reject) fac = fminf(fac, 1.f);
        after_reject = false;
        if constexpr (DENSE) {
          // the outputs this step holds: every one up to its end point, all that are left when it is the cut step; rows 0..6 of
          // the slope block are k_1..k_7 of this step, y its start
          const float tnew = tn + hs;
          while (jout < T) {
            const float to = uni(ts[jout] - t0);
            if (!(cut || to <= tnew)) break;
            const bool last = jout == T - 1;
            const float th = last ? 1.f : uni(fminf(fmaxf((to - tn) / hs, 1.1920929e-7f), 1.f));
            if (wr) {
              if (last) {
                store_state<DI>(out + (size_t)jout * DI, xs, lane);
              } else {
                float acc[DI], z[DI];
#pragma unroll
                for (int d = 0; d < DI; ++d) acc[d] = 0.f;
                for (int j = 0; j < 7; ++j) {
                  const float c = dense_w(j, th);
#pragma unroll
                  for (int d = 0; d < DI; ++d) acc[d] = fmaf(c, kst[j * KP + d], acc[d]);
                }
#pragma unroll
                for (int d = 0; d < DI; ++d) z[d] = fmaf(hs, acc[d], y[d]);
                store_state<DI>(out + (size_t)jout * DI, z, lane);
              }
              if (rec && lane == 0) { irec[jout - 1] = nacc + 1; trec[jout - 1] = th; }
            }
            ++jout;
          }
          tn = tnew;
        }
#pragma unroll
        for (int d = 0; d < DI; ++d) y[d] = xs[d];
        put_row<DI>(kst, kv);
        if (rec && lane == 0) hrec[nacc] = hs;
        ++nacc;
        h = cut ? fmaxf(h, hs * fac) : hs * fac;
        if (cut) break;
        if constexpr (DENSE) rem = dt - tn;
        else rem -= hs;
      } else {
        ++nrej;
        after_reject = true;
        h = hs * fac;
      }
    }
    if (status) break;
    if constexpr (DENSE) break;                      // the one interval is done, its outputs are written
    if (wr) store_state<DI>(out + (size_t)(t + 1) * DI, y, lane);
    if (rec && lane == 0) irec[t] = nacc;
  }
  if (status && wr) {                                // a failed trajectory: NaN from the output it did not reach
    const float qnan = __int_as_float(0x7fc00000);
    const int first = DENSE ? jout : t + 1;
    for (int i = first * DI + lane; i < T * DI; i += 64) out[i] = qnan;
    if (rec) for (int i = first - 1 + lane; i < T - 1; i += 64) {
      irec[i] = nacc;
      if constexpr (DENSE) trec[i] = 1.f;
    }
  }
  if (rec) {                                         // rows past the count (and what a rejected attempt left there) are zero
    for (size_t i = (size_t)nacc * NR * DI + lane; i < (size_t)K * NR * DI; i += 64) xrec[i] = 0.f;
    for (int i = nacc + lane; i < K; i += 64) hrec[i] = 0.f;
  }
  if (wr && lane == 0) {
    int* c = counts + (size_t)n * 4;
    c[0] = nacc; c[1] = nrej; c[2] = status; c[3] = nfe;
  }
}

// blockIdx.y = Monte-Carlo draw: its own pack, the shared initial states (z0_stride = 0) or its own slab of them, its own
// trajectories and record.  Every offset is a scalar: blockIdx.y is.
#define GP_ADAPT_DRAW_POINTERS                                                                                   \
  const size_t dr = blockIdx.y, NT = (size_t)a.N;                                                                \
  const float* pack = a.pack + dr * a.pack_stride;                                                               \
  const float* z0 = a.z0 + dr * a.z0_stride;                                                                     \
  float* zt = a.zt + dr * NT * a.T * DI;                                                                         \
  float* xstage = a.xstage ? a.xstage + dr * NT * a.K * (DENSE ? NDEN : NREC) * DI : nullptr;                    \
  float* hstep = a.xstage ? a.hstep + dr * NT * a.K : nullptr;                                                   \
  int* iend = a.xstage ? a.iend + dr * NT * (a.T - 1) : nullptr;                                                 \
  float* theta = nullptr;                                                                                        \
  if constexpr (DENSE) theta = a.xstage ? a.theta + dr * NT * (a.T - 1) : nullptr;                               \
  int* counts = a.counts + dr * NT * 4;

// One wavefront per trajectory.  The (up to four) wavefronts of a workgroup take different numbers of steps: after the pack is
// staged there is no workgroup barrier.
template <class EV, int DI, int DO, int ORDER, bool USE_LDS, bool DENSE>
__global__ __launch_bounds__(256) void rollout_adaptive_kernel(AdaptFwdArg<DENSE> a, size_t lds_f4) {
  static_assert(DI == ORDER * DO && DI <= KP, "state dim = order * D_out");
  __shared__ float kst[4][7 * KP];
  GP_ADAPT_DRAW_POINTERS
  if (USE_LDS) stage_pack_lds(pack, lds_f4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  EV ev;
  ev.init(pack, a.M, a.S, lane);
  for (int n = blockIdx.x * wpb + wave; n < a.N; n += gridDim.x * wpb)
    dopri5_trajectory<EV, DI, DO, ORDER, DENSE>(ev, a, z0, zt, xstage, hstep, iend, theta, counts, n, kst[wave], true, lane,
                                                ts_row(a.ts, n, a.ts_stride));
}

// One workgroup per trajectory.  Every evaluation carries the team's barrier, so the four wavefronts must take the same steps:
// they do, the controller's inputs are the combined slopes, which every wavefront sums from the same LDS slots in the same order.
template <class EV, int DI, int DO, int ORDER, bool DENSE>
__global__ __launch_bounds__(64 * EV::kTeam) void rollout_adaptive_team_kernel(AdaptFwdArg<DENSE> a) {
  static_assert(DI == ORDER * DO && DI <= KP, "state dim = order * D_out");
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  __shared__ float kst[EV::kTeam][7 * KP];
  GP_ADAPT_DRAW_POINTERS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, a.M, a.S, slots, wave, lane);
  for (int n = blockIdx.x; n < a.N; n += gridDim.x)
    dopri5_trajectory<EV, DI, DO, ORDER, DENSE>(ev, a, z0, zt, xstage, hstep, iend, theta, counts, n, kst[wave], wave == 0, lane,
                                                ts_row(a.ts, n, a.ts_stride));
}

// Reverse sweep: the adjoint of an explicit Runge-Kutta step, over the recorded accepted steps, step sizes constant.
//   y1 = y + h sum_j b_j k_j,  k_j = F(x_j),  x_j = y + h sum_{l<j} a_jl k_l      (j = 0..5; b_6 = 0)
//   ak_j = h b_j lam;  for j = 5..0: g = J_F(x_j)^T ak_j, lam' += g, ak_l += h a_jl g (l < j);  lam <- lam + sum g
// gzt[:, t] enters before the step that ended on ts[t] is undone (iend[t-1] = its number).  The slope adjoints live in LDS like
// the slopes of the forward pass.  Sequential per trajectory, no atomics: deterministic.
template <class EV, int DI, int DO, int ORDER>
__global__ __launch_bounds__(64 * EV::kTeam) void rollout_adaptive_bwd_kernel(AdaptBwd a) {
  static_assert(DI == ORDER * DO && DI <= KP, "state dim = order * D_out");
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  __shared__ float akst[EV::kTeam][NREC * KP];
  const size_t dr = blockIdx.y, NT = (size_t)a.N;
  const int T = a.T, K = a.K;
  const float* pack = a.pack + dr * a.pack_stride;
  const float* xstage = a.xstage + dr * NT * K * NREC * DI;
  const float* hstep = a.hstep + dr * NT * K;
  const int* iend = a.iend + dr * NT * (T - 1);
  const float* gzt = a.gzt + dr * NT * T * DI;
  float* gz0 = a.gz0 + dr * NT * DI;
  float* astage = a.astage + dr * NT * K * NREC * DO;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ak = akst[wave];
  EV ev;
  ev.init(pack, a.M, a.S, slots, wave, lane);
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    const float* gz = gzt + (size_t)n * T * DI;
    const int* ie = iend + (size_t)n * (T - 1);
    int nacc = T > 1 ? __builtin_amdgcn_readfirstlane(ie[T - 2]) : 0;
    nacc = nacc < 0 ? 0 : (nacc > K ? K : nacc);
    float lam[DI];
#pragma unroll
    for (int d = 0; d < DI; ++d) lam[d] = 0.f;
    int tq = T - 2;                                  // outputs tq + 1 and below still wait for their gradient
    for (int i = nacc;; --i) {
      while (tq >= 0 && __builtin_amdgcn_readfirstlane(ie[tq]) >= i) {
#pragma unroll
        for (int d = 0; d < DI; ++d) lam[d] += gz[(size_t)(tq + 1) * DI + d];
        --tq;
      }
      if (i == 0) break;
      const size_t row = (size_t)n * K + (i - 1);
      const float hs = uni(hstep[row]);
      const float* xr = xstage + row * NREC * DI;
      float* ar = astage + row * NREC * DO;
      for (int j = 0; j < NREC; ++j) {
        const float c = hs * dp_a[6][j];
#pragma unroll
        for (int d = 0; d < DI; ++d) ak[j * KP + d] = c * lam[d];
      }
      for (int j = NREC - 1; j >= 0; --j) {
        float x[DI], aj[DI], g[DI], af[DO];
#pragma unroll
        for (int d = 0; d < DI; ++d) { x[d] = xr[j * DI + d]; aj[d] = ak[j * KP + d]; }
        ode_vjp<EV, DI, DO, ORDER>(ev, x, aj, g, af);
        if (wave == 0) store_state<DO>(ar + j * DO, af, lane);
#pragma unroll
        for (int d = 0; d < DI; ++d) lam[d] += g[d];
        for (int l = 0; l < j; ++l) {
          const float c = hs * dp_a[j][l];
#pragma unroll
          for (int d = 0; d < DI; ++d) ak[l * KP + d] = fmaf(c, g[d], ak[l * KP + d]);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < DI; ++d) lam[d] += gz[d];
    if (wave == 0) {
      store_state<DI>(gz0 + (size_t)n * DI, lam, lane);
      float* az = astage + (size_t)n * K * NREC * DO;
      for (size_t i = (size_t)nacc * NREC * DO + lane; i < (size_t)K * NREC * DO; i += 64) az[i] = 0.f;
    }
  }
}

// Reverse sweep of the dense mode.  The outputs o a step holds add their interpolation weights to the slope adjoints:
//   G0 = sum_o g_o,  S_j = h sum_o w_j(theta_o) g_o  (j = 0..6);  w_6(1) = 0, so the seventh slope is differentiated only where a step
//   holds an output with theta < 1:  lam += J_F(x_6)^T S_6  (x_6 = y_{n+1}, lam = the adjoint of y_{n+1})
//   ak_j = h b_j lam + S_j (j = 0..5);  the stage loop of the landing sweep;  lam += G0
// astage has 7 rows per step; row 6 is zero where the step holds no interior output.  The branch on that is scalar and the same in
// the four wavefronts of a team (theta is read from memory), as the evaluation behind it carries the team's barrier.
template <class EV, int DI, int DO, int ORDER>
__global__ __launch_bounds__(64 * EV::kTeam) void rollout_dense_bwd_kernel(AdaptBwdDense a) {
  static_assert(DI == ORDER * DO && DI <= KP, "state dim = order * D_out");
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  __shared__ float akst[EV::kTeam][NDEN * KP];
  const size_t dr = blockIdx.y, NT = (size_t)a.N;
  const int T = a.T, K = a.K;
  const float* pack = a.pack + dr * a.pack_stride;
  const float* xstage = a.xstage + dr * NT * K * NDEN * DI;
  const float* hstep = a.hstep + dr * NT * K;
  const int* istep = a.iend + dr * NT * (T - 1);
  const float* theta = a.theta + dr * NT * (T - 1);
  const float* gzt = a.gzt + dr * NT * T * DI;
  float* gz0 = a.gz0 + dr * NT * DI;
  float* astage = a.astage + dr * NT * K * NDEN * DO;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ak = akst[wave];
  EV ev;
  ev.init(pack, a.M, a.S, slots, wave, lane);
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    const float* gz = gzt + (size_t)n * T * DI;
    const int* is = istep + (size_t)n * (T - 1);
    const float* th = theta + (size_t)n * (T - 1);
    int nacc = T > 1 ? __builtin_amdgcn_readfirstlane(is[T - 2]) : 0;
    nacc = nacc < 0 ? 0 : (nacc > K ? K : nacc);
    float lam[DI];
#pragma unroll
    for (int d = 0; d < DI; ++d) lam[d] = 0.f;
    int tq = T - 2;                                  // outputs tq + 1 and below still wait for their gradient
    for (int i = nacc; i >= 1; --i) {
      const size_t row = (size_t)n * K + (i - 1);
      const float hs = uni(hstep[row]);
      const float* xr = xstage + row * NDEN * DI;
      float* ar = astage + row * NDEN * DO;
      float g0[DI];
#pragma unroll
      for (int d = 0; d < DI; ++d) g0[d] = 0.f;
      for (int j = 0; j < NDEN; ++j) {
#pragma unroll
        for (int d = 0; d < DI; ++d) ak[j * KP + d] = 0.f;
      }
      bool interior = false;
      while (tq >= 0 && __builtin_amdgcn_readfirstlane(is[tq]) >= i) {
        const float t = uni(fminf(fmaxf(th[tq], 0.f), 1.f));
        interior = interior || t < 1.f;
        float g[DI];
#pragma unroll
        for (int d = 0; d < DI; ++d) { g[d] = gz[(size_t)(tq + 1) * DI + d]; g0[d] += g[d]; }
        for (int j = 0; j < NDEN; ++j) {
          const float c = hs * dense_w(j, t);
#pragma unroll
          for (int d = 0; d < DI; ++d) ak[j * KP + d] = fmaf(c, g[d], ak[j * KP + d]);
        }
        --tq;
      }
      if (interior) {
        float x[DI], aj[DI], g[DI], af[DO];
#pragma unroll
        for (int d = 0; d < DI; ++d) { x[d] = xr[(NDEN - 1) * DI + d]; aj[d] = ak[(NDEN - 1) * KP + d]; }
        ode_vjp<EV, DI, DO, ORDER>(ev, x, aj, g, af);
        if (wave == 0) store_state<DO>(ar + (NDEN - 1) * DO, af, lane);
#pragma unroll
        for (int d = 0; d < DI; ++d) lam[d] += g[d];
      } else if (wave == 0 && lane < DO) {
        ar[(NDEN - 1) * DO + lane] = 0.f;
      }
      for (int j = 0; j < NREC; ++j) {
        const float c = hs * dp_a[6][j];
#pragma unroll
        for (int d = 0; d < DI; ++d) ak[j * KP + d] = fmaf(c, lam[d], ak[j * KP + d]);
      }
      for (int j = NREC - 1; j >= 0; --j) {
        float x[DI], aj[DI], g[DI], af[DO];
#pragma unroll
        for (int d = 0; d < DI; ++d) { x[d] = xr[j * DI + d]; aj[d] = ak[j * KP + d]; }
        ode_vjp<EV, DI, DO, ORDER>(ev, x, aj, g, af);
        if (wave == 0) store_state<DO>(ar + j * DO, af, lane);
#pragma unroll
        for (int d = 0; d < DI; ++d) lam[d] += g[d];
        for (int l = 0; l < j; ++l) {
          const float c = hs * dp_a[j][l];
#pragma unroll
          for (int d = 0; d < DI; ++d) ak[l * KP + d] = fmaf(c, g[d], ak[l * KP + d]);
        }
      }
#pragma unroll
      for (int d = 0; d < DI; ++d) lam[d] += g0[d];
    }
    for (; tq >= -1; --tq) {                         // the initial state, and what a record without steps attributes to it
#pragma unroll
      for (int d = 0; d < DI; ++d) lam[d] += gz[(size_t)(tq + 1) * DI + d];
    }
    if (wave == 0) {
      store_state<DI>(gz0 + (size_t)n * DI, lam, lane);
      float* az = astage + (size_t)n * K * NDEN * DO;
      for (size_t i = (size_t)nacc * NDEN * DO + lane; i < (size_t)K * NDEN * DO; i += 64) az[i] = 0.f;
    }
  }
}

// ----------------------------------------------------------------------------------------------
// host side: the evaluators and grids of the fixed-grid rollout and of its reverse sweep (forward_route, reverse_route of gp_rollout.hpp)
// ----------------------------------------------------------------------------------------------
template <bool DENSE>
static int adaptive_fwd(int kernel, int order, int Di, int Do, const AdaptFwdArg<DENSE>& a, int nd, hipStream_t st) {
  static const char* const who = "gpode_rollout_adaptive_fwd";
  // the wave routes report the family alone
  static const char* const tags[2][kRoutes] = {
      {"rollout_adaptive_rbf_team", "rollout_adaptive_rbf_team_stream", "rollout_adaptive_rbf", "rollout_adaptive_rbf", "rollout_adaptive_rbf"},
      {"rollout_adaptive_df_team", "rollout_adaptive_df_team_stream", "rollout_adaptive_df", "rollout_adaptive_df"}};
  if (kernel != 0 && order != 1) return set_error("gpode_rollout_adaptive_fwd: DF kernel is first-order only (kernels.py:259-262)");
  return dispatch_dims(who, kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return dispatch_order<DI, DO>(who, order, [&](auto o) {
      constexpr int ORDER = decltype(o)::value;
      return forward_route<KERNEL, DI, DO>(a.N, a.M, a.S, [&](auto ev, auto map, const LaunchGeom& g) {
        using EV = typename decltype(ev)::type;
        constexpr int MAP = decltype(map)::value;
        if constexpr (MAP == kTeam) {
          if (launch_route(rollout_adaptive_team_kernel<EV, DI, DO, ORDER, DENSE>, g, nd, st, a)) return 1;
        } else {
          if (launch_route(rollout_adaptive_kernel<EV, DI, DO, ORDER, MAP == kWaveLds, DENSE>, g, nd, st, a, g.lds_f4)) return 1;
        }
        return check_launch(tags[KERNEL][g.route]);
      });
    });
  });
}

// What the kernels take, from the entry point's arguments: the draws' packs pack_floats apart, z0 a slab per draw or shared.
template <bool DENSE> static AdaptFwdArg<DENSE> adapt_fwd_arg(const AdaptFwdArgs& a, int Di, size_t pack_floats) {
  const AdaptFwd base{a.pack, pack_floats, a.M, a.S, a.z0, a.ts, a.N, a.T, a.K, a.rtol, a.atol, a.zt, a.xstage, a.hstep, a.index, a.counts};
  const size_t z0_stride = a.z0_per_draw ? (size_t)a.N * Di : 0, ts_stride = a.ts_per_traj ? (size_t)a.T : 0;
  if constexpr (DENSE) return {base, a.theta, z0_stride, ts_stride};
  else return {base, z0_stride, ts_stride};
}

int rollout_adaptive_fwd(int kernel, int order, int Di, int Do, const AdaptFwdArgs& a, bool dense, int nd, hipStream_t st) {
  size_t pf = 0;
  if (cache_sizes(kernel, Di, Do, a.M, a.S, &pf, nullptr)) return 1;
  // landing first, as the two have always been instantiated: the order decides the numbering of the object's local labels
  if (!dense) return adaptive_fwd<false>(kernel, order, Di, Do, adapt_fwd_arg<false>(a, Di, pf), nd, st);
  return adaptive_fwd<true>(kernel, order, Di, Do, adapt_fwd_arg<true>(a, Di, pf), nd, st);
}

// the reverse kernel of a mode
template <bool DENSE, class EV, int DI, int DO, int ORDER> static constexpr auto adaptive_bwd_kernel() {
  if constexpr (DENSE) return &rollout_dense_bwd_kernel<EV, DI, DO, ORDER>;
  else return &rollout_adaptive_bwd_kernel<EV, DI, DO, ORDER>;
}

template <bool DENSE>
static int adaptive_bwd(int kernel, int order, int Di, int Do, const AdaptBwdArg<DENSE>& a, int nd, hipStream_t st) {
  static const char* const who = "gpode_rollout_adaptive_bwd";
  static const char* const tags[2][2] = {{"rollout_adaptive_bwd_rbf", "rollout_adaptive_bwd_rbf_stream"},
                                         {"rollout_adaptive_bwd_df", "rollout_adaptive_bwd_df_stream"}};
  if (kernel != 0 && order != 1) return set_error("gpode_rollout_adaptive_bwd: DF kernel is first-order only");
  return dispatch_dims(who, kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return dispatch_order<DI, DO>(who, order, [&](auto o) {
      constexpr int ORDER = decltype(o)::value;
      return reverse_route<KERNEL, DI, DO>(a.N, a.M, a.S, [&](auto ev, const LaunchGeom& g) {
        using EV = typename decltype(ev)::type;
        if (launch_route(adaptive_bwd_kernel<DENSE, EV, DI, DO, ORDER>(), g, nd, st, a)) return 1;
        return check_launch(tags[KERNEL][g.route]);
      });
    });
  });
}

int rollout_adaptive_bwd(int kernel, int order, int Di, int Do, const AdaptBwdArgs& a, bool dense, int nd, hipStream_t st) {
  size_t pf = 0;
  if (cache_sizes(kernel, Di, Do, a.M, a.S, &pf, nullptr)) return 1;
  const AdaptBwd base{a.pack, pf, a.M, a.S, a.xstage, a.hstep, a.index, a.gzt, a.N, a.T, a.K, a.gz0, a.astage};
  if (!dense) return adaptive_bwd<false>(kernel, order, Di, Do, base, nd, st);
  return adaptive_bwd<true>(kernel, order, Di, Do, AdaptBwdDense{base, a.theta}, nd, st);
}

}  // namespace gp
