// gp_forward.hip -- f(x) evaluation and the persistent fixed-grid rollout (forward).
//
// Replaces, per MC draw: SVGP_Layer.forward (svpy.py:123-142) and the whole torchdiffeq solver loop
// behind Flow.forward (flow.py:68-86): T-1 steps x {1|4} RHS evaluations collapse into ONE launch in
// which each wavefront carries one trajectory from z0 to z_{T-1}.
//
// Variants
//   RBF "reg"    : the wave's slice of the packed cache (omega/phase/weights, Z, nu) is loaded once
//                  into VGPRs (cfg1: 216 floats per lane) and reused for all 4(T-1) evaluations.
//   RBF "stream" : any S, M: records are re-read from L2 each evaluation.
//   DF  "lds"    : the pack (cfg2: 98 KB) is staged once per workgroup in LDS, read with ds_read_b128.
//   DF  "stream" : pack larger than LDS (cfg5): records are re-read from L2.
#include "gp_rollout.hpp"

namespace gp {

// ----------------------------------------------------------------------------------------------
// kernels
// ----------------------------------------------------------------------------------------------
// x (N,DI) -> f (N,DO); one wave per row, grid-stride over rows.
template <class EV, int DI, int DO, bool USE_LDS>
__global__ __launch_bounds__(256) void rhs_kernel(const float* __restrict__ pack, int M, int S, size_t lds_f4,
                           const float* __restrict__ x, int N, float* __restrict__ f, int mode, Draws dw) {
  pack += blockIdx.y * dw.pack; x += blockIdx.y * dw.in; f += blockIdx.y * dw.out;      // blockIdx.y = Monte-Carlo draw
  if (USE_LDS) stage_pack_lds(pack, lds_f4);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  EV ev;
  ev.init(pack, M, S, lane);
  for (int n = blockIdx.x * wpb + wave; n < N; n += gridDim.x * wpb) {
    float xv[DI], fv[DO];
#pragma unroll
    for (int i = 0; i < DI; ++i) xv[i] = x[(size_t)n * DI + i];
    if (mode == 0) ev.template eval<0>(xv, fv);
    else if (mode == 1) ev.template eval<1>(xv, fv);
    else ev.template eval<2>(xv, fv);
    if (lane < DO) {
      float v = fv[0];
#pragma unroll
      for (int d = 1; d < DO; ++d) v = (lane == d) ? fv[d] : v;
      f[(size_t)n * DO + lane] = v;
    }
  }
}


// z0 (N,DI), ts (T) or (N,T) [dw.ts = T] -> zt (N,T,DI).  One wave per trajectory, persistent over the T-1 output intervals, each
// taken in one step (SUB = false: the kernel as it always was) or in dw.sub equal steps (xstage: (N, T-1, sub, NS, DI), the stage inputs of every step).
// Stage algebra follows torchdiffeq's fixed-grid solvers at flow.py:76-85 (3/8-rule rk4).
template <class EV, int DI, int DO, int ORDER, int METHOD, bool USE_LDS, bool SUB>
__global__ __launch_bounds__(256) void rollout_kernel(const float* __restrict__ pack, int M, int S, size_t lds_f4,
                               const float* __restrict__ z0, const float* __restrict__ ts, int N, int T,
                               float* __restrict__ zt, float* __restrict__ xstage, Draws dw) {
  static_assert(DI == ORDER * DO, "state dim = order * D_out");
  constexpr int NS = stages_of(METHOD);
  pack += blockIdx.y * dw.pack; z0 += blockIdx.y * dw.in; zt += blockIdx.y * dw.out;    // blockIdx.y = Monte-Carlo draw
  if (xstage) xstage += blockIdx.y * dw.out2;
  if (USE_LDS) stage_pack_lds(pack, lds_f4);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  EV ev;
  ev.init(pack, M, S, lane);
  const float third = (float)(1.0 / 3.0);
  const int sub = sub_count<SUB>(dw.sub);
  for (int n = blockIdx.x * wpb + wave; n < N; n += gridDim.x * wpb) {
    float y[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) y[i] = z0[(size_t)n * DI + i];
    float* out = zt + (size_t)n * T * DI;
    float* xs_out = xstage ? xstage + (size_t)n * (T - 1) * sub * NS * DI : nullptr;
    store_state<DI>(out, y, lane);
    const float* tn = ts_row(ts, n, dw.ts);
    for (int t = 0; t + 1 < T; ++t) {
      const float dt = sub_step<SUB>(tn[t], tn[t + 1], sub);
      for (int r = t * sub; r < (t + 1) * sub; ++r) {   // r: the step's row block of the record, (T-1, sub, NS, DI)
        float k1[DI];
        if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS) * DI, y, lane);
        ode_rhs<EV, DI, DO, ORDER>(ev, y, k1);
        if (METHOD == 0) {
#pragma unroll
          for (int i = 0; i < DI; ++i) y[i] = y[i] + dt * k1[i];
        } else if (METHOD == 2) {                      // midpoint: y1 = y + dt f(y + dt/2 f(y))
          float k2[DI], xs[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + 0.5f * dt * k1[i];
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 1) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k2);
#pragma unroll
          for (int i = 0; i < DI; ++i) y[i] = y[i] + dt * k2[i];
        } else {
          float k2[DI], k3[DI], k4[DI], xs[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + dt * k1[i] * third;
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 1) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k2);
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + dt * (k2[i] - k1[i] * third);
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 2) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k3);
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + dt * (k1[i] - k2[i] + k3[i]);
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 3) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k4);
#pragma unroll
          for (int i = 0; i < DI; ++i) y[i] = y[i] + (k1[i] + 3.f * (k2[i] + k3[i]) + k4[i]) * dt * 0.125f;
        }
      }
      store_state<DI>(out + (size_t)(t + 1) * DI, y, lane);
    }
  }
}

template <class EV, int DI, int DO>
__global__ __launch_bounds__(64 * EV::kTeam) void rhs_team_kernel(const float* __restrict__ pack, int M, int S,
                                                        const float* __restrict__ x, int N, float* __restrict__ f, int mode, Draws dw) {
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  pack += blockIdx.y * dw.pack; x += blockIdx.y * dw.in; f += blockIdx.y * dw.out;      // blockIdx.y = Monte-Carlo draw
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    float xv[DI], fv[DO];
#pragma unroll
    for (int i = 0; i < DI; ++i) xv[i] = x[(size_t)n * DI + i];
    if (mode == 0) ev.template eval<0>(xv, fv);
    else if (mode == 1) ev.template eval<1>(xv, fv);
    else ev.template eval<2>(xv, fv);
    if (wave == 0 && lane < DO) {
      float v = fv[0];
#pragma unroll
      for (int d = 1; d < DO; ++d) v = (lane == d) ? fv[d] : v;
      f[(size_t)n * DO + lane] = v;
    }
  }
}


template <class EV, int DI, int DO, int ORDER, int METHOD, bool SUB>
__global__ __launch_bounds__(64 * EV::kTeam) void rollout_team_kernel(const float* __restrict__ pack, int M, int S,
                                                            const float* __restrict__ z0, const float* __restrict__ ts,
                                                            int N, int T, float* __restrict__ zt, float* __restrict__ xstage, Draws dw) {
  static_assert(DI == ORDER * DO, "state dim = order * D_out");
  constexpr int NS = stages_of(METHOD);
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  // blockIdx.y = Monte-Carlo draw: its own pack (function draw), the shared initial states, its own trajectories
  pack += blockIdx.y * dw.pack; z0 += blockIdx.y * dw.in; zt += blockIdx.y * dw.out;
  if (xstage) xstage += blockIdx.y * dw.out2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  const float third = (float)(1.0 / 3.0);
  const int sub = sub_count<SUB>(dw.sub);
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    float y[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) y[i] = z0[(size_t)n * DI + i];
    float* out = zt + (size_t)n * T * DI;
    float* xs_out = (xstage && wave == 0) ? xstage + (size_t)n * (T - 1) * sub * NS * DI : nullptr;
    if (wave == 0) store_state<DI>(out, y, lane);
    const float* tn = ts_row(ts, n, dw.ts);
    for (int t = 0; t + 1 < T; ++t) {
      const float dt = sub_step<SUB>(tn[t], tn[t + 1], sub);
      for (int r = t * sub; r < (t + 1) * sub; ++r) {   // r: the step's row block of the record, (T-1, sub, NS, DI)
        float k1[DI];
        if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS) * DI, y, lane);
        ode_rhs<EV, DI, DO, ORDER>(ev, y, k1);
        if (METHOD == 0) {
#pragma unroll
          for (int i = 0; i < DI; ++i) y[i] = y[i] + dt * k1[i];
        } else if (METHOD == 2) {                      // midpoint
          float k2[DI], xs[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + 0.5f * dt * k1[i];
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 1) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k2);
#pragma unroll
          for (int i = 0; i < DI; ++i) y[i] = y[i] + dt * k2[i];
        } else {
          float k2[DI], k3[DI], k4[DI], xs[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + dt * k1[i] * third;
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 1) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k2);
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + dt * (k2[i] - k1[i] * third);
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 2) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k3);
#pragma unroll
          for (int i = 0; i < DI; ++i) xs[i] = y[i] + dt * (k1[i] - k2[i] + k3[i]);
          if (xs_out) store_state<DI>(xs_out + (size_t)(r * NS + 3) * DI, xs, lane);
          ode_rhs<EV, DI, DO, ORDER>(ev, xs, k4);
#pragma unroll
          for (int i = 0; i < DI; ++i) y[i] = y[i] + (k1[i] + 3.f * (k2[i] + k3[i]) + k4[i]) * dt * 0.125f;
        }
      }
      if (wave == 0) store_state<DI>(out + (size_t)(t + 1) * DI, y, lane);
    }
  }
}


// The evaluator and the grid of either entry point come from forward_route (gp_rollout.hpp); what is left here is the kernel
// template, its arguments and the tag per route, in the order of LaunchGeom::route.
int rhs_fwd(int kernel, int Di, int Do, int M, int S, const float* pack, const float* x, int N, float* f, int mode, hipStream_t st, Draws dw) {
  static const char* const tags[2][kRoutes] = {{"rhs_rbf_team", "rhs_rbf_team_stream", "rhs_rbf_reg42", "rhs_rbf_reg11", "rhs_rbf_stream"},
                                               {"rhs_df_team", "rhs_df_team_stream", "rhs_df_lds", "rhs_df_stream"}};
  return dispatch_dims("gpode_rhs_fwd", kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return forward_route<KERNEL, DI, DO>(N, M, S, [&](auto ev, auto map, const LaunchGeom& g) {
      using EV = typename decltype(ev)::type;
      constexpr int MAP = decltype(map)::value;
      if constexpr (MAP == kTeam) {
        if (launch_route(rhs_team_kernel<EV, DI, DO>, g, dw.nd, st, pack, M, S, x, N, f, mode, dw)) return 1;
      } else {
        if (launch_route(rhs_kernel<EV, DI, DO, MAP == kWaveLds>, g, dw.nd, st, pack, M, S, g.lds_f4, x, N, f, mode, dw)) return 1;
      }
      return check_launch(tags[KERNEL][g.route]);
    });
  });
}

// What rollout_kernel / rollout_team_kernel read of Draws: in = z0 (0: shared by the draws), out = zt, out2 = xstage.
static Draws rollout_fwd_draws(int method, int Di, const RolloutFwdArgs& a, int nd, size_t pack_floats) {
  Draws d;
  d.nd = nd; d.pack = pack_floats;
  d.in = a.z0_per_draw ? (size_t)a.N * Di : 0;
  d.out = (size_t)a.N * a.T * Di; d.out2 = record_rows(a.N, a.T, a.substeps, method) * Di;
  d.ts = a.ts_per_traj ? (size_t)a.T : 0; d.sub = a.substeps;
  return d;
}

int rollout_fwd(int kernel, int order, int method, int Di, int Do, const RolloutFwdArgs& a, int nd, hipStream_t st) {
  static const char* const who = "gpode_rollout_fwd";
  static const char* const tags[2][kRoutes] = {
      {"rollout_rbf_team", "rollout_rbf_team_stream", "rollout_rbf_reg42", "rollout_rbf_reg11", "rollout_rbf_stream"},
      {"rollout_df_team", "rollout_df_team_stream", "rollout_df_lds", "rollout_df_stream"}};
  size_t pf = 0;
  if (cache_sizes(kernel, Di, Do, a.M, a.S, &pf, nullptr)) return 1;
  if (method < 0 || method > 2) return set_error("gpode_rollout_fwd: method %d (0 euler, 1 rk4, 2 midpoint; 3 dopri5: gpode_rollout_adaptive_fwd_n)", method);
  if (kernel != 0 && order != 1) return set_error("gpode_rollout_fwd: DF kernel is first-order only (kernels.py:259-262)");
  const Draws dw = rollout_fwd_draws(method, Di, a, nd, pf);
  return dispatch_dims(who, kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return dispatch_order<DI, DO>(who, order, [&](auto o) {
      return dispatch_method(method, [&](auto m) {
        constexpr int ORDER = decltype(o)::value, METHOD = decltype(m)::value;
        return forward_route<KERNEL, DI, DO>(a.N, a.M, a.S, [&](auto ev, auto map, const LaunchGeom& g) {
          using EV = typename decltype(ev)::type;
          constexpr int MAP = decltype(map)::value;
          return dispatch_substeps(dw.sub, [&](auto sb) {
            constexpr bool SUB = decltype(sb)::value;
            if constexpr (MAP == kTeam) {
              if (launch_route(rollout_team_kernel<EV, DI, DO, ORDER, METHOD, SUB>, g, nd, st, a.pack, a.M, a.S, a.z0, a.ts, a.N, a.T, a.zt, a.xstage, dw))
                return 1;
            } else {
              if (launch_route(rollout_kernel<EV, DI, DO, ORDER, METHOD, MAP == kWaveLds, SUB>, g, nd, st, a.pack, a.M, a.S, g.lds_f4, a.z0, a.ts,
                               a.N, a.T, a.zt, a.xstage, dw))
                return 1;
            }
            return check_launch(tags[KERNEL][g.route]);
          });
        });
      });
    });
  });
}

int dims_supported(int kernel, int Di, int Do) {
  return (kernel == 0 || kernel == 1) && for_dims(kernel, Di, Do, [](auto, auto, auto) { return 0; }) == 0;
}

}  // namespace gp
