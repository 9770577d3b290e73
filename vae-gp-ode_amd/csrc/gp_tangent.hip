// gp_tangent.hip -- forward-mode (tangent-linear) twins of rhs_fwd and of the fixed-grid rollout: J_f(x) v, and the state-transition
// matrix Phi_t = d z_t / d z0 applied to K directions.
//
// Mapping: one wavefront per (row, tangent column), rows * K of them on grid_for's grid, grid-stride beyond.  Every column of a row
// carries the row's primal state itself -- the same instruction sequence on the same inputs, so the copies agree bit for bit -- and
// column 0 writes it out.  The evaluators are the streamed ones (RbfStreamEval, DfEval<D, false>: records from L2, any M and S), through
// their jvp members: one pass over the records gives f and J_f v, one reduction carries both.
//
// rollout_jvp_kernel applies the derivative of the discrete step map of rollout_kernel (gp_forward.hip) -- the exact derivative of what
// that kernel computes and the transpose of what rollout_bwd applies, not a discretisation of the variational equation.  With F the
// right-hand side on the state and dF(x) dx = J_f(x) dx (order 1) or [dx[Do:], J_f(x) dx] (order 2):
//   euler     v+ = v + h dk1,                      dk1 = dF(y) v
//   midpoint  v+ = v + h dk2,                      dk2 = dF(y + h/2 k1) (v + h/2 dk1)
//   rk4 (3/8) tangent stage inputs v + h dk1/3, v + h (dk2 - dk1/3), v + h (dk1 - dk2 + dk3);  v+ = v + h (dk1 + 3 (dk2 + dk3) + dk4) / 8
// The steps per output interval are a run-time count in ONE instantiation: this is an analysis path, the microseconds that made the
// training rollout keep two do not matter here.
#include "gp_rollout.hpp"

namespace gp {

template <class EV, int DI, int DO, int ORDER>
__device__ __forceinline__ void ode_jvp(EV& ev, const float (&y)[DI], const float (&v)[DI], float (&dy)[DI], float (&dv)[DI]) {
  float fv[DO], jf[DO];
  ev.template jvp<0>(y, v, fv, jf);
  if (ORDER == 1) {
#pragma unroll
    for (int i = 0; i < DO; ++i) { dy[i] = fv[i]; dv[i] = jf[i]; }
  } else {
#pragma unroll
    for (int i = 0; i < DO; ++i) { dy[i] = y[DO + i]; dy[DO + i] = fv[i]; dv[i] = v[DO + i]; dv[DO + i] = jf[i]; }
  }
}

// wave-uniform row index, as a scalar: the row's operands are then scalar loads
__device__ __forceinline__ int uniform(int r) { return __builtin_amdgcn_readfirstlane(r); }

// x (R,DI), v (R,K,DI) or null (the identity, K == DI) -> f (R,DO) (may be null), jv (R,K,DO).  dw: in = x, in2 = v, out = f, out2 = jv
template <class EV, int DI, int DO>
__global__ __launch_bounds__(256) void rhs_jvp_kernel(const float* __restrict__ pack, int M, int S, const float* __restrict__ x,
                                                      const float* __restrict__ v, int R, int K, float* __restrict__ f,
                                                      float* __restrict__ jv, int mode, Draws dw) {
  pack += blockIdx.y * dw.pack; x += blockIdx.y * dw.in; jv += blockIdx.y * dw.out2;      // blockIdx.y = Monte-Carlo draw
  if (v) v += blockIdx.y * dw.in2;
  if (f) f += blockIdx.y * dw.out;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  EV ev;
  ev.init(pack, M, S, lane);
  const int rows = R * K;
  for (int rw = blockIdx.x * wpb + wave; rw < rows; rw += gridDim.x * wpb) {
    const int r = uniform(rw), n = r / K, k = r - n * K;
    float xv[DI], vv[DI], fv[DO], jf[DO];
#pragma unroll
    for (int i = 0; i < DI; ++i) {
      xv[i] = x[(size_t)n * DI + i];
      vv[i] = v ? v[(size_t)r * DI + i] : (i == k ? 1.f : 0.f);
    }
    if (mode == 0) ev.template jvp<0>(xv, vv, fv, jf);
    else if (mode == 1) ev.template jvp<1>(xv, vv, fv, jf);
    else ev.template jvp<2>(xv, vv, fv, jf);
    if (f && k == 0) store_state<DO>(f + (size_t)n * DO, fv, lane);
    store_state<DO>(jv + (size_t)r * DO, jf, lane);
  }
}

// z0 (N,DI), v0 (N,K,DI) or null (the identity, K == DI), ts (T) or (N,T) [dw.ts = T] -> zt (N,T,DI) (may be null), vt (N,T,K,DI).
// dw: in = z0, in2 = v0, out = zt, out2 = vt, sub = steps per output interval
template <class EV, int DI, int DO, int ORDER, int METHOD>
__global__ __launch_bounds__(256) void rollout_jvp_kernel(const float* __restrict__ pack, int M, int S, const float* __restrict__ z0,
                                                          const float* __restrict__ v0, int K, const float* __restrict__ ts, int N, int T,
                                                          float* __restrict__ zt, float* __restrict__ vt, Draws dw) {
  static_assert(DI == ORDER * DO, "state dim = order * D_out");
  pack += blockIdx.y * dw.pack; z0 += blockIdx.y * dw.in; vt += blockIdx.y * dw.out2;     // blockIdx.y = Monte-Carlo draw
  if (v0) v0 += blockIdx.y * dw.in2;
  if (zt) zt += blockIdx.y * dw.out;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  EV ev;
  ev.init(pack, M, S, lane);
  const float third = (float)(1.0 / 3.0);
  const int sub = dw.sub;
  const int rows = N * K;
  for (int rw = blockIdx.x * wpb + wave; rw < rows; rw += gridDim.x * wpb) {
    const int r = uniform(rw), n = r / K, k = r - n * K;
    float y[DI], v[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) {
      y[i] = z0[(size_t)n * DI + i];
      v[i] = v0 ? v0[(size_t)r * DI + i] : (i == k ? 1.f : 0.f);
    }
    float* zo = (zt && k == 0) ? zt + (size_t)n * T * DI : nullptr;    // column 0 writes the primal
    float* vo = vt + ((size_t)n * T * K + k) * DI;                     // row t of this column: + t K DI
    if (zo) store_state<DI>(zo, y, lane);
    store_state<DI>(vo, v, lane);
    const float* tn = ts_row(ts, n, dw.ts);
    for (int t = 0; t + 1 < T; ++t) {
      const float dt = sub_step<true>(tn[t], tn[t + 1], sub);
      for (int s = 0; s < sub; ++s) {
        float k1[DI], d1[DI];
        ode_jvp<EV, DI, DO, ORDER>(ev, y, v, k1, d1);
        if (METHOD == 0) {
#pragma unroll
          for (int i = 0; i < DI; ++i) { y[i] = y[i] + dt * k1[i]; v[i] = v[i] + dt * d1[i]; }
        } else if (METHOD == 2) {
          float k2[DI], d2[DI], xs[DI], dx[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) { xs[i] = y[i] + 0.5f * dt * k1[i]; dx[i] = v[i] + 0.5f * dt * d1[i]; }
          ode_jvp<EV, DI, DO, ORDER>(ev, xs, dx, k2, d2);
#pragma unroll
          for (int i = 0; i < DI; ++i) { y[i] = y[i] + dt * k2[i]; v[i] = v[i] + dt * d2[i]; }
        } else {
          // (Accumulating the stage sums as the stages arrive was tried for the width-16 instantiations and spilled more, not
          // less: the registers were going to the evaluator, and df_ind_jvp's two column halves are what removed the spills --
          // DESIGN 4.6b.)
          float k2[DI], k3[DI], k4[DI], d2[DI], d3[DI], d4[DI], xs[DI], dx[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) { xs[i] = y[i] + dt * k1[i] * third; dx[i] = v[i] + dt * d1[i] * third; }
          ode_jvp<EV, DI, DO, ORDER>(ev, xs, dx, k2, d2);
#pragma unroll
          for (int i = 0; i < DI; ++i) { xs[i] = y[i] + dt * (k2[i] - k1[i] * third); dx[i] = v[i] + dt * (d2[i] - d1[i] * third); }
          ode_jvp<EV, DI, DO, ORDER>(ev, xs, dx, k3, d3);
#pragma unroll
          for (int i = 0; i < DI; ++i) { xs[i] = y[i] + dt * (k1[i] - k2[i] + k3[i]); dx[i] = v[i] + dt * (d1[i] - d2[i] + d3[i]); }
          ode_jvp<EV, DI, DO, ORDER>(ev, xs, dx, k4, d4);
#pragma unroll
          for (int i = 0; i < DI; ++i) {
            y[i] = y[i] + (k1[i] + 3.f * (k2[i] + k3[i]) + k4[i]) * dt * 0.125f;
            v[i] = v[i] + (d1[i] + 3.f * (d2[i] + d3[i]) + d4[i]) * dt * 0.125f;
          }
        }
      }
      if (zo) store_state<DI>(zo + (size_t)(t + 1) * DI, y, lane);
      store_state<DI>(vo + (size_t)(t + 1) * K * DI, v, lane);
    }
  }
}

// the streamed wave evaluator of a family, and the floats of one draw's pack
template <int KERNEL, int DI, int DO> struct TangentEval {
  using type = std::conditional_t<KERNEL == 0, RbfStreamEval<DI, DO>, DfEval<DO, false>>;
  static size_t pack_floats(int M, int S) {
    if constexpr (KERNEL == 0) return RbfLayout<DI, DO>::total_floats(M, S);
    else return DfLayout<DO>::total_floats(M, S);
  }
};

int rhs_jvp(int kernel, int Di, int Do, const RhsJvpArgs& a, int nd, hipStream_t st) {
  static const char* const tags[2] = {"rhs_jvp_rbf_stream", "rhs_jvp_df_stream"};
  return dispatch_dims("gpode_rhs_jvp", kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    using TE = TangentEval<KERNEL, DI, DO>;
    Draws dw;
    dw.nd = nd; dw.pack = TE::pack_floats(a.M, a.S);
    dw.in = a.x_per_draw ? (size_t)a.R * DI : 0; dw.in2 = a.x_per_draw ? (size_t)a.R * a.K * DI : 0;
    dw.out = (size_t)a.R * DO; dw.out2 = (size_t)a.R * a.K * DO;
    int grid, block;
    grid_for(a.R * a.K, grid, block);
    hipLaunchKernelGGL((rhs_jvp_kernel<typename TE::type, DI, DO>), dim3(grid, nd), block, 0, st, a.pack, a.M, a.S, a.x, a.v, a.R, a.K, a.f,
                       a.jv, a.mode, dw);
    return check_launch(tags[KERNEL]);
  });
}

int rollout_jvp(int kernel, int order, int method, int Di, int Do, const RolloutJvpArgs& a, int nd, hipStream_t st) {
  static const char* const who = "gpode_rollout_jvp";
  static const char* const tags[2] = {"rollout_jvp_rbf_stream", "rollout_jvp_df_stream"};
  return dispatch_dims(who, kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return dispatch_order<DI, DO>(who, order, [&](auto o) {
      return dispatch_method(method, [&](auto m) {
        constexpr int ORDER = decltype(o)::value, METHOD = decltype(m)::value;
        using TE = TangentEval<KERNEL, DI, DO>;
        Draws dw;
        dw.nd = nd; dw.pack = TE::pack_floats(a.M, a.S);
        dw.in = a.z0_per_draw ? (size_t)a.N * DI : 0; dw.in2 = a.z0_per_draw ? (size_t)a.N * a.K * DI : 0;
        dw.out = (size_t)a.N * a.T * DI; dw.out2 = (size_t)a.N * a.T * a.K * DI;
        dw.ts = a.ts_per_traj ? (size_t)a.T : 0; dw.sub = a.substeps;
        int grid, block;
        grid_for(a.N * a.K, grid, block);
        hipLaunchKernelGGL((rollout_jvp_kernel<typename TE::type, DI, DO, ORDER, METHOD>), dim3(grid, nd), block, 0, st, a.pack, a.M, a.S,
                           a.z0, a.v0, a.K, a.ts, a.N, a.T, a.zt, a.vt, dw);
        return check_launch(tags[KERNEL]);
      });
    });
  });
}

}  // namespace gp
