// gp_rollout.hpp -- what the persistent rollout kernels share: the wave-mapped evaluators (policy objects), the ODE right-hand side on
// the state, the state store, and the host-side launch policy (grid shapes, the team / wave threshold, the compiled widths).
// Used by gp_forward.hip (fixed-grid solvers), gp_adaptive.hip (Dormand-Prince), gp_backward.hip (reverse sweep) and gp_tangent.hip
// (forward mode: the jvp members of the streamed evaluators).
#pragma once
#include "gp_eval.hpp"
#include "gp_team.hpp"
#include "gp_launch.hpp"
#include <type_traits>

namespace gp {

// ----------------------------------------------------------------------------------------------
// evaluators (policy objects): operator()(x, f) leaves f(x) in every lane
// ----------------------------------------------------------------------------------------------
template <int DI, int DO, int SJ, int MJ> struct RbfRegEval {
  using L = RbfLayout<DI, DO>;
  float4 rff[SJ * DO][L::RQ];
  float4 ind[MJ][L::RQ2];
  const float* wl;
  __device__ __forceinline__ void init(const float* pack, int M, int S, int lane) {
    const float4* p4 = reinterpret_cast<const float4*>(pack);
#pragma unroll
    for (int r = 0; r < SJ * DO; ++r)
#pragma unroll
      for (int q = 0; q < L::RQ; ++q) rff[r][q] = p4[(r * L::RQ + q) * 64 + lane];
    const float4* i4 = p4 + L::rff_f4(S);
#pragma unroll
    for (int j = 0; j < MJ; ++j)
#pragma unroll
      for (int q = 0; q < L::RQ2; ++q) ind[j][q] = i4[(j * L::RQ2 + q) * 64 + lane];
    wl = pack + 4 * (L::rff_f4(S) + L::ind_f4(M));
  }
  template <int MODE> __device__ __forceinline__ void eval(const float (&x)[DI], float (&f)[DO]) const {
    float acc[DO];
#pragma unroll
    for (int d = 0; d < DO; ++d) acc[d] = 0.f;
    if (MODE != 2) {
#pragma unroll
      for (int j = 0; j < SJ; ++j)
#pragma unroll
        for (int d = 0; d < DO; ++d) rbf_rff_record<DI, DO>(rff[j * DO + d], x, acc[d]);
    }
    if (MODE != 1) {
#pragma unroll
      for (int j = 0; j < MJ; ++j) rbf_ind_record<DI, DO>(ind[j], x, wl, acc);
    }
    wave_sum_all<DO>(acc, f);
  }
};

template <int DI, int DO> struct RbfStreamEval {
  using L = RbfLayout<DI, DO>;
  const float4* rff4;
  const float4* ind4;
  const float* wl;
  int SJ, MJ, lane;
  __device__ __forceinline__ void init(const float* pack, int M, int S, int lane_) {
    rff4 = reinterpret_cast<const float4*>(pack);
    ind4 = rff4 + L::rff_f4(S);
    wl = pack + 4 * (L::rff_f4(S) + L::ind_f4(M));
    SJ = cdiv(S, 64); MJ = cdiv(M, 64); lane = lane_;
  }
  template <int MODE> __device__ __forceinline__ void eval(const float (&x)[DI], float (&f)[DO]) const {
    float acc[DO];
#pragma unroll
    for (int d = 0; d < DO; ++d) acc[d] = 0.f;
    if (MODE != 2) {
      for (int j = 0; j < SJ; ++j) {
#pragma unroll
        for (int d = 0; d < DO; ++d) {
          float4 r[L::RQ];
#pragma unroll
          for (int q = 0; q < L::RQ; ++q) r[q] = rff4[((j * DO + d) * L::RQ + q) * 64 + lane];
          rbf_rff_record<DI, DO>(r, x, acc[d]);
        }
      }
    }
    if (MODE != 1) {
      for (int j = 0; j < MJ; ++j) {
        float4 r[L::RQ2];
#pragma unroll
        for (int q = 0; q < L::RQ2; ++q) r[q] = ind4[(j * L::RQ2 + q) * 64 + lane];
        rbf_ind_record<DI, DO>(r, x, wl, acc);
      }
    }
    wave_sum_all<DO>(acc, f);
  }
  // f(x) and J_f(x) v in every lane: the records are read once for both, and one reduction carries the 2 DO partials (gp_tangent.hip)
  template <int MODE> __device__ __forceinline__ void jvp(const float (&x)[DI], const float (&v)[DI], float (&f)[DO], float (&jv)[DO]) const {
    float acc[DO], jacc[DO];
#pragma unroll
    for (int d = 0; d < DO; ++d) acc[d] = jacc[d] = 0.f;
    if (MODE != 2) {
      for (int j = 0; j < SJ; ++j) {
#pragma unroll
        for (int d = 0; d < DO; ++d) {
          float4 r[L::RQ];
#pragma unroll
          for (int q = 0; q < L::RQ; ++q) r[q] = rff4[((j * DO + d) * L::RQ + q) * 64 + lane];
          rbf_rff_jvp<DI, DO>(r, x, v, acc[d], jacc[d]);
        }
      }
    }
    if (MODE != 1) {
      for (int j = 0; j < MJ; ++j) {
        float4 r[L::RQ2];
#pragma unroll
        for (int q = 0; q < L::RQ2; ++q) r[q] = ind4[(j * L::RQ2 + q) * 64 + lane];
        rbf_ind_jvp<DI, DO>(r, x, v, wl, acc, jacc);
      }
    }
    wave_sum_pair<DO>(acc, jacc, f, jv);
  }
};

extern __shared__ __attribute__((aligned(16))) float4 gp_smem4[];

// DF: records from LDS (USE_LDS) or from global/L2.
template <int D, bool USE_LDS> struct DfEval {
  using L = DfLayout<D>;
  const float4* g4;  // global pack (records)
  const float* uni;  // uniform tail (global; scalar loads)
  int SJ, MJ, lane, ind_off;
  __device__ __forceinline__ void init(const float* pack, int M, int S, int lane_) {
    g4 = reinterpret_cast<const float4*>(pack);
    ind_off = (int)L::rff_f4(S);
    uni = pack + 4 * (L::rff_f4(S) + L::ind_f4(M));
    SJ = cdiv(S, 64); MJ = cdiv(M, 64); lane = lane_;
  }
  __device__ __forceinline__ float4 ld(int idx) const {
    if constexpr (USE_LDS) return gp_smem4[idx];
    else return g4[idx];
  }
  template <int MODE> __device__ __forceinline__ void eval(const float (&x)[D], float (&f)[D]) const {
    float acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.f;
    if (MODE != 2) {
      for (int j = 0; j < SJ; ++j) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
          float4 r[L::RQ];
#pragma unroll
          for (int q = 0; q < L::RQ; ++q) r[q] = ld(((j * D + i) * L::RQ + q) * 64 + lane);
          df_rff_record<D>(r, x, acc);
        }
      }
    }
    if (MODE != 1) {
      for (int j = 0; j < MJ; ++j) {
        float4 r[L::RQ2];
#pragma unroll
        for (int q = 0; q < L::RQ2; ++q) r[q] = ld(ind_off + (j * L::RQ2 + q) * 64 + lane);
        df_ind_record<D>(r, x, uni, acc);
      }
    }
    wave_sum_all<D>(acc, f);
  }
  // f(x) and J_f(x) v in every lane, as RbfStreamEval::jvp
  template <int MODE> __device__ __forceinline__ void jvp(const float (&x)[D], const float (&v)[D], float (&f)[D], float (&jv)[D]) const {
    float acc[D], jacc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = jacc[d] = 0.f;
    if (MODE != 2) {
      for (int j = 0; j < SJ; ++j) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
          float4 r[L::RQ];
#pragma unroll
          for (int q = 0; q < L::RQ; ++q) r[q] = ld(((j * D + i) * L::RQ + q) * 64 + lane);
          df_rff_jvp<D>(r, x, v, acc, jacc);
        }
      }
    }
    if (MODE != 1) {
      for (int j = 0; j < MJ; ++j) {
        float4 r[L::RQ2];
#pragma unroll
        for (int q = 0; q < L::RQ2; ++q) r[q] = ld(ind_off + (j * L::RQ2 + q) * 64 + lane);
        df_ind_jvp<D>(r, x, v, uni, acc, jacc);
      }
    }
    wave_sum_pair<D>(acc, jacc, f, jv);
  }
};

// cooperative copy of the record part of a pack into LDS (whole workgroup), then barrier
__device__ __forceinline__ void stage_pack_lds(const float* pack, size_t n_f4) {
  const float4* g4 = reinterpret_cast<const float4*>(pack);
  for (size_t i = threadIdx.x; i < n_f4; i += blockDim.x) gp_smem4[i] = g4[i];
  __syncthreads();
}

// The time grid of trajectory n: ts + n * stride (stride 0: the one grid every trajectory shares).  n is the same in every lane of a
// wavefront but lives in a vector register where it derives from threadIdx; read through the first lane it is a scalar, so the row
// pointer is one and the grid's entries stay scalar loads -- the step size multiplies the stage algebra as a scalar either way.
__device__ __forceinline__ const float* ts_row(const float* __restrict__ ts, int n, size_t stride) {
  return ts + (size_t)__builtin_amdgcn_readfirstlane(n) * stride;
}

// Sub-steps: two instantiations of each rollout kernel.  SUB = false is the kernel as it always was -- one step per output interval,
// the count a compile-time 1, so that the loop over the steps of an interval folds away and the launches with one step run the code
// they always ran; SUB = true reads the count from Draws::sub (measured: a run-time count in ONE instantiation cost every one-step
// launch 3 us at configs[0] and 6 us at configs[1]).  dispatch_substeps chooses on the host.
template <bool SUB> __device__ __forceinline__ int sub_count(int sub) { return SUB ? sub : 1; }
// The solver step inside the output interval [t0, t1] cut into `sub` equal steps: ONE fp32 division per interval, so that any sub gives
// the refined grid's own differences wherever those are exact in fp32 (a product with a rounded 1/sub would not).  Wave-uniform like
// its operands: read through the first lane the quotient stays a scalar.
template <bool SUB> __device__ __forceinline__ float sub_step(float t0, float t1, int sub) {
  if constexpr (!SUB) return t1 - t0;
  else return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((t1 - t0) / (float)sub)));
}

// Recorded stage inputs per step of a fixed-grid solver (0 euler, 1 rk4, 2 midpoint) -- the kernels' NS -- and the rows of a draw's
// record (N, T-1, sub, NS, .): the ONE place that spells the layout on the host.
constexpr int stages_of(int method) { return method == 0 ? 1 : (method == 1 ? 4 : 2); }
inline size_t record_rows(int N, int T, int sub, int method) { return (size_t)N * (T - 1) * sub * stages_of(method); }

template <int DI> __device__ __forceinline__ void store_state(float* __restrict__ dst, const float (&y)[DI], int lane) {
  if (lane < DI) {
    float v = y[0];
#pragma unroll
    for (int i = 1; i < DI; ++i) v = (lane == i) ? y[i] : v;
    dst[lane] = v;
  }
}

// ODE right-hand side on the state (flow.py:27-45): order 1: f(y); order 2: [v ; f(s,v)].
template <class EV, int DI, int DO, int ORDER>
__device__ __forceinline__ void ode_rhs(EV& ev, const float (&y)[DI], float (&dy)[DI]) {
  float fv[DO];
  ev.template eval<0>(y, fv);
  if (ORDER == 1) {
#pragma unroll
    for (int i = 0; i < DO; ++i) dy[i] = fv[i];
  } else {
#pragma unroll
    for (int i = 0; i < DO; ++i) { dy[i] = y[DO + i]; dy[DO + i] = fv[i]; }
  }
}

// ODE-level VJP (flow.py:27-45): order 1: dy = f(y); order 2: dy = [y[q:], f(y)].
// a (DI) = adjoint of dy  ->  gx (DI) = (d dy / d y)^T a ;  af (DO) = the part that multiplies J_f.
struct NoGrads {};
template <class EV, int DI, int DO, int ORDER, class GR = NoGrads>
__device__ __forceinline__ void ode_vjp(EV& ev, const float (&x)[DI], const float (&a)[DI], float (&gx)[DI], float (&af)[DO], GR* G = nullptr) {
#pragma unroll
  for (int i = 0; i < DO; ++i) af[i] = ORDER == 1 ? a[i] : a[DO + i];
  if constexpr (std::is_same<GR, NoGrads>::value) ev.vjp(x, af, gx);
  else ev.vjp_grad(x, af, gx, *G);                  // the row's parameter-gradient terms ride along (PGRAD form of the reverse sweep)
  if (ORDER != 1) {
#pragma unroll
    for (int i = 0; i < DO; ++i) gx[DO + i] += a[i];
  }
}

// ----------------------------------------------------------------------------------------------
// host-side launch policy: which evaluator a launch runs on, and its grid.  The ONE place that knows it -- rhs_fwd and rollout_fwd
// (gp_forward.hip), the landing and dense dopri5 (gp_adaptive.hip) and the reverse sweeps (gp_backward.hip, gp_adaptive.hip) hand
// forward_route / reverse_route a callable and supply only their kernel template, its arguments and their tags.
// ----------------------------------------------------------------------------------------------
static const size_t kLdsLimitBytes = 150 * 1024;  // 160 KiB per CU; leave headroom

template <int DI, int DO, int SJ, int MJ> constexpr bool rbf_reg_fits() {
  return 4 * (SJ * DO * RbfLayout<DI, DO>::RQ + MJ * RbfLayout<DI, DO>::RQ2) <= 260;
}

static inline void grid_for(int N, int& grid, int& block) {
  // one wave per row.  Few rows: 1 wave per workgroup so they spread over all 256 CUs;
  // many rows: 4 waves per workgroup, at most 2 workgroups per CU resident, grid-stride beyond.
  if (N <= 1024) { block = 64; grid = N; }
  else { block = 256; grid = (N + 3) / 4; if (grid > 2048) grid = 2048; }
  if (grid < 1) grid = 1;
}

static const int kTeamMaxRows = 2048;  // below this, 4 waves per trajectory beat 1 (all 1024 SIMDs busy sooner)
static inline int team_grid(int N) { return N < 2048 ? N : 2048; }

// register-resident team when the quarter pack fits (S <= 256, M <= 128, D <= 8), streamed team otherwise
template <int DI, int DO> static bool rbf_team_ok(int M, int S) {
  if constexpr (DO <= 8) return RbfTeamEval<DI, DO, 1>::fits(M, S);
  return false;
}
template <int D> static bool df_team_ok(int M, int S) {
  if constexpr (D <= 8) return DfTeamEval<D, 1>::fits(M, S);
  return false;
}

template <int V> using int_c = std::integral_constant<int, V>;
template <class T> struct type_c { using type = T; };

// A route: the evaluator (a type), the mapping (a type) and this.  `route` numbers the family's routes in the order of the ladder
// below -- the index into a consumer's table of tags.  lds_f4: float4 of pack a wave kernel stages in LDS, 0 on every other route.
enum Mapping { kTeam, kWave, kWaveLds };             // one workgroup of four wavefronts per row / one wavefront per row (pack in LDS)
using team_c = int_c<kTeam>;
using wave_c = int_c<kWave>;
using wave_lds_c = int_c<kWaveLds>;
struct LaunchGeom { int route, grid, block; size_t lds_f4; };
enum { kRouteTeam, kRouteTeamStream, kRouteRbfReg42, kRouteRbfReg11, kRouteRbfStream, kRouteDfLds = 2, kRouteDfStream, kRoutes = 5 };

// The forward ladder of a kernel family (KERNEL 0: RBF, 1: divergence-free, DI = DO) at N rows: f(type_c<EV>, mapping, geometry).
template <int KERNEL, int DI, int DO, class F> static int forward_route(int N, int M, int S, F&& f) {
  int grid, block;
  grid_for(N, grid, block);
  if constexpr (KERNEL == 0) {
    if (N <= kTeamMaxRows && DO <= 16) {
      if (RbfTeamEval<DI, DO, 1>::fits(M, S)) return f(type_c<RbfTeamEval<DI, DO, 1>>{}, team_c{}, LaunchGeom{kRouteTeam, team_grid(N), 256, 0});
    }
    if (N <= kTeamMaxRows)       // past the register-resident quarter pack: the same team, records streamed from L2
      return f(type_c<RbfStreamTeam<DI, DO>>{}, team_c{}, LaunchGeom{kRouteTeamStream, team_grid(N), 256, 0});
    const int SJ = cdiv(S, 64), MJ = cdiv(M, 64);
    if constexpr (rbf_reg_fits<DI, DO, 4, 2>()) {
      if (SJ == 4 && MJ == 2) return f(type_c<RbfRegEval<DI, DO, 4, 2>>{}, wave_c{}, LaunchGeom{kRouteRbfReg42, grid, block, 0});
    }
    if constexpr (rbf_reg_fits<DI, DO, 1, 1>()) {
      if (SJ == 1 && MJ == 1) return f(type_c<RbfRegEval<DI, DO, 1, 1>>{}, wave_c{}, LaunchGeom{kRouteRbfReg11, grid, block, 0});
    }
    return f(type_c<RbfStreamEval<DI, DO>>{}, wave_c{}, LaunchGeom{kRouteRbfStream, grid, block, 0});
  } else {
    static_assert(DI == DO, "the divergence-free kernel maps R^D to R^D");
    using L = DfLayout<DO>;
    const size_t f4 = L::rff_f4(S) + L::ind_f4(M);
    if constexpr (DO <= 8) {
      if (N <= kTeamMaxRows && DfTeamEval<DO, 1>::fits(M, S)) return f(type_c<DfTeamEval<DO, 1>>{}, team_c{}, LaunchGeom{kRouteTeam, team_grid(N), 256, 0});
    }
    if (N <= kTeamMaxRows)       // e.g. BASELINE configs[4] (D = 16, M = 512): 4 wavefronts per trajectory, records streamed from L2
      return f(type_c<DfStreamTeam<DO>>{}, team_c{}, LaunchGeom{kRouteTeamStream, team_grid(N), 256, 0});
    // N > kTeamMaxRows from here on: a workgroup evaluates many rows, so staging the pack in LDS pays whenever it fits
    if (f4 * 16 <= kLdsLimitBytes) return f(type_c<DfEval<DO, true>>{}, wave_lds_c{}, LaunchGeom{kRouteDfLds, 256, 256, f4});
    return f(type_c<DfEval<DO, false>>{}, wave_c{}, LaunchGeom{kRouteDfStream, grid, block, 0});
  }
}

// The reverse side (rollout_bwd, rhs_vjp, the dopri5 sweeps) runs on a team at any number of rows: register-resident (route 0) when
// the quarter pack fits and D <= 8 -- a narrower limit than the forward team's, the sweep holds the adjoints as well -- streamed
// (route 1) otherwise: f(type_c<EV>, geometry).
template <int KERNEL, int DI, int DO, class F> static int reverse_route(int rows, int M, int S, F&& f) {
  if constexpr (DO <= 8) {
    if constexpr (KERNEL == 0) {
      if (rbf_team_ok<DI, DO>(M, S)) return f(type_c<RbfTeamEval<DI, DO, 1>>{}, LaunchGeom{kRouteTeam, team_grid(rows), 256, 0});
    } else {
      if (df_team_ok<DO>(M, S)) return f(type_c<DfTeamEval<DO, 1>>{}, LaunchGeom{kRouteTeam, team_grid(rows), 256, 0});
    }
  }
  using Stream = std::conditional_t<KERNEL == 0, RbfStreamTeam<DI, DO>, DfStreamTeam<DO>>;
  return f(type_c<Stream>{}, LaunchGeom{kRouteTeamStream, team_grid(rows), 256, 0});
}

// The launch of a route, draws on gridDim.y.  A pack staged in LDS may pass the 64 KB a kernel gets by default: set_max_lds.
template <class... P, class... A> static int launch_route(void (*kern)(P...), const LaunchGeom& g, int nd, hipStream_t st, A... args) {
  if (set_max_lds((const void*)kern, g.lds_f4 * 16)) return 1;
  hipLaunchKernelGGL(kern, dim3(g.grid, nd), g.block, g.lds_f4 * 16, st, args...);
  return 0;
}

// dispatch tables -----------------------------------------------------------------------------
#define GP_RBF_DIMS(X) X(6, 6) X(6, 3) X(4, 4) X(4, 2) X(2, 2) X(2, 1) X(8, 8) X(8, 4) X(16, 16) X(16, 8) X(3, 3) X(12, 6)
#define GP_DF_DIMS(X) X(6) X(4) X(2) X(3) X(8) X(16) X(5) X(7) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

// The compiled widths of a kernel family (0: RBF, anything else: divergence-free): f(int_c<KERNEL>, int_c<DI>, int_c<DO>), which
// returns 0 or 1; -1 for a width that is not compiled.
template <class F> static int for_dims(int kernel, int Di, int Do, F&& f) {
  if (kernel == 0) {
#define X(a, b) if (Di == a && Do == b) return f(int_c<0>{}, int_c<a>{}, int_c<b>{});
    GP_RBF_DIMS(X)
#undef X
  } else {
#define X(a) if (Di == a && Do == a) return f(int_c<1>{}, int_c<a>{}, int_c<a>{});
    GP_DF_DIMS(X)
#undef X
  }
  return -1;
}
// the same for an entry point: who names it in the error text
template <class F> static int dispatch_dims(const char* who, int kernel, int Di, int Do, F&& f) {
  const int rc = for_dims(kernel, Di, Do, f);
  return rc < 0 ? set_error("%s: no specialisation for kernel=%d Di=%d Do=%d", who, kernel, Di, Do) : rc;
}

// Order 1 or 2 of a compiled width, whichever DI == ORDER * DO allows: f(int_c<ORDER>).
template <int DI, int DO, class F> static int dispatch_order(const char* who, int order, F&& f) {
  if constexpr (DI == DO) { if (order == 1) return f(int_c<1>{}); }
  if constexpr (DI == 2 * DO) { if (order == 2) return f(int_c<2>{}); }
  return set_error("%s: order=%d needs Di == order*Do (Di=%d Do=%d)", who, order, DI, DO);
}

// One step per output interval (the kernels as they always were) or Draws::sub of them: f(std::bool_constant<SUB>).
// force_substep_kernels (capi.hip, gpode_test_substep_kernels): a door for tests, shut unless a test opens it, that sends a count of 1
// through the SUB = true instantiation as well -- the way to hold that instantiation to itself on a refined grid.
bool* force_substep_kernels();
template <class F> static int dispatch_substeps(int sub, F&& f) {
  return sub == 1 && !*force_substep_kernels() ? f(std::false_type{}) : f(std::true_type{});
}

// The fixed-grid solver, 0 euler, 1 rk4, 2 midpoint (the caller has refused every other value): f(int_c<METHOD>).
template <class F> static int dispatch_method(int method, F&& f) {
  return method == 0 ? f(int_c<0>{}) : method == 1 ? f(int_c<1>{}) : f(int_c<2>{});
}

}  // namespace gp
