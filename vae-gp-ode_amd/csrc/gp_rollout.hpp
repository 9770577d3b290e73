// gp_rollout.hpp -- what the persistent rollout kernels share: the wave-mapped evaluators (policy objects), the ODE right-hand side on
// the state, the state store, and the host-side launch policy (grid shapes, the team / wave threshold, the compiled widths).
// Used by gp_forward.hip (fixed-grid solvers) and gp_adaptive.hip (Dormand-Prince).
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
};

// cooperative copy of the record part of a pack into LDS (whole workgroup), then barrier
__device__ __forceinline__ void stage_pack_lds(const float* pack, size_t n_f4) {
  const float4* g4 = reinterpret_cast<const float4*>(pack);
  for (size_t i = threadIdx.x; i < n_f4; i += blockDim.x) gp_smem4[i] = g4[i];
  __syncthreads();
}

// ODE right-hand side on the state (flow.py:27-45): order 1: f(y); order 2: [v ; f(s,v)].
template <class EV, int DI, int DO, int ORDER>
__device__ __forceinline__ void ode_rhs(const EV& ev, const float (&y)[DI], float (&dy)[DI]) {
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

template <int DI> __device__ __forceinline__ void store_state(float* __restrict__ dst, const float (&y)[DI], int lane) {
  if (lane < DI) {
    float v = y[0];
#pragma unroll
    for (int i = 1; i < DI; ++i) v = (lane == i) ? y[i] : v;
    dst[lane] = v;
  }
}

template <class EV, int DI, int DO, int ORDER>
__device__ __forceinline__ void ode_rhs_mut(EV& ev, const float (&y)[DI], float (&dy)[DI]) {
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
// host-side launch policy
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

// dispatch tables -----------------------------------------------------------------------------
#define GP_RBF_DIMS(X) X(6, 6) X(6, 3) X(4, 4) X(4, 2) X(2, 2) X(2, 1) X(8, 8) X(8, 4) X(16, 16) X(16, 8) X(3, 3) X(12, 6)
#define GP_DF_DIMS(X) X(6) X(4) X(2) X(3) X(8) X(16) X(5) X(7) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

}  // namespace gp
