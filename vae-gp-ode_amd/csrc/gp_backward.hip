// gp_backward.hip -- reverse sweep of the fixed-grid rollout and parameter gradients of f.
//
// The reference back-propagates through the unrolled solver with autograd (use_adjoint=False,
// main.py:85,209-210): 4(T-1) RHS graphs per draw.  Here the same discretise-then-optimise gradient is
// computed by two kernels per draw:
//
//  A  rollout_bwd_team_kernel  one workgroup (4 waves) per trajectory walks the steps backwards over the
//     stage inputs the forward stored (xstage), applying the adjoint of the 3/8-rule (or Euler) stage
//     algebra; each stage costs one vector-Jacobian product J_f(x)^T a.  Outputs dL/dz0 and the stage
//     adjoints a (astage).  Sequential in t, parallel over trajectories.
//  B  param_grad_team_kernel   with (x, a) known for every (trajectory, step, stage) row, the parameter
//     gradient is a plain sum over rows -- no sequential dependence left.  Each wave keeps its quarter of
//     the pack AND the matching gradient accumulators in registers and streams a chunk of rows; chunk
//     results go to a slab that a second kernel sums in fixed order (deterministic, no float atomics).
//     Gradients come out in PACK LAYOUT (d/d om, d/d aw, d/d z, d/d cc ... + the uniform tail), which
//     gp_cache_bwd.hip chains back to the raw parameters.
#include "gp_rollout.hpp"

namespace gp {

template <int DI, int DO, int NJ>
__device__ __forceinline__ void store_grads_rbf(const typename RbfTeamEval<DI, DO, NJ>::Grads& G, float* __restrict__ out, int M, int S,
                                                int wave, int lane, float (*sInd)[64][4 * RbfLayout<DI, DO>::RQ2],
                                                float (*sUni)[((DO + 1) / 2) * DI]);
template <int D, int NJ, int PART = 0>
__device__ __forceinline__ void store_grads_df(const typename DfTeamEval<D, NJ>::Grads& G, float* __restrict__ out, int M, int S, int wave,
                                               int lane, float (*sInd)[64][4 * DfLayout<D>::RQ2],
                                               float (*sUni)[2 * D * ((D + 1) / 2) + (D + 1) / 2]);

template <class EV, bool PG> struct GradsOf { using type = NoGrads; };
template <class EV> struct GradsOf<EV, true> { using type = typename EV::Grads; };

// PG (register-resident team evaluators only): the parameter-gradient sums of the rows this workgroup walks are accumulated in
// the same pass (EV::vjp_grad) and written to slab[blockIdx.x] in pack layout -- what param_grad_{rbf,df}_kernel computes from the
// stored (x, a) rows in a launch of its own, the first node of the backward pass's side branch.
// SUB (gp_rollout.hpp): false = one step per output interval, the kernel as it always was; true = dw.sub steps per interval, walked
// last first; the record is (N, T-1, sub, NS, .) and gzt[t] enters when the walk reaches the start of interval t either way.
template <class EV, int DI, int DO, int ORDER, int METHOD, bool PG = false, bool SUB = false>
__global__ __launch_bounds__(64 * EV::kTeam) void rollout_bwd_team_kernel(const float* __restrict__ pack, int M, int S,
                                                                const float* __restrict__ xstage, const float* __restrict__ gzt,
                                                                const float* __restrict__ ts, int N, int T,
                                                                float* __restrict__ gz0, float* __restrict__ astage, Draws dw,
                                                                float* __restrict__ slab = nullptr, size_t pack_floats = 0) {
  constexpr int NS = stages_of(METHOD);
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  // blockIdx.y = Monte-Carlo draw
  pack += blockIdx.y * dw.pack; xstage += blockIdx.y * dw.in; gzt += blockIdx.y * dw.in2; gz0 += blockIdx.y * dw.out; astage += blockIdx.y * dw.out2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  using GR = typename GradsOf<EV, PG>::type;
  GR G;
  if constexpr (PG) G.zero();
  const float third = (float)(1.0 / 3.0);
  const int sub = sub_count<SUB>(dw.sub);
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const float* gz = gzt + (size_t)n * T * DI;
    const float* xs = xstage + (size_t)n * (T - 1) * sub * NS * DI;
    float* as = astage + (size_t)n * (T - 1) * sub * NS * DO;
    float lam[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) lam[i] = gz[(size_t)(T - 1) * DI + i];
    const float* tn = ts_row(ts, n, dw.ts);          // this trajectory's grid (dw.ts = 0: the shared one)
    for (int t = T - 2; t >= 0; --t) {
      const float dt = sub_step<SUB>(tn[t], tn[t + 1], sub);
      for (int r = (t + 1) * sub - 1; r >= t * sub; --r) {   // the interval's steps, last first: row block r of the record
        const float* xt = xs + (size_t)r * NS * DI;
        float* at = as + (size_t)r * NS * DO;
        float x[DI], g[DI], af[DO];
        if (METHOD == 0) {
          float a1[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) { a1[i] = dt * lam[i]; x[i] = xt[i]; }
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a1, g, af, &G);
          if (wave == 0) store_state<DO>(at, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) lam[i] += g[i];
        } else if (METHOD == 2) {
          // midpoint: y1 = y + dt k2, k2 = f(x2), x2 = y + dt/2 k1, k1 = f(y)
          float a1[DI], a2[DI], ay[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) { a2[i] = dt * lam[i]; x[i] = xt[DI + i]; }
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a2, g, af, &G);
          if (wave == 0) store_state<DO>(at + DO, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) { ay[i] = lam[i] + g[i]; a1[i] = 0.5f * dt * g[i]; x[i] = xt[i]; }
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a1, g, af, &G);
          if (wave == 0) store_state<DO>(at, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) lam[i] = ay[i] + g[i];
        } else {
          // y1 = y + (k1 + 3(k2+k3) + k4) dt/8 ;  x2 = y + dt k1/3 ; x3 = y + dt(k2 - k1/3) ; x4 = y + dt(k1 - k2 + k3)
          float a1[DI], a2[DI], a3[DI], a4[DI], ay[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) {
            const float l8 = lam[i] * dt * 0.125f;
            a1[i] = l8; a4[i] = l8; a2[i] = 3.f * l8; a3[i] = 3.f * l8; ay[i] = lam[i];
          }
#pragma unroll
          for (int i = 0; i < DI; ++i) x[i] = xt[3 * DI + i];
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a4, g, af, &G);
          if (wave == 0) store_state<DO>(at + 3 * DO, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) { ay[i] += g[i]; a1[i] += dt * g[i]; a2[i] -= dt * g[i]; a3[i] += dt * g[i]; }
#pragma unroll
          for (int i = 0; i < DI; ++i) x[i] = xt[2 * DI + i];
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a3, g, af, &G);
          if (wave == 0) store_state<DO>(at + 2 * DO, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) { ay[i] += g[i]; a2[i] += dt * g[i]; a1[i] -= dt * third * g[i]; }
#pragma unroll
          for (int i = 0; i < DI; ++i) x[i] = xt[1 * DI + i];
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a2, g, af, &G);
          if (wave == 0) store_state<DO>(at + 1 * DO, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) { ay[i] += g[i]; a1[i] += dt * third * g[i]; }
#pragma unroll
          for (int i = 0; i < DI; ++i) x[i] = xt[i];
          ode_vjp<EV, DI, DO, ORDER, GR>(ev, x, a1, g, af, &G);
          if (wave == 0) store_state<DO>(at, af, lane);
#pragma unroll
          for (int i = 0; i < DI; ++i) lam[i] = ay[i] + g[i];
        }
      }
#pragma unroll
      for (int i = 0; i < DI; ++i) lam[i] += gz[(size_t)t * DI + i];
    }
    if (wave == 0) store_state<DI>(gz0 + (size_t)n * DI, lam, lane);
  }
  if constexpr (PG) {
    float* out = slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * pack_floats;
    if constexpr (std::is_same<EV, RbfTeamEval<DI, DO, 1>>::value) {
      using L = RbfLayout<DI, DO>;
      __shared__ __attribute__((aligned(16))) float sInd[2][64][4 * L::RQ2];
      __shared__ float sUni[TEAM][((DO + 1) / 2) * DI];
      store_grads_rbf<DI, DO, 1>(G, out, M, S, wave, lane, sInd, sUni);
    } else {
      using L = DfLayout<DO>;
      constexpr int DH = (DO + 1) / 2;
      __shared__ __attribute__((aligned(16))) float sInd[2][64][4 * L::RQ2];
      __shared__ float sUni[TEAM][2 * DO * DH + DH];
      store_grads_df<DO, 1>(G, out, M, S, wave, lane, sInd, sUni);
    }
  }
}

// rows (R,DI), adjoints (R,DO) -> gx (R,DI) = J_f(x)^T a   (used for the f_prior(Z) path of the cache backward)
template <class EV, int DI, int DO>
__global__ __launch_bounds__(64 * EV::kTeam) void rhs_vjp_team_kernel(const float* __restrict__ pack, int M, int S,
                                                            const float* __restrict__ x, const float* __restrict__ a, int R,
                                                            float* __restrict__ gx, int prior_only, Draws dw) {
  __shared__ float slots[2 * EV::kTeam * TeamCombine::DP];
  pack += blockIdx.y * dw.pack; x += blockIdx.y * dw.in; a += blockIdx.y * dw.in2; gx += blockIdx.y * dw.out;   // blockIdx.y = Monte-Carlo draw
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  for (int n = blockIdx.x; n < R; n += gridDim.x) {
    float xv[DI], av[DO], g[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) xv[i] = x[(size_t)n * DI + i];
#pragma unroll
    for (int i = 0; i < DO; ++i) av[i] = a[(size_t)n * DO + i];
    ev.vjp(xv, av, g, prior_only != 0);
    if (wave == 0) store_state<DI>(gx + (size_t)n * DI, g, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// B: parameter gradients in pack layout
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void st4(float* __restrict__ base, size_t f4_index, const float* v) {
  reinterpret_cast<float4*>(base)[f4_index] = make_float4(v[0], v[1], v[2], v[3]);
}

// this workgroup's gradient sums -> its slab (pack layout); shared by the parameter-sum kernel and the PGRAD reverse sweep
template <int DI, int DO, int NJ>
__device__ __forceinline__ void store_grads_rbf(const typename RbfTeamEval<DI, DO, NJ>::Grads& G, float* __restrict__ out, int M, int S,
                                                int wave, int lane, float (*sInd)[64][4 * RbfLayout<DI, DO>::RQ2],
                                                float (*sUni)[((DO + 1) / 2) * DI]) {
  using L = RbfLayout<DI, DO>;
  constexpr int DH = (DO + 1) / 2;
  const int SJ = cdiv(S, 64), MJ = cdiv(M, 64);
#pragma unroll
  for (int jn = 0; jn < NJ; ++jn) {
    const int j = wave + TEAM * jn;
    if (j < SJ) {
#pragma unroll
      for (int d = 0; d < DO; ++d)
#pragma unroll
        for (int q = 0; q < L::RQ; ++q) st4(out, (size_t)((j * DO + d) * L::RQ + q) * 64 + lane, &G.rff[jn * DO + d][4 * q]);
    }
  }
  // inducing record j = wave>>1: the two halves share the z fields -> add through LDS, lower half stores
  const int j = wave >> 1, half = wave & 1;
  if (half == 1) {
#pragma unroll
    for (int q = 0; q < 4 * L::RQ2; ++q) sInd[j][lane][q] = G.ind[q];
  }
  // uniform tail: lane-reduce this wave's partial of d/d wl[half*DH+dd][i]
  {
    float flat[DH * DI], red[DH * DI];
#pragma unroll
    for (int e = 0; e < DH * DI; ++e) flat[e] = G.gwl[e / DI][e % DI];
    wave_sum_all<DH * DI>(flat, red);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < DH * DI; ++e) sUni[wave][e] = red[e];
    }
  }
  __syncthreads();
  if (half == 0 && j < MJ) {
    float* ind_out = out + 4 * L::rff_f4(S);
    float v[4 * L::RQ2];
#pragma unroll
    for (int q = 0; q < 4 * L::RQ2; ++q) v[q] = G.ind[q] + sInd[j][lane][q];
#pragma unroll
    for (int q = 0; q < L::RQ2; ++q) st4(ind_out, (size_t)(j * L::RQ2 + q) * 64 + lane, &v[4 * q]);
  }
  if (threadIdx.x < DO * DI) {
    const int d = threadIdx.x / DI, i = threadIdx.x % DI;
    const int h = d / DH, dd = d % DH;
    float* uni_out = out + 4 * (L::rff_f4(S) + L::ind_f4(M));
    uni_out[d * DI + i] = sUni[h][dd * DI + i] + sUni[h + 2][dd * DI + i];
  }
}

// The rows [r0, r1) of a chunk for the register-resident DF parameter-sum kernels, one row ahead: the (wave-uniform, scalar) loads of
// row r + 1 are issued before the arithmetic of row r, so their latency hides behind a row's worth of work instead of standing at
// the top of every row.  The index is clamped, not branched around: the last row asks for itself again and the copy is dropped, so
// nothing past r1 - 1 is read and no row of the next chunk can reach these sums.
template <int DI, int DO, class ROW>
__device__ __forceinline__ void chunk_rows_ahead(const float* __restrict__ xr, const float* __restrict__ ar, int r0, int r1, ROW&& row) {
  if (r0 >= r1) return;
  // The first row goes through readfirstlane (it is uniform already): were it a plain load, the compiler would merge it with the
  // load at the bottom of the loop into ONE load of a loop-carried address at the top of every row -- the loop this replaces.
  float xn[DI], an[DO];
#pragma unroll
  for (int i = 0; i < DI; ++i) xn[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xr[(size_t)r0 * DI + i])));
#pragma unroll
  for (int i = 0; i < DO; ++i) an[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ar[(size_t)r0 * DO + i])));
  // Every load issued so far (the pack's records, the uniform tail) lands here: a scalar load still pending at the loop's entry makes
  // its first use inside the loop a wait for ALL scalar loads -- they return out of order -- in every row, the row just requested
  // included.
  __builtin_amdgcn_s_waitcnt(0x0070);                // vmcnt(0) lgkmcnt(0)
  for (int r = r0; r < r1; ++r) {
    float x[DI], a[DO];
#pragma unroll
    for (int i = 0; i < DI; ++i) x[i] = xn[i];
#pragma unroll
    for (int i = 0; i < DO; ++i) a[i] = an[i];
    const int rn = min(r + 1, r1 - 1);
#pragma unroll
    for (int i = 0; i < DI; ++i) xn[i] = xr[(size_t)rn * DI + i];
#pragma unroll
    for (int i = 0; i < DO; ++i) an[i] = ar[(size_t)rn * DO + i];
    __builtin_amdgcn_sched_barrier(0);               // nothing in the block uses them: left alone, the scheduler puts them last
    row(x, a);
  }
}
// ... with the loop unswitched on prior_only by hand (row(x, a, std::bool_constant)): a row has to stay ONE basic block -- with the
// branch inside the loop the compiler sinks the next row's loads past it, to the end of the iteration, and they wait as before.
template <int DI, int DO, class ROW>
__device__ __forceinline__ void chunk_rows_ahead(const float* __restrict__ xr, const float* __restrict__ ar, int r0, int r1, int prior_only,
                                                 ROW&& row) {
  if (prior_only) chunk_rows_ahead<DI, DO>(xr, ar, r0, r1, [&](const float (&x)[DI], const float (&a)[DO]) { row(x, a, std::true_type()); });
  else chunk_rows_ahead<DI, DO>(xr, ar, r0, r1, [&](const float (&x)[DI], const float (&a)[DO]) { row(x, a, std::false_type()); });
}

template <int DI, int DO, int NJ>
__global__ __launch_bounds__(256) void param_grad_rbf_kernel(const float* __restrict__ pack, int M, int S,
                                                              const float* __restrict__ xr, const float* __restrict__ ar,
                                                              int R, int rows_per_chunk, float* __restrict__ slab,
                                                              size_t pack_floats, int prior_only, Draws dw, int slab_chunks) {
  // blockIdx.y = Monte-Carlo draw: its pack, its rows, its chunk slabs
  pack += blockIdx.y * dw.pack; xr += blockIdx.y * dw.in; ar += blockIdx.y * dw.in2; slab += (size_t)blockIdx.y * slab_chunks * pack_floats;
  using EV = RbfTeamEval<DI, DO, NJ>;
  using L = RbfLayout<DI, DO>;
  constexpr int DH = (DO + 1) / 2;
  __shared__ float slots[2 * TEAM * TeamCombine::DP];
  __shared__ __attribute__((aligned(16))) float sInd[2][64][4 * L::RQ2];
  __shared__ float sUni[TEAM][DH * DI];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  typename EV::Grads G;
  G.zero();
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  for (int r = r0; r < r1; ++r) {
    float x[DI], a[DO];
#pragma unroll
    for (int i = 0; i < DI; ++i) x[i] = xr[(size_t)r * DI + i];
#pragma unroll
    for (int i = 0; i < DO; ++i) a[i] = ar[(size_t)r * DO + i];
    ev.grad_row(x, a, G, prior_only != 0);
  }
  store_grads_rbf<DI, DO, NJ>(G, slab + (size_t)blockIdx.x * pack_floats, M, S, wave, lane, sInd, sUni);
}

template <int D, int NJ, int PART>
__device__ __forceinline__ void store_grads_df(const typename DfTeamEval<D, NJ>::Grads& G, float* __restrict__ out, int M, int S, int wave,
                                               int lane, float (*sInd)[64][4 * DfLayout<D>::RQ2],
                                               float (*sUni)[2 * D * ((D + 1) / 2) + (D + 1) / 2]) {
  using L = DfLayout<D>;
  constexpr int DH = (D + 1) / 2;
  constexpr int NU = 2 * D * DH + DH;
  const int SJ = cdiv(S, 64), MJ = cdiv(M, 64);
  if constexpr (PART != 2) {
#pragma unroll
    for (int jn = 0; jn < NJ; ++jn) {
      const int j = wave + TEAM * jn;
      if (j < SJ) {
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
          for (int q = 0; q < L::RQ; ++q) st4(out, (size_t)((j * D + i) * L::RQ + q) * 64 + lane, &G.rff[jn * D + i][4 * q]);
      }
    }
  }
  if constexpr (PART == 1) return;                   // the inducing records and the uniform tail are another workgroup's
  const int j = wave >> 1, half = wave & 1;
  if (half == 1) {
#pragma unroll
    for (int q = 0; q < 4 * L::RQ2; ++q) sInd[j][lane][q] = G.ind[q];
  }
  {
    // lane-reduce the uniform partials in chunks of <= 8
    float flat[NU];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < DH; ++b) { flat[a * DH + b] = G.gwab[a][b]; flat[D * DH + a * DH + b] = G.gil2[a][b]; }
#pragma unroll
    for (int b = 0; b < DH; ++b) flat[2 * D * DH + b] = G.gvar[b];
    float red[NU];
    wave_sum_all<NU>(flat, red);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < NU; ++e) sUni[wave][e] = red[e];
    }
  }
  __syncthreads();
  if (half == 0 && j < MJ) {
    float* ind_out = out + 4 * L::rff_f4(S);
    float v[4 * L::RQ2];
#pragma unroll
    for (int q = 0; q < 4 * L::RQ2; ++q) v[q] = G.ind[q] + sInd[j][lane][q];
#pragma unroll
    for (int q = 0; q < L::RQ2; ++q) st4(ind_out, (size_t)(j * L::RQ2 + q) * 64 + lane, &v[4 * q]);
  }
  {
    float* uni_out = out + 4 * (L::rff_f4(S) + L::ind_f4(M));
    const int t = threadIdx.x;
    if (t < D * D) {  // wab and il2: entry (a,b)
      const int a = t / D, b = t % D, h = b / DH, bb = b % DH;
      uni_out[a * D + b] = sUni[h][a * DH + bb] + sUni[h + 2][a * DH + bb];
      uni_out[D * D + a * D + b] = sUni[h][D * DH + a * DH + bb] + sUni[h + 2][D * DH + a * DH + bb];
    }
    if (t < D) {
      const int h = t / DH, bb = t % DH;
      uni_out[2 * D * D + t] = sUni[h][2 * D * DH + bb] + sUni[h + 2][2 * D * DH + bb];
    }
  }
}

template <int D, int NJ>
__global__ __launch_bounds__(256) void param_grad_df_kernel(const float* __restrict__ pack, int M, int S,
                                                             const float* __restrict__ xr, const float* __restrict__ ar,
                                                             int R, int rows_per_chunk, float* __restrict__ slab,
                                                             size_t pack_floats, int prior_only, Draws dw, int slab_chunks) {
  // blockIdx.y = Monte-Carlo draw: its pack, its rows, its chunk slabs
  pack += blockIdx.y * dw.pack; xr += blockIdx.y * dw.in; ar += blockIdx.y * dw.in2; slab += (size_t)blockIdx.y * slab_chunks * pack_floats;
  using EV = DfTeamEval<D, NJ>;
  using L = DfLayout<D>;
  constexpr int DH = (D + 1) / 2;
  constexpr int NU = 2 * D * DH + DH;  // gwab, gil2, gvar partials of one wave
  __shared__ float slots[2 * TEAM * TeamCombine::DP];
  __shared__ __attribute__((aligned(16))) float sInd[2][64][4 * L::RQ2];
  __shared__ float sUni[TEAM][NU];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  typename EV::Tail tail;
  ev.load_tail(tail, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1);
  typename EV::Grads G;
  G.zero();
  const int r0 = blockIdx.x * rows_per_chunk;
  const int r1 = min(R, r0 + rows_per_chunk);
  chunk_rows_ahead<D, D>(xr, ar, r0, r1, prior_only,
                         [&](const float (&x)[D], const float (&a)[D], auto po) { ev.grad_row(x, a, G, decltype(po)::value, tail); });
  store_grads_df<D, NJ>(G, slab + (size_t)blockIdx.x * pack_floats, M, S, wave, lane, sInd, sUni);
}

// The same sums with the PACK split over two workgroups per chunk of rows (blockIdx.z: 0 = the Fourier-feature records, 1 = the
// inducing records and the uniform tail): either half keeps under 256 registers, so the two share a CU -- the unsplit kernel's 432
// registers allow one wavefront per SIMD, whose every dependent instruction waits out its full latency (168 us at configs[1], the
// first and longest node of the backward pass's side branch).
template <int D, int PART>
__device__ __forceinline__ void pgrad_df_part(const float* __restrict__ pack, int M, int S, const float* __restrict__ xr,
                                              const float* __restrict__ ar, int r0, int r1, float* __restrict__ out, int prior_only) {
  using EV = DfTeamEval<D, 1>;
  using L = DfLayout<D>;
  constexpr int DH = (D + 1) / 2;
  constexpr int NU = 2 * D * DH + DH;
  __shared__ float slots[2 * TEAM * TeamCombine::DP];
  __shared__ __attribute__((aligned(16))) float sInd[2][64][4 * L::RQ2];
  __shared__ float sUni[TEAM][NU];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EV ev;
  ev.init(pack, M, S, slots, wave, lane);
  typename EV::Tail tail;
  if constexpr (PART != 1) ev.load_tail(tail, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1);
  typename EV::Grads G;
  G.zero();
  if constexpr (PART == 1)                           // the Fourier-feature records do not look at prior_only
    chunk_rows_ahead<D, D>(xr, ar, r0, r1, [&](const float (&x)[D], const float (&a)[D]) { ev.template grad_row_part<1>(x, a, G, false, tail); });
  else
    chunk_rows_ahead<D, D>(xr, ar, r0, r1, prior_only, [&](const float (&x)[D], const float (&a)[D], auto po) {
      ev.template grad_row_part<PART>(x, a, G, decltype(po)::value, tail);
    });
  store_grads_df<D, 1, PART>(G, out, M, S, wave, lane, sInd, sUni);
}
template <int D>
__global__ __launch_bounds__(256, 2) void param_grad_df_split_kernel(const float* __restrict__ pack, int M, int S,
                                                                      const float* __restrict__ xr, const float* __restrict__ ar,
                                                                      int R, int rows_per_chunk, float* __restrict__ slab,
                                                                      size_t pack_floats, int prior_only, Draws dw, int slab_chunks) {
  pack += blockIdx.y * dw.pack; xr += blockIdx.y * dw.in; ar += blockIdx.y * dw.in2; slab += (size_t)blockIdx.y * slab_chunks * pack_floats;
  const int r0 = blockIdx.x * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
  float* out = slab + (size_t)blockIdx.x * pack_floats;
  if (blockIdx.z == 0) pgrad_df_part<D, 1>(pack, M, S, xr, ar, r0, r1, out, prior_only);
  else pgrad_df_part<D, 2>(pack, M, S, xr, ar, r0, r1, out, prior_only);
}

// ---------------------------------------------------------------------------------------------
// B (streamed): the same sums for shapes past the register-resident team (S > 256, M > 128, DF D = 16).
// A workgroup still owns a chunk of rows, but walks the records one batch of four wavefronts at a time: a
// wavefront holds ONE record and that record's gradient in registers, streams the chunk's rows past it (x, a are
// wave-uniform loads from L2) and writes the finished record gradient to the slab; the uniform-tail partials stay
// in registers across the inducing batches.
// ---------------------------------------------------------------------------------------------
template <int DI, int DO>
__global__ __launch_bounds__(256) void param_grad_rbf_stream_kernel(const float* __restrict__ pack, int M, int S,
                                                                     const float* __restrict__ xr, const float* __restrict__ ar,
                                                                     int R, int rows_per_chunk, float* __restrict__ slab,
                                                                     size_t pack_floats, int prior_only, Draws dw, int slab_chunks) {
  // blockIdx.y = Monte-Carlo draw: its pack, its rows, its chunk slabs
  pack += blockIdx.y * dw.pack; xr += blockIdx.y * dw.in; ar += blockIdx.y * dw.in2; slab += (size_t)blockIdx.y * slab_chunks * pack_floats;
  using L = RbfLayout<DI, DO>;
  constexpr int DH = (DO + 1) / 2;
  __shared__ __attribute__((aligned(16))) float sInd[2][64][4 * L::RQ2];
  __shared__ float sUni[TEAM][DH * DI];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float4* p4 = reinterpret_cast<const float4*>(pack);
  const float4* i4 = p4 + L::rff_f4(S);
  const float* wl = pack + 4 * (L::rff_f4(S) + L::ind_f4(M));
  const int r0 = blockIdx.x * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
  float* out = slab + (size_t)blockIdx.x * pack_floats;
  const int SJ = cdiv(S, 64), MJ = cdiv(M, 64);
  for (int rec = wave; rec < SJ * DO; rec += TEAM) {
    float4 rq[L::RQ];
    load_record<L::RQ>(p4, rec, lane, rq);
    float g[4 * L::RQ];
#pragma unroll
    for (int q = 0; q < 4 * L::RQ; ++q) g[q] = 0.f;
    const int d = rec % DO;
    for (int r = r0; r < r1; ++r) {
      float x[DI], gx[DI];
#pragma unroll
      for (int i = 0; i < DI; ++i) { x[i] = xr[(size_t)r * DI + i]; gx[i] = 0.f; }
      rbf_rff_bwd<DI, DO, true>(rq, x, ar[(size_t)r * DO + d], gx, g);
    }
#pragma unroll
    for (int q = 0; q < L::RQ; ++q) st4(out, ((size_t)rec * L::RQ + q) * 64 + lane, &g[4 * q]);
  }
  const int half = wave & 1;
  float gwl[DH][DI];
#pragma unroll
  for (int d = 0; d < DH; ++d)
#pragma unroll
    for (int i = 0; i < DI; ++i) gwl[d][i] = 0.f;
  float* ind_out = out + 4 * L::rff_f4(S);
  for (int jb = 0; jb < MJ; jb += 2) {
    const int j = jb + (wave >> 1);
    const bool valid = j < MJ;
    float4 ind[L::RQ2];
    float gi[4 * L::RQ2];
#pragma unroll
    for (int q = 0; q < 4 * L::RQ2; ++q) gi[q] = 0.f;
    if (valid) {
      load_record<L::RQ2>(i4, j, lane, ind);
      if (!prior_only) {
        for (int r = r0; r < r1; ++r) {
          asm volatile("" ::: "memory");   // as in the DF kernel below
          float x[DI], a[DO], gx[DI];
#pragma unroll
          for (int i = 0; i < DI; ++i) { x[i] = xr[(size_t)r * DI + i]; gx[i] = 0.f; }
#pragma unroll
          for (int i = 0; i < DO; ++i) a[i] = ar[(size_t)r * DO + i];
          rbf_ind_half_bwd<DI, DO, true>(ind, x, wl, half, a, gx, gi, gwl);
        }
      }
    }
    if (half == 1) {
#pragma unroll
      for (int q = 0; q < 4 * L::RQ2; ++q) sInd[wave >> 1][lane][q] = gi[q];
    }
    __syncthreads();
    if (half == 0 && valid) {
      float v[4 * L::RQ2];
#pragma unroll
      for (int q = 0; q < 4 * L::RQ2; ++q) v[q] = gi[q] + sInd[wave >> 1][lane][q];
#pragma unroll
      for (int q = 0; q < L::RQ2; ++q) st4(ind_out, ((size_t)j * L::RQ2 + q) * 64 + lane, &v[4 * q]);
    }
    __syncthreads();
  }
  {
    float flat[DH * DI], red[DH * DI];
#pragma unroll
    for (int e = 0; e < DH * DI; ++e) flat[e] = gwl[e / DI][e % DI];
    wave_sum_all<DH * DI>(flat, red);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < DH * DI; ++e) sUni[wave][e] = red[e];
    }
  }
  __syncthreads();
  if (threadIdx.x < DO * DI) {
    const int d = threadIdx.x / DI, i = threadIdx.x % DI;
    const int h = d / DH, dd = d % DH;
    float* uni_out = out + 4 * (L::rff_f4(S) + L::ind_f4(M));
    uni_out[d * DI + i] = sUni[h][dd * DI + i] + sUni[h + 2][dd * DI + i];
  }
}

// NP: column parts per inducing record (one wavefront each): 2 (halves) up to D = 8, 4 at D = 16 so that the uniform-parameter
// partials (2 x D x ceil(D/NP) registers) stay out of scratch
template <int D, int NP>
__global__ __launch_bounds__(256) void param_grad_df_stream_kernel(const float* __restrict__ pack, int M, int S,
                                                                    const float* __restrict__ xr, const float* __restrict__ ar,
                                                                    int R, int rows_per_chunk, float* __restrict__ slab,
                                                                    size_t pack_floats, int prior_only, Draws dw, int slab_chunks) {
  // blockIdx.y = Monte-Carlo draw: its pack, its rows, its chunk slabs
  pack += blockIdx.y * dw.pack; xr += blockIdx.y * dw.in; ar += blockIdx.y * dw.in2; slab += (size_t)blockIdx.y * slab_chunks * pack_floats;
  using L = DfLayout<D>;
  constexpr int DQ = (D + NP - 1) / NP;
  constexpr int NU = 2 * D * DQ + DQ;
  constexpr int RPI = TEAM / NP;                     // records per iteration of the inducing loop
  static_assert(TEAM % NP == 0, "column parts per team");
  __shared__ __attribute__((aligned(16))) float sInd[RPI][NP - 1][64][4 * L::RQ2];
  __shared__ float sUni[TEAM][NU];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float4* p4 = reinterpret_cast<const float4*>(pack);
  const float4* i4 = p4 + L::rff_f4(S);
  const float* uni = pack + 4 * (L::rff_f4(S) + L::ind_f4(M));
  const int r0 = blockIdx.x * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
  float* out = slab + (size_t)blockIdx.x * pack_floats;
  const int SJ = cdiv(S, 64), MJ = cdiv(M, 64);
  for (int rec = wave; rec < SJ * D; rec += TEAM) {
    float4 rq[L::RQ];
    load_record<L::RQ>(p4, rec, lane, rq);
    float g[4 * L::RQ];
#pragma unroll
    for (int q = 0; q < 4 * L::RQ; ++q) g[q] = 0.f;
    for (int r = r0; r < r1; ++r) {
      float x[D], a[D], gx[D];
#pragma unroll
      for (int i = 0; i < D; ++i) { x[i] = xr[(size_t)r * D + i]; a[i] = ar[(size_t)r * D + i]; gx[i] = 0.f; }
      df_rff_bwd<D, true>(rq, x, a, gx, g);
    }
#pragma unroll
    for (int q = 0; q < L::RQ; ++q) st4(out, ((size_t)rec * L::RQ + q) * 64 + lane, &g[4 * q]);
  }
  const int part = wave % NP, slot = wave / NP;
  float gwab[D][DQ], gil2[D][DQ], gvar[DQ];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < DQ; ++b) { gwab[a][b] = 0.f; gil2[a][b] = 0.f; }
#pragma unroll
  for (int b = 0; b < DQ; ++b) gvar[b] = 0.f;
  float* ind_out = out + 4 * L::rff_f4(S);
  for (int jb = 0; jb < MJ; jb += RPI) {
    const int j = jb + slot;
    const bool valid = j < MJ;
    float4 ind[L::RQ2];
    float gi[4 * L::RQ2];
#pragma unroll
    for (int q = 0; q < 4 * L::RQ2; ++q) gi[q] = 0.f;
    if (valid) {
      load_record<L::RQ2>(i4, j, lane, ind);
      if (!prior_only) {
        for (int r = r0; r < r1; ++r) {
          asm volatile("" ::: "memory");   // uniform-table loads stay in the loop (hoisted, 2 D^2 + D values spill)
          float x[D], a[D], gx[D];
#pragma unroll
          for (int i = 0; i < D; ++i) { x[i] = xr[(size_t)r * D + i]; a[i] = ar[(size_t)r * D + i]; gx[i] = 0.f; }
          df_ind_part_bwd<D, NP, true>(ind, x, uni, part, a, gx, gi, gwab, gil2, gvar);
        }
      }
    }
    if (part > 0) {
#pragma unroll
      for (int q = 0; q < 4 * L::RQ2; ++q) sInd[slot][part - 1][lane][q] = gi[q];
    }
    __syncthreads();
    if (part == 0 && valid) {
      float v[4 * L::RQ2];
#pragma unroll
      for (int q = 0; q < 4 * L::RQ2; ++q) {
        v[q] = gi[q];
#pragma unroll
        for (int pp = 0; pp < NP - 1; ++pp) v[q] += sInd[slot][pp][lane][q];
      }
#pragma unroll
      for (int q = 0; q < L::RQ2; ++q) st4(ind_out, ((size_t)j * L::RQ2 + q) * 64 + lane, &v[4 * q]);
    }
    __syncthreads();
  }
  {
    float flat[NU];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < DQ; ++b) { flat[a * DQ + b] = gwab[a][b]; flat[D * DQ + a * DQ + b] = gil2[a][b]; }
#pragma unroll
    for (int b = 0; b < DQ; ++b) flat[2 * D * DQ + b] = gvar[b];
    float red[NU];
    wave_sum_all<NU>(flat, red);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < NU; ++e) sUni[wave][e] = red[e];
    }
  }
  __syncthreads();
  {
    // column b belongs to part b / DQ; the wavefronts w = part, part + NP, ... hold its partials
    float* uni_out = out + 4 * (L::rff_f4(S) + L::ind_f4(M));
    for (int t = threadIdx.x; t < D * D; t += 256) {
      const int a = t / D, b = t % D, pt = b / DQ, bb = b % DQ;
      float v0 = 0.f, v1 = 0.f;
      for (int w = pt; w < TEAM; w += NP) { v0 += sUni[w][a * DQ + bb]; v1 += sUni[w][D * DQ + a * DQ + bb]; }
      uni_out[a * D + b] = v0;
      uni_out[D * D + a * D + b] = v1;
    }
    if (threadIdx.x < D) {
      const int t = threadIdx.x, pt = t / DQ, bb = t % DQ;
      float v = 0.f;
      for (int w = pt; w < TEAM; w += NP) v += sUni[w][2 * D * DQ + bb];
      uni_out[2 * D * D + t] = v;
    }
  }
}

// gpack[e] = sum_c slab[c][e] in a fixed order: 16 interleaved partial sums per element (independent load streams),
// combined through LDS.  grid = ceil(pack_floats / 64), block = 1024 (64 elements x 16 chunk groups).
__global__ __launch_bounds__(1024) void reduce_slab_kernel(const float* __restrict__ slab, int nchunk, size_t pack_floats,
                                                            float* __restrict__ gpack, int accumulate, size_t gpack_dstride, int slab_chunks) {
  __shared__ float red[16][64];
  slab += (size_t)blockIdx.y * slab_chunks * pack_floats; gpack += blockIdx.y * gpack_dstride;   // blockIdx.y = Monte-Carlo draw
  const int ex = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const size_t e = (size_t)blockIdx.x * 64 + ex;
  float acc = 0.f;
  if (e < pack_floats) {
#pragma unroll 8
    for (int c = cg; c < nchunk; c += 16) acc += slab[(size_t)c * pack_floats + e];
  }
  red[cg][ex] = acc;
  __syncthreads();
  if (cg == 0 && e < pack_floats) {
    float v = accumulate ? gpack[e] : 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) v += red[g][ex];
    gpack[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// What rollout_bwd_team_kernel reads of Draws: in = xstage, in2 = gzt, out = gz0, out2 = astage -- the record's rows in Di and in Do.
static Draws rollout_bwd_draws(int method, int Di, int Do, const RolloutBwdArgs& a, int nd, size_t pack_floats) {
  const size_t rows = record_rows(a.N, a.T, a.substeps, method);
  Draws d;
  d.nd = nd; d.pack = pack_floats;
  d.in = rows * Di; d.in2 = (size_t)a.N * a.T * Di;
  d.out = (size_t)a.N * Di; d.out2 = rows * Do;
  d.ts = a.ts_per_traj ? (size_t)a.T : 0; d.sub = a.substeps;
  return d;
}

// The register-resident or the streamed team, and the grid: reverse_route (gp_rollout.hpp).
int rollout_bwd(int kernel, int order, int method, int Di, int Do, const RolloutBwdArgs& a, int nd, hipStream_t st) {
  static const char* const who = "gpode_rollout_bwd";
  static const char* const tags[2][2] = {{"rollout_bwd_rbf", "rollout_bwd_rbf_stream"}, {"rollout_bwd_df", "rollout_bwd_df_stream"}};
  size_t pf = 0;
  if (cache_sizes(kernel, Di, Do, a.M, a.S, &pf, nullptr)) return 1;
  if (method < 0 || method > 2) return set_error("gpode_rollout_bwd: method %d (0 euler, 1 rk4, 2 midpoint; 3 dopri5: gpode_rollout_adaptive_bwd_n)", method);
  if (kernel != 0 && order != 1) return set_error("gpode_rollout_bwd: DF kernel is first-order only");
  const Draws dw = rollout_bwd_draws(method, Di, Do, a, nd, pf);
  return dispatch_dims(who, kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return dispatch_order<DI, DO>(who, order, [&](auto o) {
      return dispatch_method(method, [&](auto m) {
        constexpr int ORDER = decltype(o)::value, METHOD = decltype(m)::value;
        return reverse_route<KERNEL, DI, DO>(a.N, a.M, a.S, [&](auto ev, const LaunchGeom& g) {
          using EV = typename decltype(ev)::type;
          return dispatch_substeps(dw.sub, [&](auto sb) {
            if (launch_route(rollout_bwd_team_kernel<EV, DI, DO, ORDER, METHOD, false, decltype(sb)::value>, g, nd, st, a.pack, a.M, a.S, a.xstage,
                             a.gzt, a.ts, a.N, a.T, a.gz0, a.astage, dw, (float*)nullptr, (size_t)0))
              return 1;
            return check_launch(tags[KERNEL][g.route]);
          });
        });
      });
    });
  });
}

// ---- reverse sweep + parameter sums in one pass (rollout_bwd_team_kernel<..., PG = true>) --------------------------------------
// Built for the first-order register-resident teams of the widths below and the Euler / 3-8-rule solvers; pgrad_chunks() = 0 for
// every other shape: the caller then runs rollout_bwd and param_grad separately.
// (RBF widths up to 6: 376 registers at q = 6 with the 3/8 rule.  q = 8 spills 181 registers, and the divergence-free kernel, whose
//  parameter-sum kernel alone takes 432, spills 945 -- besides, at configs[1] its sums (168 us) sit on the side branch, and moving them
//  into the main branch's sweep lengthens the chain the encoder's backward follows by about what the side branch gets shorter)
#define GP_PGRAD_RBF_DIMS(X) X(6) X(4) X(2) X(3)
// f(int_c<D>) for a width the fused form is built for, 0 for every other
template <class F> static int pgrad_width(int kernel, int Do, F&& f) {
  if (kernel == 0) {
#define X(d) if (Do == d) return f(int_c<d>{});
    GP_PGRAD_RBF_DIMS(X)
#undef X
  }
  return 0;
}
int rollout_bwd_pgrad_chunks(int kernel, int order, int method, int Di, int Do, int M, int S, int N) {
  if (order != 1 || Di != Do || (method != 0 && method != 1) || N < 1) return 0;
  return pgrad_width(kernel, Do, [&](auto d) { return rbf_team_ok<decltype(d)::value, decltype(d)::value>(M, S) ? team_grid(N) : 0; });
}
int rollout_bwd_pgrad(int kernel, int order, int method, int Di, int Do, const RolloutBwdArgs& a, int nd, hipStream_t st) {
  size_t pf = 0;
  if (cache_sizes(kernel, Di, Do, a.M, a.S, &pf, nullptr)) return 1;
  const int grid = rollout_bwd_pgrad_chunks(kernel, order, method, Di, Do, a.M, a.S, a.N);
  if (grid == 0) return set_error("gpode_rollout_bwd_pgrad: no fused form for kernel=%d order=%d method=%d Di=%d Do=%d M=%d S=%d", kernel, order,
                                  method, Di, Do, a.M, a.S);
  if (a.nchunk != grid) return set_error("gpode_rollout_bwd_pgrad: slab for %d chunks, the launch has %d", a.nchunk, grid);
  const Draws dw = rollout_bwd_draws(method, Di, Do, a, nd, pf);
  const LaunchGeom g{kRouteTeam, grid, 256, 0};      // one chunk slab per workgroup of the register-resident team
  const int done = pgrad_width(kernel, Do, [&](auto d) {
    constexpr int D = decltype(d)::value;
    const auto sweep = [&](auto m) {                 // Euler and the 3/8 rule only (rollout_bwd_pgrad_chunks): no midpoint instantiation
      return dispatch_substeps(dw.sub, [&](auto sb) {
        return launch_route(rollout_bwd_team_kernel<RbfTeamEval<D, D, 1>, D, D, 1, decltype(m)::value, true, decltype(sb)::value>, g, nd, st,
                            a.pack, a.M, a.S, a.xstage, a.gzt, a.ts, a.N, a.T, a.gz0, a.astage, dw, a.slab, pf);
      });
    };
    if (method == 0) sweep(int_c<0>{});
    else sweep(int_c<1>{});
    return 1;
  });
  if (!done) return set_error("gpode_rollout_bwd_pgrad: width %d not built", Do);
  if (check_launch("rollout_bwd_pgrad")) return 1;
  // the chunk slabs -> the pack-layout gradient of every draw (gpack is dense per draw)
  hipLaunchKernelGGL(reduce_slab_kernel, dim3((unsigned)((pf + 63) / 64), nd), 1024, 0, st, a.slab, grid, pf, a.gpack, 0, pf, grid);
  return check_launch("reduce_slab");
}

int rhs_vjp(int kernel, int Di, int Do, int M, int S, const float* pack, const float* x, const float* a, int R, float* gx,
            int prior_only, hipStream_t st, Draws dw) {
  static const char* const tags[2][2] = {{"rhs_vjp_rbf", "rhs_vjp_rbf_stream"}, {"rhs_vjp_df", "rhs_vjp_df_stream"}};
  if (R <= 0) return 0;
  return dispatch_dims("gpode_rhs_vjp", kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int KERNEL = decltype(k)::value, DI = decltype(di)::value, DO = decltype(dO)::value;
    return reverse_route<KERNEL, DI, DO>(R, M, S, [&](auto ev, const LaunchGeom& g) {
      using EV = typename decltype(ev)::type;
      if (launch_route(rhs_vjp_team_kernel<EV, DI, DO>, g, dw.nd, st, pack, M, S, x, a, R, gx, prior_only, dw)) return 1;
      return check_launch(tags[KERNEL][g.route]);
    });
  });
}

// rows (R,Di) x adjoints (R,Do) -> gpack (pack layout).  slab: nchunk * pack_floats floats of scratch.
template <int DI, int DO>
static int launch_pgrad_rbf(const float* pack, int M, int S, const float* xr, const float* ar, int R, int rpc, int used, float* slab,
                            size_t pf, int prior_only, hipStream_t st, Draws dw, int nchunk) {
  if constexpr (DO <= 8) {
    if (rbf_team_ok<DI, DO>(M, S)) {
      hipLaunchKernelGGL((param_grad_rbf_kernel<DI, DO, 1>), dim3(used, dw.nd), 256, 0, st, pack, M, S, xr, ar, R, rpc, slab, pf, prior_only, dw, nchunk);
      return check_launch("param_grad_rbf");
    }
  }
  hipLaunchKernelGGL((param_grad_rbf_stream_kernel<DI, DO>), dim3(used, dw.nd), 256, 0, st, pack, M, S, xr, ar, R, rpc, slab, pf, prior_only, dw, nchunk);
  return check_launch("param_grad_rbf_stream");
}

template <int D>
static int launch_pgrad_df(const float* pack, int M, int S, const float* xr, const float* ar, int R, int rpc, int used, float* slab,
                           size_t pf, int prior_only, hipStream_t st, Draws dw, int nchunk) {
  if constexpr (D <= 8) {
    if (df_team_ok<D>(M, S)) {
      // many rows (the rows of a training step): the pack split over two co-resident workgroups per chunk
      if constexpr (D == 6) {
        if (R >= 1024) {
          hipLaunchKernelGGL((param_grad_df_split_kernel<D>), dim3(used, dw.nd, 2), 256, 0, st, pack, M, S, xr, ar, R, rpc, slab, pf, prior_only, dw, nchunk);
          return check_launch("param_grad_df_split");
        }
      }
      hipLaunchKernelGGL((param_grad_df_kernel<D, 1>), dim3(used, dw.nd), 256, 0, st, pack, M, S, xr, ar, R, rpc, slab, pf, prior_only, dw, nchunk);
      return check_launch("param_grad_df");
    }
  }
  hipLaunchKernelGGL((param_grad_df_stream_kernel<D, (D > 8 ? 4 : 2)>), dim3(used, dw.nd), 256, 0, st, pack, M, S, xr, ar, R, rpc, slab, pf, prior_only, dw, nchunk);
  return check_launch("param_grad_df_stream");
}

int param_grad(int kernel, int Di, int Do, int M, int S, const float* pack, const float* xr, const float* ar, int R,
               float* slab, int nchunk, float* gpack, int accumulate, int prior_only, hipStream_t st, Draws dw) {
  size_t pf = 0;
  if (cache_sizes(kernel, Di, Do, M, S, &pf, nullptr)) return 1;
  if (R <= 0 || nchunk <= 0) return set_error("gpode_param_grad: R=%d nchunk=%d", R, nchunk);
  const int rpc = cdiv(R, nchunk);
  const int used = cdiv(R, rpc);
  // the parameter-sum kernels are not templated on an evaluator: their own choice, on the predicate of the reverse side
  const int rc = dispatch_dims("gpode_param_grad", kernel, Di, Do, [&](auto k, auto di, auto dO) {
    constexpr int DI = decltype(di)::value, DO = decltype(dO)::value;
    if constexpr (decltype(k)::value == 0) return launch_pgrad_rbf<DI, DO>(pack, M, S, xr, ar, R, rpc, used, slab, pf, prior_only, st, dw, nchunk);
    else return launch_pgrad_df<DO>(pack, M, S, xr, ar, R, rpc, used, slab, pf, prior_only, st, dw, nchunk);
  });
  if (rc) return rc;
  const char* route = *last_launch_slot();           // which parameter-sum kernel ran: what the entry point reports (tests/integrator_routes.py)
  hipLaunchKernelGGL(reduce_slab_kernel, dim3((unsigned)((pf + 63) / 64), dw.nd), 1024, 0, st, slab, used, pf, gpack, accumulate, dw.out, nchunk);
  if (check_launch("reduce_slab")) return 1;
  *last_launch_slot() = route;
  return 0;
}

}  // namespace gp
