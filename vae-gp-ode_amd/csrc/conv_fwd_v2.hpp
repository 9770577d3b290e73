// conv_fwd_v2.hpp -- forward of decnn.7 (ConvTranspose2d 32 -> 16, 13 -> 28, vae.py:113-121) on the fp32 matrix cores, second engine:
// the forward variant of conv_bwd_v2.hpp (PRODUCER / CONSUMER wavefronts, weights resident in the consumers' registers).
//
//   y[co][oy][ox] = bias[co] + sum_{ci,ky,kx} x[ci][iy][ix] w[ci][co][ky][kx],   oy = S iy - P + ky         (gather form)
//
// Geometry is the first engine's (conv_mfma.hpp, FwdPolicy<L>::C<cls>): one GEMM per stride-parity class cls = py S + px,
// D[co][pixel] = sum_k W[co][k] X[k][pixel], k = (tap, 4 source channels) per v_mfma_f32_16x16x4_f32, A := weights, B := pixels, so a
// lane ends up with one pixel and four channels of a tile.  The four classes of decnn.7 have 9 / 6 / 6 / 4 taps (72 / 48 / 48 / 32
// k-steps) and the same 14 x 14 grid of q-positions: pixel q of class (py, px) is output (2 qy + py - 1, 2 qx + px - 1).
//
//   * Weights in registers.  The A fragments of all 200 k-steps of the layer's single 16-channel co tile are loaded once per launch;
//     a consumer holds all of them (one consumer per SIMD, two wavefronts per SIMD, 256 registers each, as k_conv_bwd_data_v2<Dec4>).
//     The k-loop reads ONE LDS operand per MFMA at a per-lane base computed once per tile plus a compile-time offset per k-step.  Tap
//     shifts are negative in the gather form: the largest shift is folded into the lane base, so every offset is a non-negative
//     immediate of the ds_read.
//   * The q-positions of a workgroup's images form ONE stream cut into windows of 128 = 8 tiles regardless of image boundaries; SIMD s
//     takes tiles s and s + 4 of every window through all four classes: 2 x 200 MFMAs per SIMD and window.  The two column-parity
//     classes of a row parity run back to back in one k-loop (120 and 80 steps), and the lane then stores float2{px = 1, px = 0} --
//     neighbouring output columns -- exactly as the first engine's PAIR form does.
//   * A ring of NBUF = 3 zero-padded single-image plane buffers (38.9 KB each); the padding is written once.  Four producer
//     wavefronts (one per SIMD, raised priority) stream the next window's images from HBM into the free buffers: all loads first
//     with clamped indices, then the LDS stores, BatchNorm + ReLU of the source (bn_math.hpp, the arithmetic the backward recomputes
//     the ReLU mask with) applied on the way.  The {mean, invstd, gamma, beta} table sits in the unused plane tails of buffer 0.
//     ONE workgroup barrier per window.
//   * STATS: the BatchNorm statistics of the output are summed by the producers from the stored output, lane by lane in the order
//     of the first engine, whose image groups, grid and reduction the kernel keeps, so that they are bit-identical to the first
//     engine's (a float sum depends on its order, and these sums reach every gradient of a training step); finalised by the last
//     workgroup (bn_sink.hpp).
#pragma once
#include "conv_mfma.hpp"

namespace gp {

template <class L> struct FwV2 {
  using PL = FwdPolicy<L, L::CO>;                    // geometry: plane stride, classes, tap shifts, pixel addresses, output offsets
  template <int CLS> using C = typename PL::template C<CLS>;
  static constexpr int KC = L::CI, NC = L::CO, KK = L::K * L::K, KG = KC / 4;
  static_assert(NC == 16 && L::S == 2 && PL::NCLS == 4, "one co tile, four stride-parity classes");
  static constexpr int NKS = KK * KG;                // k-steps of all classes: (class, tap, 4 source channels), class-major
  static constexpr int NPX = C<0>::npc;              // q-positions per image (the same grid in every class)
  static_assert(C<1>::npc == NPX && C<2>::npc == NPX && C<3>::npc == NPX && C<1>::nx == C<0>::nx && C<2>::nx == C<0>::nx &&
                C<3>::nx == C<0>::nx, "the classes share one q-grid");
  static constexpr int SH = L::HI, OHW = L::HO * L::HO;
  static constexpr int SRC = KC * SH * SH;           // source floats per image
  static constexpr int PS = PL::PS, HP = PL::HP, PADL = PL::PADL, IMG = KC * PS;
  static constexpr int NCW = 4, NTHR = 64 * (NCW + 4), NLT = NTHR - 64 * NCW;
  static constexpr int TPW = 2;                      // tiles per consumer per window
  static constexpr int WIN = 16 * NCW * TPW;         // q-positions per window
  static constexpr int PF = 2;                       // k-steps of operands in flight ahead of the MFMAs
  static constexpr int NBUF = (2 * WIN - 2) / NPX + 2;   // images two consecutive windows can touch
  static constexpr int MAXS = PADL * (HP + 1);       // largest tap shift (PADL rows and PADL columns back), folded into the lane base
  static constexpr int TFO = (HP * HP + 3) / 4 * 4;  // in_bn entry of a plane's channel, behind the plane (buffer 0)
  static_assert(igemm_tf_in_pad<PL>(), "the input-transform table fits the plane tails");
  static_assert(TPW * (PF + 1) <= 15, "LDS reads in flight within what lgkmcnt counts");
  static_assert(NPX <= 256 && SRC % 4 == 0 && SH * SH <= NLT, "float4 source, producer offset table");
  // LDS byte offsets relative to the lane's base: 0 <= MAXS + tap_off <= MAXS, plus the group of four source channels
  static_assert(4 * (MAXS + (KG - 1) * 4 * PS) < 65536, "operand offsets fit the ds_read immediate");
  static constexpr int CST = NBUF * IMG;             // [2][NC]: bias, statistics shift (read at the epilogue: not live across the k-loop)
  // STATS sums the output exactly as the first engine does (k_conv_igemm<FwdPolicy<L, 16>, IPG, 4, 1, true, 512, true>): groups of IPG
  // images per workgroup, NSW wavefronts that split a group's (row parity, tile) jobs by cost, one partial sum per wavefront and lane
  static constexpr int IPG = 2, NSW = 8;
  static constexpr int RED = CST + 2 * NC;           // STATS: [NSW][NC][2] wavefront sums, then [NC][2] workgroup sums
  static constexpr size_t lds_bytes(bool stats) { return sizeof(float) * ((size_t)RED + (stats ? (NSW + 1) * 2 * NC : 0)); }
};

// one window's tiles of one consumer through the two column-parity classes of row parity PY: k-steps [0, N0) belong to class 2 PY
// (px = 0), [N0, N) to class 2 PY + 1.  The operands of step s + PF are requested, unconditionally, in front of the MFMAs of step s;
// sched_barrier keeps the order.
template <class E, int PY>
__device__ __forceinline__ void fwv2_pair(const float* __restrict__ s_buf, const int (&base)[2][E::TPW], const float (&wr)[E::NKS],
                                          f32x4 (&acc)[2][E::TPW]) {
  using G0 = typename E::template C<2 * PY>;
  using G1 = typename E::template C<2 * PY + 1>;
  constexpr int N0 = G0::ntaps * E::KG, N = N0 + G1::ntaps * E::KG, W0 = G0::slab_taps * E::KG;
  static_assert(G1::slab_taps == G0::slab_taps + G0::ntaps, "class-major weight registers");
  float bf[E::PF + 1][E::TPW];
  auto fetch = [&](auto sc) {
    constexpr int S = decltype(sc)::value, c = S >= N0 ? 1 : 0, s = c ? S - N0 : S;
    const int off = E::MAXS + (c ? G1::tap_off(s / E::KG) : G0::tap_off(s / E::KG)) + (s % E::KG) * 4 * E::PS;
#pragma unroll
    for (int t = 0; t < E::TPW; ++t) bf[S % (E::PF + 1)][t] = s_buf[base[c][t] + off];
  };
#pragma unroll
  for (int t = 0; t < E::TPW; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  static_for<E::PF>([&](auto sc) { fetch(sc); });
  static_for<N>([&](auto sc) {
    constexpr int S = decltype(sc)::value, c = S >= N0 ? 1 : 0;
    if constexpr (S + E::PF < N) fetch(std::integral_constant<int, S + E::PF>{});
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < E::TPW; ++t) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[W0 + S], bf[S % (E::PF + 1)][t], acc[c][t], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  });
}

// grid.x <= number of CUs (with STATS: min(image groups, CUs), the first engine's grid), block FwV2::NTHR, LDS FwV2::lds_bytes(STATS)
template <class L, bool HAS_BN, bool STATS>
__global__ __launch_bounds__(FwV2<L>::NTHR) void k_conv_fwd_v2(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ y, int B,
                                                               const float* __restrict__ in_bn, BnSink sink) {
  using E = FwV2<L>;
  constexpr int KC = E::KC, NC = E::NC, KK = E::KK, KG = E::KG, NPX = E::NPX, IMG = E::IMG, PS = E::PS, HP = E::HP, WIN = E::WIN;
  constexpr int SH = E::SH, PADL = E::PADL, NLT = E::NLT, NBUF = E::NBUF, TPW = E::TPW, NCW = E::NCW, OHW = E::OHW;
  float* s_buf = igemm_smem;                         // [NBUF][KC][PS] zero-padded planes, index (iy + PADL) * HP + ix + PADL
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // images of this workgroup: image j is blockIdx.x + j gridDim.x; with STATS the first engine's assignment, groups of IPG consecutive
  // images, group k of the workgroup = group blockIdx.x + k gridDim.x (the statistics are summed per workgroup, in its order)
  const int bx = blockIdx.x, ngx = gridDim.x, ngroups = (B + E::IPG - 1) / E::IPG;
  const int ngrp = bx < ngroups ? (ngroups - 1 - bx) / ngx + 1 : 0;
  const int nit = STATS ? (ngrp ? E::IPG * (ngrp - 1) + min(E::IPG, B - E::IPG * (bx + (ngrp - 1) * ngx)) : 0)
                        : (bx < B ? (B - 1 - bx) / ngx + 1 : 0);
  auto img = [&](int j) { return STATS ? E::IPG * (bx + (j / E::IPG) * ngx) + j % E::IPG : bx + j * ngx; };
  const int npx = nit * NPX, nwin = (npx + WIN - 1) / WIN;
  // last image a window reads (window i covers stream positions [i WIN, i WIN + WIN) of the workgroup)
  auto last_img = [&](int i) { return min(nit - 1, (i * WIN + WIN - 1) / NPX); };

  // the padding is written here and never again
  for (int e = tid; e < NBUF * IMG / 4; e += E::NTHR) reinterpret_cast<float4*>(s_buf)[e] = float4{0.f, 0.f, 0.f, 0.f};
  if (tid < NC) {
    s_buf[E::CST + tid] = bias ? bias[tid] : 0.f;
    s_buf[E::CST + NC + tid] = STATS ? bn_sink_shift(sink, tid) : 0.f;
  }
  __syncthreads();
  if constexpr (HAS_BN) {
    for (int e = tid; e < KC; e += E::NTHR) *reinterpret_cast<float4*>(s_buf + e * PS + E::TFO) = reinterpret_cast<const float4*>(in_bn)[e];
    __syncthreads();
  }
  // STATS: sums of (y - k), (y - k)^2 of the first engine's wavefronts pw and pw + 4 (its cost ranks 2 pw, 2 pw + 1), kept by producer pw
  float bs[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, bq[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  if (wave >= NCW) {
    // producer: image j of the workgroup -> buffer j % NBUF.  All loads first, then the stores.
    __builtin_amdgcn_s_setprio(3);
    const int lt = tid - 64 * NCW;
    constexpr int N4 = E::SRC / 4;
    // the SH * SH float4 of a group of four planes go to the first SH * SH producer threads, each with the planes and plane offsets
    // of its four elements in registers (group g adds 4 g planes)
    int otab[4], opl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * min(lt, SH * SH - 1) + k, pl = e / (SH * SH), q = e % (SH * SH);
      opl[k] = pl * PS;
      otab[k] = pl * PS + (q / SH + PADL) * HP + q % SH + PADL;
    }
    auto stage = [&](int j) __attribute__((always_inline)) {
      const float4* src = reinterpret_cast<const float4*>(x) + (size_t)img(j) * N4;
      float* buf = s_buf + (j % NBUF) * IMG;
      if (lt < SH * SH) {
        float4 v[KG];
#pragma unroll
        for (int g = 0; g < KG; ++g) v[g] = src[g * SH * SH + lt];
#pragma unroll
        for (int g = 0; g < KG; ++g) {
          float* d = buf + 4 * g * PS;
          float e[4] = {v[g].x, v[g].y, v[g].z, v[g].w};
          if constexpr (HAS_BN) {
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = bn_relu(e[k], *reinterpret_cast<const float4*>(s_buf + 4 * g * PS + opl[k] + E::TFO));
          }
          d[otab[0]] = e[0]; d[otab[1]] = e[1]; d[otab[2]] = e[2]; d[otab[3]] = e[3];
        }
      }
    };
    // images [0, last_img(0)] before window 0; during window i those of window i + 1 not yet staged.  The oldest image window i reads
    // is newer than last_img(i + 1) - NBUF (NBUF covers the span of two windows), so those buffers are free.
    // STATS.  The output is bit-identical to the first engine's whatever the tiling, but a sum of floats depends on its order, and
    // the statistics feed every gradient of the step.  So the producers, which idle most of a window, sum them from the output the
    // consumers have stored (read back through L2 once a whole group is stored), lane by lane in the first engine's order.
    // Visibility: the consumers' plain global stores of a window precede the workgroup barrier that ends it, the loads here follow
    // it; a workgroup-scope release / acquire pair (__syncthreads) orders global memory between the wavefronts of a workgroup, which
    // share the CU's vector cache (the kernel is not compiled for threadgroup-split mode).  A group is read only after ALL of it is
    // stored, so no cache line fetched here holds bytes of this workgroup that are written later.
    // The first engine's wavefront of cost rank jw takes the jobs whose cost midpoint lies in [wtot jw / NSW, wtot (jw + 1) / NSW),
    // row parity 0 first, tiles ascending, lane lr the group's position 16 tile + lr, even column before odd (k_conv_igemm's jobs();
    // a change of that split breaks the identity, which tests/test_gpu_conv_fwd_v2.py asserts).
    const int pw = wave - NCW, slr = lane & 15, slk = lane >> 4;
    float kk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) kk[r] = STATS ? s_buf[E::CST + NC + 4 * slk + r] : 0.f;
    auto stats_group = [&](int k) __attribute__((always_inline)) {
      const int b0 = E::IPG * (bx + k * ngx), mtot = min(E::IPG, B - b0) * NPX, njobs = (mtot + 15) / 16;
      constexpr int NT0 = E::template C<0>::ntaps + E::template C<1>::ntaps, NT1 = E::template C<2>::ntaps + E::template C<3>::ntaps;
      const int wtot = njobs * (NT0 + NT1);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int jw = 2 * pw + e, lo = (wtot * jw) / E::NSW, hi = (wtot * (jw + 1)) / E::NSW;
        static_for<2>([&](auto pyc) {
          constexpr int PY = decltype(pyc)::value, ntaps = PY ? NT1 : NT0;
          using G1 = typename E::template C<2 * PY + 1>;
          const int cbase = PY ? njobs * NT0 : 0;
          const int nlo = lo - cbase - ntaps / 2, nhi = hi - cbase - ntaps / 2;
          const int ub = min(njobs, nlo <= 0 ? 0 : (nlo + ntaps - 1) / ntaps), ue = min(njobs, nhi <= 0 ? 0 : (nhi + ntaps - 1) / ntaps);
          constexpr int U = 8;                       // tiles whose loads are in flight together
          for (int u0 = ub; u0 < ue; u0 += U) {
            float2 v[U][4];
#pragma unroll
            for (int t = 0; t < U; ++t) {
              const int m = min((u0 + t) * 16 + slr, mtot - 1), im = m / NPX, p = m - im * NPX;
              const float* yp = y + ((size_t)(b0 + im) * NC + 4 * slk) * OHW + G1::out_off(p);
#pragma unroll
              for (int r = 0; r < 4; ++r) v[t][r] = *reinterpret_cast<const float2*>(yp + (size_t)r * OHW);
            }
#pragma unroll
            for (int t = 0; t < U; ++t) {
              if (u0 + t < ue && (u0 + t) * 16 + slr < mtot) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float d1 = v[t][r].x - kk[r], d0 = v[t][r].y - kk[r];
                  bs[e][r] += d1; bq[e][r] = fmaf(d1, d1, bq[e][r]);
                  bs[e][r] += d0; bq[e][r] = fmaf(d0, d0, bq[e][r]);
                }
              }
            }
          }
        });
      }
    };
    int staged = -1, summed = 0;
    if (nit > 0)
      for (; staged < last_img(0); ) stage(++staged);
    __syncthreads();
    for (int i = 0; i < nwin; ++i) {
      if (i + 1 < nwin)
        for (const int j1 = last_img(i + 1); staged < j1; ) stage(++staged);
      if constexpr (STATS) {
        // groups stored completely by the windows before this one (a cache line of y never holds data this workgroup reads later)
        __builtin_amdgcn_s_setprio(0);
        for (; summed < ngrp && min(npx, E::IPG * NPX * (summed + 1)) <= i * WIN; ++summed) stats_group(summed);
        __builtin_amdgcn_s_setprio(3);
      }
      __syncthreads();                               // window i consumed, window i + 1's images staged
    }
    __builtin_amdgcn_s_setprio(0);
    if constexpr (STATS)
      for (; summed < ngrp; ++summed) stats_group(summed);
  } else {
    // consumer: tiles wave and wave + NCW of every window, all four classes
    const int lr = lane & 15, lk = lane >> 4;
    float wr[E::NKS];                                // A fragment of class c, k-step s: w[ci = 4 (s % KG) + lk][co = lr][tap s / KG of c]
    static_for<4>([&](auto cc) {
      using G = typename E::template C<decltype(cc)::value>;
#pragma unroll
      for (int s = 0; s < G::ntaps * KG; ++s) {
        const int t = s / KG, ky = G::py + L::S * (t / G::ntx), kx = G::px + L::S * (t % G::ntx);
        wr[G::slab_taps * KG + s] = w[((size_t)(4 * (s % KG) + lk) * NC + lr) * KK + ky * L::K + kx];
      }
    });
    __syncthreads();                                 // window 0's images staged
    for (int i = 0; i < nwin; ++i) {
      const int t0 = i * WIN + 16 * wave;            // stream position of tile 0's lane 0; tile t starts 16 NCW t further
      if (t0 < npx) {                                // wave-uniform: the window holds positions of this consumer
        // per tile ONE register lives across the k-loops: (image j of the workgroup) << 8 | position in the image; what the operand
        // addresses and the stores need is derived from it where it is used
        int jp[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const int m = min(t0 + 16 * NCW * t + lr, npx - 1);   // past the end: alias the last position (resident), masked at the store
          const int j = m / NPX;
          jp[t] = j << 8 | (m - j * NPX);
        }
        static_for<2>([&](auto pyc) {
          constexpr int PY = decltype(pyc)::value;
          using G0 = typename E::template C<2 * PY>;       // px = 0: odd output columns
          using G1 = typename E::template C<2 * PY + 1>;   // px = 1: even output columns
          static_assert(G0::out_off(0) == G1::out_off(0) + 1 && G0::out_off(NPX - 1) == G1::out_off(NPX - 1) + 1 &&
                        G1::out_off(0) % 2 == 0 && L::HO % 2 == 0, "paired classes write neighbouring, 8-byte aligned columns");
          int base[2][TPW];
#pragma unroll
          for (int t = 0; t < TPW; ++t) {
            const int lb = ((jp[t] >> 8) % NBUF) * IMG + lk * PS - E::MAXS;
            base[0][t] = lb + G0::pix_addr(jp[t] & 255);
            base[1][t] = lb + G1::pix_addr(jp[t] & 255);
          }
          f32x4 acc[2][TPW];
          fwv2_pair<E, PY>(s_buf, base, wr, acc);
          // lane: position mm[t], channels 4 lk + r, columns (even, odd) = (px = 1, px = 0)
          const float4 b4 = *reinterpret_cast<const float4*>(s_buf + E::CST + 4 * lk);
          const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int t = 0; t < TPW; ++t) {
            int c = jp[t];
            asm volatile("" : "+v"(c));              // a fresh value: nothing derived from jp[t] above stays live through the k-loop
            if (t0 + 16 * NCW * t + lr < npx) {
              const int j = c >> 8;
              float* yp = y + ((size_t)img(j) * NC + 4 * lk) * OHW + G1::out_off(c & 255);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float v0 = acc[0][t][r] + bv[r], v1 = acc[1][t][r] + bv[r];
                *reinterpret_cast<float2*>(yp + (size_t)r * OHW) = float2{v1, v0};
              }
            }
          }
        });
      }
      __syncthreads();                               // window i consumed, window i + 1's images staged
    }
  }

  if constexpr (STATS) {
    // as the first engine: over the 16 lanes of a row, then over its wavefronts in order through LDS (behind the buffers); producer pw
    // holds the sums of wavefronts pw and pw + NCW
    float* red = s_buf + E::RED;                     // [NSW][NC][2]
    float* s_sm = red + E::NSW * 2 * NC;             // [NC][2]
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = row_allreduce16(bs[e][r]), b = row_allreduce16(bq[e][r]);
        if (lr == 0 && wave >= NCW) {
          red[((wave - NCW + NCW * e) * NC + 4 * lk + r) * 2] = a;
          red[((wave - NCW + NCW * e) * NC + 4 * lk + r) * 2 + 1] = b;
        }
      }
    __syncthreads();
    if (tid < 2 * NC) {
      float t = 0.f;
      for (int wv = 0; wv < E::NSW; ++wv) t += red[wv * 2 * NC + tid];
      s_sm[tid] = t;
    }
    __syncthreads();
    bn_sink_publish<NC, E::NTHR>(sink, s_sm);
  }
}

}  // namespace gp
