// conv_bwd_v2.hpp -- d/d input of decnn.7 (ConvTranspose2d 32 -> 16, 13 -> 28) and decnn.4 (64 -> 32, 6 -> 13) (vae.py:113-121) on
// the fp32 matrix cores, second engine: PRODUCER / CONSUMER wavefronts with the weights resident in the consumers' registers.
//
//   gx[ci][iy][ix] = sum_{co,ky,kx} gy[co][S iy - P + ky][S ix - P + kx] w[ci][co][ky][kx]        (an ordinary strided convolution)
//
// Same GEMM view, plane layout and geometry as the first engine (conv_mfma.hpp, BwdDataPolicy): D[ci][pixel] = sum_k W[ci][k] X[k][pixel],
// k = (tap, 4 source channels) per v_mfma_f32_16x16x4_f32, A := weights, B := pixels, so a lane ends up with one pixel and four
// channels of a tile.  What changed is where the operands live and who does what:
//
//   * Weights in registers.  A wavefront owns one 16-channel ci tile, and the A fragments of all k-steps of that tile (16 ci x KC co
//     x 25 taps / 64 lanes: 100 VGPRs for decnn.7, 200 for decnn.4) are loaded once per launch.  The k-loop then reads ONE LDS operand
//     per MFMA (the first engine: two), at a per-lane base computed once per tile plus a compile-time offset per k-step -- a tap is a
//     constant shift in the zero-padded plane, a group of four source channels a constant number of planes -- that fits the ds_read
//     offset field.
//     (32x32x2 would halve the operand reads per flop as well, but its A fragments for 32 ci are 200 VGPRs for decnn.7: the weights
//     would have to stay in LDS, 51 KB, and the third plane buffer below would not fit.)
//   * A ring of single-image plane buffers (no weight slabs).  The pixels of a workgroup's images form ONE stream that is cut into
//     windows of WIN pixels regardless of image boundaries: a tile may take its first pixels from one image and the rest from the
//     next, and only the last window of a workgroup is partial.  While a window is multiplied the buffers it does not read take the
//     images the next window needs; NBUF covers the images the two windows span together.
//   * decnn.7 (100 weight VGPRs: two consumers per SIMD fit the 168-register cap of three wavefronts per SIMD): 8 consumers, windows of
//     128 pixels = 8 tiles, 3 buffers of 53.8 KB.  Wavefront w takes ci tile w >> 2 of tiles (w & 3) and (w & 3) + 4 of every window,
//     so the two consumers of a SIMD (w, w + 4) split the same pixel tiles by channels.  169 pixels per image quantised per image to 11
//     tiles of 16 would waste 4 % (to 6 tiles of 32: 12 %).
//   * decnn.4 (200 weight VGPRs: one consumer per SIMD, two wavefronts per SIMD, 256 registers each): 4 consumers, wavefront w owns ci
//     tile w and takes all 4 tiles of every window of 64 pixels.  An image has only 36 pixels, so a window touches up to three images
//     and two consecutive windows up to five: 5 buffers of 28.8 KB.  At 4096 images a CU gets 16 images = 576 pixels = 9 windows.
//     With one consumer on its SIMD, the operands of the next PF k-steps of all 4 tiles are in flight in front of every step's MFMAs
//     (TPW (PF + 1) = 12 reads, within what lgkmcnt counts).
//   * Either way every SIMD issues the same MFMAs per window, and four producer wavefronts (one per SIMD, raised priority as in
//     conv_wgrad_v2.hpp) stream the next images from HBM into the free buffers.  ONE workgroup barrier per window.
#pragma once
#include "conv_mfma.hpp"

namespace gp {

template <class L> struct BdV2 {
  using PL = BwdDataPolicy<L, L::CI>;                // geometry: plane stride, tap shifts, pixel addresses
  static constexpr int KC = L::CO, NC = L::CI, KK = L::K * L::K;
  static constexpr int NCT = NC / 16;                // ci tiles
  static constexpr int NKS = KK * (KC / 4);          // k-steps per tile: (tap, 4 source channels), tap-major
  static constexpr int NPX = L::HI * L::HI;          // output pixels per image
  static constexpr int SRC = KC * L::HO * L::HO;     // source floats per image
  static constexpr int PS = PL::PS, HP = PL::HP, IMG = KC * PS;
  static constexpr int CPS = NKS <= 100 ? 2 : 1;     // consumer wavefronts per SIMD: two when two weight sets fit beside a producer
  static constexpr int NCW = 4 * CPS, NTHR = 64 * (NCW + 4), NLT = NTHR - 64 * NCW;
  static constexpr int TSPLIT = NCW / NCT;           // consumers of one ci tile: they split a window's pixel tiles
  static constexpr int TPW = CPS == 2 ? 2 : 4;       // tiles per consumer per window
  static constexpr int WIN = 16 * TSPLIT * TPW;      // pixels per window
  static constexpr int PF = 2;                       // k-steps of operands in flight ahead of the MFMAs
  // fewest tiles with a k-loop instance of their own; below it a partial last window runs on aliased pixels.  One consumer per SIMD:
  // every window at TPW tiles -- a second 800-MFMA instance spilled weights under the 256-register cap, and a workgroup's last window
  // is the only one that can be partial
  static constexpr int NTMIN = CPS == 2 ? 1 : TPW;
  static constexpr int NBUF = (2 * WIN - 2) / NPX + 2;   // images two consecutive windows can touch
  static_assert(NCW % NCT == 0 && TSPLIT * NCT == NCW, "the consumers split the ci tiles evenly");
  static_assert(TPW * (PF + 1) <= 15, "LDS reads in flight within what lgkmcnt counts");
  static_assert(KC % 4 == 0 && SRC % 4 == 0, "float4 source");
  // the source rows hold whole float4 (one base address per float4), or the element -> plane offsets of a group of four planes
  // (HO * HO float4) repeat and fit one register table per producer thread
  static constexpr bool ROW4 = L::HO % 4 == 0;
  static_assert(ROW4 || L::HO * L::HO <= NLT, "producer offset table");
  // LDS byte offset of k-step s relative to the lane's base (the ds_read offset field holds 16 bits)
  static constexpr int koff(int s) { return (s / (KC / 4)) / L::K * HP + (s / (KC / 4)) % L::K + (s % (KC / 4)) * 4 * PS; }
  static_assert(4 * koff(NKS - 1) < 65536, "operand offsets fit the ds_read immediate");
  static constexpr size_t lds_bytes() { return sizeof(float) * (size_t)NBUF * IMG; }
};

// one window's tiles of one consumer: all NKS k-steps of NT pixel tiles against the wavefront's ci tile (weights in wr).
// The operands of step s + PF are requested, unconditionally, in front of the MFMAs of step s; sched_barrier keeps the order.
template <class E, int NT>
__device__ __forceinline__ void bdv2_tiles(const float* __restrict__ s_buf, const int (&base)[E::TPW], const float (&wr)[E::NKS],
                                           f32x4 (&acc)[E::TPW]) {
  float bf[E::PF + 1][NT];
  auto fetch = [&](auto sc) {
    constexpr int s = decltype(sc)::value;
#pragma unroll
    for (int t = 0; t < NT; ++t) bf[s % (E::PF + 1)][t] = s_buf[base[t] + E::koff(s)];
  };
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  static_for<E::PF>([&](auto sc) { fetch(sc); });
  static_for<E::NKS>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    if constexpr (s + E::PF < E::NKS) fetch(std::integral_constant<int, s + E::PF>{});
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[s], bf[s % (E::PF + 1)][t], acc[t], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  });
}

// the first nt (wave-uniform, 1..TPW) tiles of a window: one instance per tile count from NTMIN on
template <class E, int NT>
__device__ __forceinline__ void bdv2_window(int nt, const float* __restrict__ s_buf, const int (&base)[E::TPW], const float (&wr)[E::NKS],
                                            f32x4 (&acc)[E::TPW]) {
  if constexpr (NT > E::NTMIN) {
    if (nt < NT) { bdv2_window<E, NT - 1>(nt, s_buf, base, wr, acc); return; }
  }
  bdv2_tiles<E, NT>(s_buf, base, wr, acc);
}

// grid.x <= number of CUs (images blockIdx.x + j gridDim.x), block BdV2::NTHR, LDS BdV2::lds_bytes()
template <class L>
__global__ __launch_bounds__(BdV2<L>::NTHR) void k_conv_bwd_data_v2(const float* __restrict__ gy, const float* __restrict__ w,
                                                                    float* __restrict__ gx, int B) {
  using E = BdV2<L>;
  using PL = typename E::PL;
  constexpr int KC = E::KC, NC = E::NC, KK = E::KK, NPX = E::NPX, IMG = E::IMG, PS = E::PS, HP = E::HP, WIN = E::WIN, NKS = E::NKS;
  constexpr int HO = L::HO, P = L::P, NLT = E::NLT, NBUF = E::NBUF, TPW = E::TPW, TSPLIT = E::TSPLIT;
  float* s_buf = igemm_smem;                         // [NBUF][KC][PS] zero-padded planes, index (oy + P) * HP + ox + P
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nit = ((int)blockIdx.x < B) ? (B - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;   // images of this workgroup
  const int npx = nit * NPX, nwin = (npx + WIN - 1) / WIN;
  // last image a window reads (window i covers stream pixels [i WIN, i WIN + WIN) of the workgroup)
  auto last_img = [&](int i) { return min(nit - 1, (i * WIN + WIN - 1) / NPX); };

  // the padding (row and column 0 of every plane) is written here and never again
  for (int e = tid; e < NBUF * IMG / 4; e += E::NTHR) reinterpret_cast<float4*>(s_buf)[e] = float4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  if (wave >= E::NCW) {
    // producer: image j of the workgroup -> buffer j % NBUF.  All loads first (clamped index, no branch), then the stores.
    __builtin_amdgcn_s_setprio(3);
    const int lt = tid - 64 * E::NCW;
    constexpr int N4 = E::SRC / 4;
    // odd widths: the HO * HO float4 of a group of four planes go to the first HO * HO producer threads, each with the plane offsets
    // of its four elements in registers (group g adds 4 g planes)
    int otab[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * min(lt, HO * HO - 1) + k, pl = e / (HO * HO), q = e % (HO * HO);
      otab[k] = pl * PS + (q / HO + P) * HP + q % HO + P;
    }
    auto stage = [&](int j) __attribute__((always_inline)) {
      const float4* src = reinterpret_cast<const float4*>(gy) + (size_t)((int)blockIdx.x + j * (int)gridDim.x) * N4;
      float* buf = s_buf + (j % NBUF) * IMG;
      if constexpr (E::ROW4) {
        // a float4 is four columns of one source row (HO % 4 == 0), so one base address and four constant offsets
        constexpr int NLD = (N4 + NLT - 1) / NLT;
        float4 v[NLD];
#pragma unroll
        for (int i = 0; i < NLD; ++i) v[i] = src[min(lt + NLT * i, N4 - 1)];
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
          const int f = lt + NLT * i;
          const int pl = (4 * f) / (HO * HO), q = (4 * f) % (HO * HO), row = q / HO, col = q % HO;
          float* d = buf + pl * PS + (row + P) * HP + col + P;
          if (f < N4) { d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w; }
        }
      } else if (lt < HO * HO) {
        float4 v[KC / 4];
#pragma unroll
        for (int g = 0; g < KC / 4; ++g) v[g] = src[g * HO * HO + lt];
#pragma unroll
        for (int g = 0; g < KC / 4; ++g) {
          float* d = buf + 4 * g * PS;
          d[otab[0]] = v[g].x; d[otab[1]] = v[g].y; d[otab[2]] = v[g].z; d[otab[3]] = v[g].w;
        }
      }
    };
    // images [0, last_img(0)] before window 0; during window i those of window i + 1 not yet staged.  The oldest image window i reads
    // is newer than last_img(i + 1) - NBUF (NBUF covers the span of two windows), so those buffers are free.
    int staged = -1;
    if (nit > 0)
      for (; staged < last_img(0); ) stage(++staged);
    __syncthreads();
    for (int i = 0; i < nwin; ++i) {
      if (i + 1 < nwin)
        for (const int j1 = last_img(i + 1); staged < j1; ) stage(++staged);
      __syncthreads();                               // window i consumed, window i + 1's images staged
    }
    return;
  }

  // consumer: ci tile ct of tiles sm + TSPLIT t (t < TPW) of every window
  const int lr = lane & 15, lk = lane >> 4, ct = wave / TSPLIT, sm = wave % TSPLIT;
  float wr[NKS];                                     // A fragment of k-step s: w[ci = 16 ct + lr][co = 4 (s % (KC/4)) + lk][tap s / (KC/4)]
#pragma unroll
  for (int s = 0; s < NKS; ++s) wr[s] = w[((size_t)(16 * ct + lr) * KC + 4 * (s % (KC / 4)) + lk) * KK + s / (KC / 4)];
  __syncthreads();                                   // window 0's images staged
  for (int i = 0; i < nwin; ++i) {
    const int t0 = i * WIN + 16 * sm;                // stream pixel of tile 0's lane 0; tile t starts 16 TSPLIT t further
    int base[TPW], mm[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      mm[t] = t0 + 16 * TSPLIT * t + lr;
      const int m = min(mm[t], npx - 1);             // past the end: alias the last pixel (resident), masked at the store
      const int j = m / NPX, p = m - j * NPX;
      base[t] = (j % NBUF) * IMG + lk * PS + PL::template C<0>::pix_addr(p);
    }
    f32x4 acc[TPW];
    // wave-uniform: tiles of this window that hold pixels
    const int nt = t0 < npx ? min(TPW, (npx - t0 + 16 * TSPLIT - 1) / (16 * TSPLIT)) : 0;
    if (nt > 0) bdv2_window<E, TPW>(nt, s_buf, base, wr, acc);
    // lane: pixel mm[t], channels 16 ct + 4 lk + r
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      if (t < nt && mm[t] < npx) {
        const int j = mm[t] / NPX, p = mm[t] - j * NPX;
        float* o = gx + ((size_t)((int)blockIdx.x + j * (int)gridDim.x) * NC + 16 * ct + 4 * lk) * NPX + p;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(size_t)r * NPX] = acc[t][r];
      }
    }
    __syncthreads();                                 // window i consumed, window i + 1's images staged
  }
}

}  // namespace gp
