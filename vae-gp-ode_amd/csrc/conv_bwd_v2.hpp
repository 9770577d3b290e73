// conv_bwd_v2.hpp -- d/d input of decnn.7 (ConvTranspose2d 32 -> 16, 13 -> 28, vae.py:113-121) on the fp32 matrix cores, second
// engine: PRODUCER / CONSUMER wavefronts with the weights resident in the consumers' registers.
//
//   gx[ci][iy][ix] = sum_{co,ky,kx} gy[co][S iy - P + ky][S ix - P + kx] w[ci][co][ky][kx]        (an ordinary strided convolution)
//
// Same GEMM view, plane layout and geometry as the first engine (conv_mfma.hpp, BwdDataPolicy): D[ci][pixel] = sum_k W[ci][k] X[k][pixel],
// k = (tap, 4 source channels) per v_mfma_f32_16x16x4_f32, A := weights, B := pixels, so a lane ends up with one pixel and four
// channels of a tile.  What changed is where the operands live and who does what:
//
//   * Weights in registers.  A wavefront owns one 16-channel ci tile, and the A fragments of all 100 k-steps of that tile (16 ci x 16 co
//     x 25 taps / 64 lanes = 100 VGPRs) are loaded once per launch.  The k-loop then reads ONE LDS operand per MFMA (the first engine:
//     two), at a per-lane base computed once per tile plus a compile-time offset per k-step -- a tap is a constant shift in the
//     zero-padded plane, a group of four source channels a constant number of planes -- that fits the ds_read offset field.
//     (32x32x2 would halve the operand reads per flop as well, but its A fragments for 32 ci are 200 VGPRs: the weights would have to
//     stay in LDS, 51 KB, and the third plane buffer below would not fit.)
//   * Three single-image plane buffers (3 x 53.8 KB; no weight slabs).  The pixels of a workgroup's images form ONE stream that is
//     cut into windows of 128 pixels = 8 tiles of 16, regardless of image boundaries: a tile may take its first pixels from one image
//     and the rest from the next.  169 pixels per image quantised per image to 11 tiles of 16 waste 4 % (to 6 tiles of 32: 12 %);
//     here only the last window of a workgroup is partial.  A window touches at most two images, so while it is multiplied the third
//     buffer takes the image the next window needs.
//   * Wavefronts 0..7 consume: wavefront w takes ci tile w >> 2 of tiles (w & 3) and (w & 3) + 4 of every window, so the two
//     consumers of a SIMD (w, w + 4) split the same pixel tiles by channels and every SIMD issues the same MFMAs per window.
//     Wavefronts 8..11 (one per SIMD, raised priority as in conv_wgrad_v2.hpp) stream the next image from HBM into the free buffer.
//     ONE workgroup barrier per window.
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
  static constexpr int NBUF = 3, NCW = 8, NTHR = 768, NLT = NTHR - 64 * NCW;
  static constexpr int TPW = 2;                      // tiles per consumer per window
  static constexpr int WIN = 16 * 4 * TPW;           // pixels per window: TPW tiles per SIMD
  static constexpr int PF = 2;                       // k-steps of operands in flight ahead of the MFMAs
  static_assert(NCT * 4 == NCW, "the two consumers of a SIMD split the output channels");
  static_assert(KC % 4 == 0 && L::HO % 4 == 0 && SRC % 4 == 0, "float4 rows of the source");
  static_assert(WIN <= NPX, "a window touches at most two images");
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

// grid.x <= number of CUs (images blockIdx.x + j gridDim.x), block 768, LDS BdV2::lds_bytes()
template <class L>
__global__ __launch_bounds__(768) void k_conv_bwd_data_v2(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ gx,
                                                          int B) {
  using E = BdV2<L>;
  using PL = typename E::PL;
  constexpr int KC = E::KC, NC = E::NC, KK = E::KK, NPX = E::NPX, IMG = E::IMG, PS = E::PS, HP = E::HP, WIN = E::WIN, NKS = E::NKS;
  constexpr int HO = L::HO, P = L::P, NLT = E::NLT;
  float* s_buf = igemm_smem;                         // [NBUF][KC][PS] zero-padded planes, index (oy + P) * HP + ox + P
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nit = ((int)blockIdx.x < B) ? (B - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;   // images of this workgroup
  const int npx = nit * NPX, nwin = (npx + WIN - 1) / WIN;
  // last image a window reads (window i covers stream pixels [i WIN, i WIN + WIN) of the workgroup)
  auto last_img = [&](int i) { return min(nit - 1, (i * WIN + WIN - 1) / NPX); };

  // the padding (row and column 0 of every plane) is written here and never again
  for (int e = tid; e < E::NBUF * IMG / 4; e += E::NTHR) reinterpret_cast<float4*>(s_buf)[e] = float4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  if (wave >= E::NCW) {
    // producer: image j of the workgroup -> buffer j % 3.  All loads first (clamped index, no branch), then the stores: a float4 is four
    // columns of one source row (HO % 4 == 0), so one base address and four constant offsets.
    __builtin_amdgcn_s_setprio(3);
    const int lt = tid - 64 * E::NCW;
    constexpr int N4 = E::SRC / 4, NLD = (N4 + NLT - 1) / NLT;
    auto stage = [&](int j) __attribute__((always_inline)) {
      const float4* src = reinterpret_cast<const float4*>(gy) + (size_t)((int)blockIdx.x + j * (int)gridDim.x) * N4;
      float* buf = s_buf + (j % E::NBUF) * IMG;
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
    };
    if (nit > 0) stage(0);                           // window 0 reads image 0 only (WIN <= NPX)
    __syncthreads();
    for (int i = 0; i < nwin; ++i) {
      // window i reads images up to last_img(i) >= (last_img(i) + 1) - 2: the buffer of image last_img(i) + 1 is free
      if (i + 1 < nwin && last_img(i + 1) > last_img(i)) stage(last_img(i + 1));
      __syncthreads();                               // window i consumed, window i + 1's images staged
    }
    return;
  }

  // consumer
  const int lr = lane & 15, lk = lane >> 4, ct = wave >> 2, sm = wave & 3;
  float wr[NKS];                                     // A fragment of k-step s: w[ci = 16 ct + lr][co = 4 (s % (KC/4)) + lk][tap s / (KC/4)]
#pragma unroll
  for (int s = 0; s < NKS; ++s) wr[s] = w[((size_t)(16 * ct + lr) * KC + 4 * (s % (KC / 4)) + lk) * KK + s / (KC / 4)];
  __syncthreads();                                   // image 0 staged
  for (int i = 0; i < nwin; ++i) {
    const int t0 = i * WIN + 16 * sm;                // stream pixel of tile 0's lane 0; tile t starts 64 t further
    int base[E::TPW], mm[E::TPW];
#pragma unroll
    for (int t = 0; t < E::TPW; ++t) {
      mm[t] = t0 + 64 * t + lr;
      const int m = min(mm[t], npx - 1);             // past the end: alias the last pixel (resident), masked at the store
      const int j = m / NPX, p = m - j * NPX;
      base[t] = (j % E::NBUF) * IMG + lk * PS + PL::template C<0>::pix_addr(p);
    }
    f32x4 acc[E::TPW];
    int nt = 0;                                      // wave-uniform: tiles of this window that hold pixels
    if (t0 + 64 < npx) { bdv2_tiles<E, 2>(s_buf, base, wr, acc); nt = 2; }
    else if (t0 < npx) { bdv2_tiles<E, 1>(s_buf, base, wr, acc); nt = 1; }
    // lane: pixel mm[t], channels 16 ct + 4 lk + r
#pragma unroll
    for (int t = 0; t < E::TPW; ++t) {
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
