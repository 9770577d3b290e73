// vae_optim.hip -- the optimiser step over all parameter tensors in one launch, and the gradient gather in front of it.
#include <hip/hip_runtime.h>
#include "gp_launch.hpp"

// ---------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam defaults as used at main.py:194: betas (0.9, 0.999), eps 1e-8, no weight decay),
// all parameter tensors in ONE launch: a table of (param, grad, exp_avg, exp_avg_sq) pointers with prefix
// offsets; each thread finds its tensor by binary search.
// ---------------------------------------------------------------------------------------------
namespace gp {
__global__ void k_adam_multi(float* const* __restrict__ params, const float* const* __restrict__ grads,
                             float* const* __restrict__ m1, float* const* __restrict__ m2, const long long* __restrict__ offs,
                             int ntensors, long long total, float lr, float beta1, float beta2, float eps, float bc1, float bc2,
                             int* __restrict__ step_dev) {
  int step = 0;
  if (step_dev) {                                    // step counter kept on the device (captured graphs replay with a live count)
    step = step_dev[0] + 1;                          // this update's number; published below by the last workgroup to finish
    const float t = (float)step;
    bc1 = 1.f - powf(beta1, t);
    bc2 = 1.f - powf(beta2, t);
  }
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (offs[mid] <= e) lo = mid; else hi = mid - 1; }
    const long long i = e - offs[lo];
    const float g = grads[lo][i];
    const float a = beta1 * m1[lo][i] + (1.f - beta1) * g;
    const float b = beta2 * m2[lo][i] + (1.f - beta2) * g * g;
    m1[lo][i] = a;
    m2[lo][i] = b;
    // torch: denom = sqrt(v)/sqrt(bc2) + eps ; p -= lr/bc1 * m / denom
    params[lo][i] -= (lr / bc1) * a / (sqrtf(b) / sqrtf(bc2) + eps);
  }
  if (step_dev) {
    // every workgroup has read step_dev[0] before it takes a ticket, so the last one may advance it (no separate launch for the
    // counter: one graph node less on the tail of every step)
    // (no memory fence: nothing but the counter is handed between workgroups, and the ticket is a device-scope atomic; a
    // __threadfence() here writes the L2 back -- measured 15 us on this 22 us kernel)
    __syncthreads();
    if (threadIdx.x == 0) {
      if (atomicAdd(&step_dev[1], 1) == (int)gridDim.x - 1) {
        step_dev[1] = 0;
        step_dev[0] = step;
      }
    }
  }
}

// flat[offs[t] + i] = grads[t][i] for every tensor of the table: the data-parallel gradient bucket filled in ONE launch
// from the tensors autograd handed over (instead of one accumulate kernel per parameter into persistent views)
__global__ void k_gather_multi(const float* const* __restrict__ grads, const long long* __restrict__ offs, int ntensors,
                               long long total, float* __restrict__ flat) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = ntensors - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (offs[mid] <= e) lo = mid; else hi = mid - 1; }
    flat[e] = grads[lo][e - offs[lo]];
  }
}

int gather_multi(const float* const* grads, const long long* offs, int ntensors, long long total, float* flat, hipStream_t st) {
  hipLaunchKernelGGL(k_gather_multi, ew_grid((size_t)total), 256, 0, st, grads, offs, ntensors, total, flat);
  return check_launch("gather_multi");
}

// step_dev != nullptr: int[2] {step count, 0}: the count is advanced by the kernel and used as this update's number (host `step` ignored)
int adam_multi(float* const* params, const float* const* grads, float* const* m1, float* const* m2, const long long* offs,
               int ntensors, long long total, float lr, float beta1, float beta2, float eps, int step, int* step_dev, hipStream_t st) {
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  // with the device-side count every workgroup takes a ticket on ONE address (the last one publishes the count), so the grid is
  // capped; an iteration of the grid-stride loop is a chain of dependent loads (binary search of the offsets, the tensor's pointers,
  // its data: ~1.5 us), so the cap is high: 2048 workgroups against 128 gave configs[1] 2.62 -> 2.59 ms, configs[2] / [3] -8 us,
  // configs[0] unchanged (profiles/r03d_ab_switches.txt)
  constexpr unsigned cap = 2048;
  unsigned grid = ew_grid((size_t)total);
  if (step_dev && grid > cap) grid = cap;
  hipLaunchKernelGGL(k_adam_multi, grid, 256, 0, st, params, grads, m1, m2, offs, ntensors, total, lr, beta1, beta2, eps, bc1, bc2,
                     step_dev);
  return check_launch("adam_multi");
}
}  // namespace gp
