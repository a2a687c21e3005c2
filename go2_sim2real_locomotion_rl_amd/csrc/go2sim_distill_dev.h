// go2sim_distill_dev.h -- private to csrc/: the kernels the two distillation updates share, next to go2sim_train_dev.h.  The MLP student's update
// (go2sim_distill.hip) and the recurrent student's (go2sim_rdistill.hip) include it; both run the behaviour loss on rows of means, keep the float64 sum of
// a window that is walked in pieces, and report the same six statistics.  Not part of the C ABI.
//   k_distill_head        one row per lane: residual, rho into a float64 per-workgroup partial, rho' / (N A) into dZ [rows][Apad] with zero padding
//   k_distill_finalize    the head's partials in workgroup order, weighted once, onto the running loss sum
//   k_distill_accumulate  k_reduce_partials across pieces of a window: the float64 sum is kept between pieces and rounded after the last one
//   k_distill_reset / k_distill_stats   the running sum and the statistics block
#ifndef GO2SIM_DISTILL_DEV_H
#define GO2SIM_DISTILL_DEV_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "go2sim_train_dev.h"
#include "../../include/go2sim_distill.h"

namespace {

// the handle's scalar block has the layout k_adam knows (S_LR, S_NORM); the running sum of the pairs' losses takes a slot the PPO sums use there
constexpr int D_SUM_LOSS = S_SUM_VL;

struct DistillHeadArgs {
  const float* mu;             // [n][A]: this sub-batch's forward
  const float* teacher;        // [.][A], rows through idx
  const int32_t* idx;
  float* dz;                   // [n][Apad]
  double* part;                // [workgroups]
  int n, A, Apad, huber;
  double w;                    // 1 / (N A)
};

// One row per lane.  The loop runs over the Apad columns of dZ whatever the data; padded columns and nothing else get an exact zero.
__global__ __launch_bounds__(WGT) void k_distill_head(DistillHeadArgs h) {
  __shared__ double s_red[WGT];
  const int r = blockIdx.x * WGT + threadIdx.x;
  double sum = 0.0;
  if (r < h.n) {
    const size_t src = (size_t)h.idx[r];
    for (int a = 0; a < h.Apad; ++a) {
      float g = 0.0f;
      if (a < h.A) {
        const double d = (double)h.mu[(size_t)r * h.A + a] - (double)h.teacher[src * h.A + a];
        double rho, drho;
        if (h.huber) {
          const double ad = fabs(d);
          rho = ad <= 1.0 ? 0.5 * d * d : ad - 0.5;
          drho = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
        } else {
          rho = d * d;
          drho = 2.0 * d;
        }
        sum += rho;
        g = (float)(drho * h.w);
      }
      h.dz[(size_t)r * h.Apad + a] = g;
    }
  }
  const double t = wg_sum(s_red, sum);
  if (threadIdx.x == 0) h.part[blockIdx.x] = t;
}

// one thread: the window's (or the tail's) head partials in workgroup order, weighted once, onto the running sum
__global__ void k_distill_finalize(const double* __restrict__ part, int n_wg, double w, double* __restrict__ scal) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < n_wg; ++i) s += part[i];
  scal[D_SUM_LOSS] += s * w;
}

// k_reduce_partials across sub-batches: entry i continues the float64 sum of the earlier sub-batches' chunks (first: from zero) and is rounded into the
// gradient vector after the last one
__global__ __launch_bounds__(WGT) void k_distill_accumulate(const float* __restrict__ partial, int n_chunks, size_t slab, double* __restrict__ acc, int first, int last,
                                                            float* __restrict__ grads) {
  const size_t i = (size_t)blockIdx.x * WGT + threadIdx.x;
  if (i >= slab) return;
  double s = first ? 0.0 : acc[i];
  for (int c = 0; c < n_chunks; ++c) s += (double)partial[(size_t)c * slab + i];
  if (last) grads[i] = (float)s;
  else acc[i] = s;
}

__global__ void k_distill_reset(double* scal) { if (blockIdx.x == 0 && threadIdx.x == 0) scal[D_SUM_LOSS] = 0.0; }
__global__ void k_distill_stats(const double* __restrict__ scal, double step, double pairs, double windows, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  out[GO2SIM_DISTILL_ST_LOSS] = scal[D_SUM_LOSS] / (pairs > 0.0 ? pairs : 1.0);
  out[GO2SIM_DISTILL_ST_LR] = scal[S_LR]; out[GO2SIM_DISTILL_ST_GRAD_NORM] = scal[S_NORM];
  out[GO2SIM_DISTILL_ST_STEP] = step; out[GO2SIM_DISTILL_ST_PAIRS] = pairs; out[GO2SIM_DISTILL_ST_WINDOWS] = windows;
}

}  // namespace
#endif
