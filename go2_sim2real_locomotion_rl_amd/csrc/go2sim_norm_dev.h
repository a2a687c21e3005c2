// go2sim_norm_dev.h -- private to csrc/: the float64 moment code of the empirical normaliser (include/go2sim_norm.h states the law and the fold order),
// shared by the observation normaliser (go2sim_norm.hip) and the reward normaliser of random network distillation (go2sim_rnd.hip).  Not part of the C ABI.
//   Mom, mom_merge    the moments (n, mean, M2) of a set of rows, and Chan's merge of two sets
//   fold_chunks       one column's moments over the chunks of a call, in chunk order, from the per-chunk (mean, centred squares)
//   norm_law          count' / mean' / var' of the law from the float32 state and a batch's moments, in float64
#ifndef GO2SIM_NORM_DEV_H
#define GO2SIM_NORM_DEV_H
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/go2sim_norm.h"

namespace {

constexpr int CH = GO2SIM_NORM_ROW_CHUNK;   // rows of one moments workgroup: the unit of the fixed fold order

struct Mom { double n, mean, M2; };

// Chan et al.: the moments of the union from those of two sets
__device__ __forceinline__ void mom_merge(Mom& a, double nb, double mb, double M2b) {
  const double n = a.n + nb, delta = mb - a.mean;
  a.mean = a.mean + delta * (nb / n);
  a.M2 = a.M2 + M2b + delta * delta * (a.n * nb / n);
  a.n = n;
}

__device__ __forceinline__ int chunk_rows(int i, int n_rows) { return min(CH, n_rows - i * CH); }

// column c's moments over all chunks of the call, in chunk order: the batch mean as the weighted mean of the chunk means, then the chunks' centred squares
// moved to it, M2 = sum_i (M2_i + n_i (mean_i - mean)^2) -- two passes over the chunk moments, one division per column, nothing of the size of mean^2
__device__ __forceinline__ Mom fold_chunks(const double* __restrict__ part, int d, int c, int n_rows) {
  const int nch = (n_rows + CH - 1) / CH;
  if (nch == 1) return Mom{(double)n_rows, part[c], part[(size_t)d + c]};
  // FB chunks' loads are issued together, the sums stay in chunk order: the 16 chunks of 4096 rows cost two round trips to memory, not sixteen
  constexpr int FB = 8;
  double s = 0.0;
  for (int i0 = 0; i0 < nch; i0 += FB) {
    double m[FB];
#pragma unroll
    for (int k = 0; k < FB; ++k) m[k] = i0 + k < nch ? part[(size_t)(2 * (i0 + k)) * d + c] : 0.0;
#pragma unroll
    for (int k = 0; k < FB; ++k)
      if (i0 + k < nch) s += (double)chunk_rows(i0 + k, n_rows) * m[k];
  }
  const double mean = s / (double)n_rows;
  double q = 0.0;
  for (int i0 = 0; i0 < nch; i0 += FB) {
    double m[FB], m2[FB];
#pragma unroll
    for (int k = 0; k < FB; ++k) {
      m[k] = i0 + k < nch ? part[(size_t)(2 * (i0 + k)) * d + c] : 0.0;
      m2[k] = i0 + k < nch ? part[(size_t)(2 * (i0 + k) + 1) * d + c] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < FB; ++k)
      if (i0 + k < nch) { const double e = m[k] - mean; q += m2[k] + (double)chunk_rows(i0 + k, n_rows) * (e * e); }
  }
  return Mom{(double)n_rows, mean, q};
}

// the law of include/go2sim_norm.h for one column: state (m, v, cnt) and the batch's moments b (b.n > 0) -> mean' and var' (clamped at zero) in float64
__device__ __forceinline__ void norm_law(double m, double v, long long cnt, const Mom& b, double& m1, double& v1) {
  const double cnt1 = (double)cnt + b.n, rate = b.n / cnt1;
  const double dm = b.mean - m;
  m1 = m + rate * dm;
  v1 = v + rate * (b.M2 / b.n - v + dm * (b.mean - m1));
  if (v1 < 0.0) v1 = 0.0;
}

}  // namespace
#endif
