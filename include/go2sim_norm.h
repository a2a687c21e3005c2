/* go2sim_norm.h -- C ABI of the empirical observation normaliser: `rsl_rl.modules.EmpiricalNormalization` (rsl-rl-lib==2.2.4) as the runner puts
 * it in front of the policy.  rsl_rl is a third-party package that is not part of the reference tree; the law is stated here.
 *
 * Conventions follow go2sim_train.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call below synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is numpy float64
 * (tests/norm_ref.py).
 *
 * A handle holds on the device mean[d], var[d], std[d] as float32 (the storage of rsl_rl's buffers: a state dict round-trips without loss), count
 * as int64, and the two constants eps and until.  Initial state: mean 0, var 1, std 1, count 0.
 *
 * The law.  With a batch of n rows whose column moments are mean_b and the BIASED variance var_b = M2_b / n:
 *   count' = count + n;  rate = n / count'
 *   mean'  = mean + rate (mean_b - mean)
 *   var'   = var + rate (var_b - var + (mean_b - mean) (mean_b - mean'))
 *   std'   = sqrt(var')
 * applied when the caller asks for an update and count < until (tested before the update: the batch that crosses `until` is counted whole); then
 *   y = (x - mean) / (std + eps)                                   float32 operations, a correctly rounded division
 * with the statistics as they are after the update.
 *
 * Numerics.  The batch moments are float64 and two-pass: per chunk of GO2SIM_NORM_ROW_CHUNK rows the column mean, then the squares centred on it; over
 * the chunks, in chunk order, the batch mean as the weighted mean of the chunk means, then M2 = sum_i (M2_i + n_i (mean_i - mean)^2) -- the same two
 * passes one level up.  Records of ranks are folded in record order with Chan's pairwise formula
 *   n = n_a + n_b;  delta = mean_b - mean_a;  mean = mean_a + delta (n_b / n);  M2 = M2_a + M2_b + delta^2 (n_a n_b / n)
 * In none of these is anything of the size of mean^2.  The update runs in float64 from the float32 state; mean', var' and std' =
 * sqrt(var' in float64) are each rounded to float32 once.  A var' that rounding took below zero is stored as zero (a NaN stays a NaN).  The result is
 * a function of (state, data, n_rows) alone: fixed chunks, fixed fold order, no floating-point atomics -- equal calls on equal states give equal
 * bits on any stream and for any alignment of x.  Columns are independent: a NaN in column j reaches column j's statistics only.
 * Bounds: tests/norm_ref.py derives them (state: one float32 rounding of a float64 result with the error of an n-term float64 sum; output: what
 * follows from it through the formula above).
 *
 * Launches (csrc/go2sim_norm.hip), both normalisers of a call in each of them (blockIdx.y):
 *   k_norm_moments   one workgroup of 1024 lanes per chunk: lanes run across the columns of consecutive rows (a flat, coalesced read of the row-major
 *                    chunk with dword loads, so a row of 49 or 45 floats and an x that starts 4 bytes off a 16-byte boundary need nothing special),
 *                    the lanes of a column are added in lane order through LDS.  Workgroup 0 also copies the state aside.
 *   k_norm_apply     32 rows per workgroup: every workgroup folds the chunk moments (or the ranks' records) per column, applies the law to the
 *                    copy of the state and normalises its rows; workgroup 0 stores the new state.  Without an update it is the only launch.
 *   k_norm_record    (go2sim_norm_moments) folds the chunk moments into the record;  k_norm_snapshot (go2sim_norm_merge_step) copies the state aside.
 */
#ifndef GO2SIM_NORM_H
#define GO2SIM_NORM_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_NORM_ROW_CHUNK 256

typedef struct go2sim_norm go2sim_norm_t;

/* n_features >= 1; eps >= 0 (rsl_rl's default 1e-2; kept as float32); until <= 0: the statistics never stop (rsl_rl's None), the runner uses 1e8.
 * Waits for the device. */
int go2sim_norm_create(int device, int n_features, double eps, double until, go2sim_norm_t** out);
int go2sim_norm_destroy(go2sim_norm_t* h);
/* mean, var, std: float32 [n_features] in host memory, count: int64; bit-exact both ways.  Both wait for the stream. */
int go2sim_norm_get_state(go2sim_norm_t* h, float* mean, float* var, float* std, int64_t* count, void* stream);
int go2sim_norm_set_state(go2sim_norm_t* h, const float* mean, const float* var, const float* std, int64_t count, void* stream);

/* The per-env-step call for one or two normalisers (b and its arrays may all be NULL): x [n_rows][d] and y [n_rows][d] row-major device arrays.
 * update != 0 and count < until: fold the batch into the statistics (the law above); then y = (x - mean) / (std + eps).  Two launches with an
 * update, one without, none for n_rows == 0 (success, state unchanged).  GO2SIM_E_BADARG for n_rows < 0, a NULL x or y, or y == x (the state is
 * unchanged then); x and y that overlap in part are the caller's error.  The first call with more rows than any before it grows the handle's
 * workspace (an allocation; the old one is kept until go2sim_norm_destroy, nothing waits). */
int go2sim_norm_step(go2sim_norm_t* a, const float* x_a, float* y_a, go2sim_norm_t* b, const float* x_b, float* y_b, int n_rows, int update,
                     void* stream);

/* The same step for a batch sharded over ranks.  A record is float64 [len]: per normaliser n, mean_b[d], M2_b[d] (a first, then b). */
int go2sim_norm_record_len(go2sim_norm_t* a, go2sim_norm_t* b, int* len);
/* this rank's record from its rows (n_rows == 0: n = 0 and zeros); record_dev is device memory; two launches, the state is not touched */
int go2sim_norm_moments(go2sim_norm_t* a, const float* x_a, go2sim_norm_t* b, const float* x_b, int n_rows, double* record_dev, void* stream);
/* records_dev [n_records][len] (device memory, rank order): folds the records in record order with Chan's formula (records with n = 0 are passed
 * over), feeds the union's (n, mean, M2 / n) into the law under the same condition as go2sim_norm_step, and normalises this rank's n_rows rows
 * (n_rows == 0 is allowed: the statistics still move).  One record made by go2sim_norm_moments from the same rows gives the bits of
 * go2sim_norm_step.  Two launches. */
int go2sim_norm_merge_step(go2sim_norm_t* a, const float* x_a, float* y_a, go2sim_norm_t* b, const float* x_b, float* y_b, int n_rows,
                           const double* records_dev, int n_records, int update, void* stream);

#ifdef __cplusplus
}
#endif
#endif
