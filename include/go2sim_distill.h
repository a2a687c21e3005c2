/* go2sim_distill.h -- C ABI of teacher-student distillation: the collection step that runs student and teacher side by side and the behaviour-cloning
 * update of the student.  It restates `rsl_rl.algorithms.Distillation` + `rsl_rl.modules.StudentTeacher` (rsl_rl 2.3 on) on top of the fused MLP of
 * include/go2sim_policy.h and the backward kernels of the PPO update (include/go2sim_train.h; csrc/go2sim_train_dev.h holds what the two share).
 *
 * Conventions follow go2sim_train.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given stream,
 * no call synchronises with the host unless it says so.  There is no CPU twin: the checker is torch float64 autograd (tests/distill_ref.py).
 *
 * The law.
 *   Modules: student = MLP(num_student_obs -> student_hidden_dims -> A), teacher = MLP(num_teacher_obs -> teacher_hidden_dims -> A), both ELU, depths
 *   and widths independent within GO2SIM_MLP_MAX_LAYERS / _WIDTH; std[A] = init_noise_std.
 *   Collection, per env step: mean = student(obs); actions = mean + std n with n from the Philox stream of go2sim_policy_act (same key, purpose 11,
 *   same counter layout); teacher_actions = teacher(teacher_obs).  The env steps on the student's actions.  Stored per step: obs [T][N][Ds],
 *   teacher_actions [T][N][A], dones.
 *   Update: cnt = 0; for each epoch e < E and each step t < T: cnt += 1 and the pair (e, t) joins the open window; when cnt % G == 0
 *   (G = gradient_length) the window closes: gradient of the window's loss, optional clip, one Adam step, a new window opens.  Windows run across
 *   epoch boundaries; when G > T a window may hold the same step twice; pairs left in an open window at the end are dropped (no gradient, not carried
 *   into the next update).
 *   Per pair  l_t = mean over N envs and A actions of rho(student(obs_t) - teacher_actions_t):
 *     mse:   rho(d) = d^2;                                 d loss / d mean[row][a] = 2 d / (N A)
 *     huber: rho(d) = d^2 / 2 for |d| <= 1, else |d| - 1/2;  d loss / d mean[row][a] = clamp(d, -1, 1) / (N A)
 *   A window's loss is the sum of its l_t; parameters are constant inside a window.
 *   Reported: mean_behavior_loss = sum of l_t over all E T pairs / (E T); the dropped tail is included (forward and head run for it, no backward).
 *   std gets no gradient and is outside the optimizer.
 *   Clip, if max_grad_norm is given: grads *= min(1, max_grad_norm / (||grads|| + 1e-6)) over the student's parameters.
 *   Adam(lr, 0.9, 0.999, 1e-8), bias corrections in float64 from the step count.  The learning rate is fixed.
 *
 * Numerics follow go2sim_train.h: fp32 fma chains on v_mfma_f32_16x16x4_f32, float64 for every scalar and every sum over chunks or workgroups, no
 * floating-point atomics, every sum in a fixed order (equal inputs give equal bits), padded entries exact zeros.  Against torch float64 autograd, per
 * parameter tensor,  max|g - g64| <= C_GRAD max(max|g32 - g64|, 2^-24 max|g64|)  and after whole updates  max|p - p64| <= C_UPD max|p32 - p64|, with
 * the constants of go2sim_train.h (C_GRAD = 16, C_UPD = 8); the means are held to the policy step's bound (C_MLP = 7, include/go2sim_policy.h).
 * Worst measured over tests/test_distill_gpu.py on the MI355X: 5.00 against C_GRAD (the small student's last weight, a window of 3 steps x 37 envs, huber), 2.13
 * against C_UPD ((T, E, G) = (3, 1, 3) at 17 envs, the first weight; the other update cases sit at 1.00: one or two Adam steps of size lr land on the float32
 * yardstick's own values), 1.68 against C_MLP; the loss statistic agrees with a float64 evaluation on the library's own means to 3.5e-16 relative.
 *
 * Workspaces: a window at the training shape is G N = 15 x 4096 = 61 440 rows = 120 chunks of GO2SIM_PPO_ROW_CHUNK, more than any PPO mini-batch.
 * The handle WALKS THE WINDOW IN SUB-BATCHES of sub_rows rows (default GO2SIM_DISTILL_SUB_ROWS = 8192 = 16 chunks; a multiple of the chunk): forward,
 * head and backward of one sub-batch reuse one set of row workspaces and 16 chunk slabs, then the slabs are added, in chunk order, onto a float64
 * accumulator of the padded gradient vector that is rounded once after the last sub-batch.  That is the sum over all of the window's chunks in chunk
 * order, started from zero: the bits do not depend on sub_rows.  The head's per-workgroup partials of the whole window are kept (one float64 per 256
 * rows) and added in workgroup order after the last sub-batch.  Memory at the training shape (student 49 -> 256 -> 256 -> 256 -> 12, padded vector
 * 152 336 floats): activations and dZ of 8192 rows 42 MB, 16 slabs 9.7 MB, accumulator + gradients + Adam 3 MB, the row-index list of one update
 * (E T N int32) 0.4 MB per epoch.
 */
#ifndef GO2SIM_DISTILL_H
#define GO2SIM_DISTILL_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim_policy.h"
#include "go2sim_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_DISTILL_SUB_ROWS 8192
#define GO2SIM_DISTILL_N_STATS 6

typedef struct go2sim_distill go2sim_distill_t;

enum go2sim_distill_loss { GO2SIM_DISTILL_MSE = 0, GO2SIM_DISTILL_HUBER };
enum go2sim_distill_vec { GO2SIM_DISTILL_PARAMS = 0, GO2SIM_DISTILL_GRADS, GO2SIM_DISTILL_ADAM_M, GO2SIM_DISTILL_ADAM_V };
/* go2sim_distill_stats writes GO2SIM_DISTILL_N_STATS float64: mean behaviour loss over the pairs since the last reset, learning rate, gradient norm
 * of the last apply, optimizer steps, pairs counted since the last reset, windows applied since the last reset */
enum go2sim_distill_stat { GO2SIM_DISTILL_ST_LOSS = 0, GO2SIM_DISTILL_ST_LR, GO2SIM_DISTILL_ST_GRAD_NORM, GO2SIM_DISTILL_ST_STEP, GO2SIM_DISTILL_ST_PAIRS,
                           GO2SIM_DISTILL_ST_WINDOWS };

typedef struct go2sim_distill_cfg {
  double learning_rate;
  double max_grad_norm;       /* <= 0: no clip */
  double beta1, beta2, eps;   /* Adam; 0.9, 0.999, 1e-8 */
  int loss_type;              /* enum go2sim_distill_loss */
  int sub_rows;               /* rows of a sub-batch; 0: GO2SIM_DISTILL_SUB_ROWS; otherwise a positive multiple of GO2SIM_PPO_ROW_CHUNK */
} go2sim_distill_cfg_t;

/* Student and teacher forward in ONE launch (two networks side by side, as go2sim_policy_act runs actor and critic), then the sampling kernel of
 * go2sim_policy_act on the student's mean.  Writes actions, mean and teacher_actions, each [n_rows][A]; all three are required.  actions and mean equal
 * go2sim_policy_act(student, NULL, ...) bit for bit at the same seed and step, teacher_actions equals go2sim_mlp_forward(teacher, ...) bit for bit.
 * The two networks must end in the same width and live on the same device. */
int go2sim_distill_act(go2sim_mlp_t* student, go2sim_mlp_t* teacher, const float* obs, const float* teacher_obs, const float* std_dev, int n_rows, uint64_t seed,
                       uint32_t step, int deterministic, float* actions, float* mean, float* teacher_actions, void* stream);

/* The trainer handle over the student's go2sim_mlp_t: it owns the workspaces, the gradients, Adam's m and v, the step count and the learning rate; the
 * optimizer writes the weight arrays go2sim_distill_act reads.  n_actions must equal the student's last width; max_window_rows is the largest window
 * (gradient_length x envs) a call may bring. */
int go2sim_distill_create(go2sim_mlp_t* student, int n_actions, const go2sim_distill_cfg_t* cfg, int max_window_rows, go2sim_distill_t** out);
int go2sim_distill_destroy(go2sim_distill_t* h);

/* One window: rows idx[0 .. n_rows) of obs [.][Ds] and teacher_actions [.][A] (int32 device indices; a row may appear more than once), n_rows a
 * multiple of n_envs, every row weighted 1 / (n_envs A).  Leaves the gradient on the device and adds the window's n_rows / n_envs pairs to the running
 * loss sum.  go2sim_distill_loss_only: the forward and the head alone (the dropped tail): the running loss sum moves, the gradient does not. */
int go2sim_distill_window_grad(go2sim_distill_t* h, const float* obs, const float* teacher_actions, const int32_t* idx_dev, int n_rows, int n_envs, void* stream);
int go2sim_distill_loss_only(go2sim_distill_t* h, const float* obs, const float* teacher_actions, const int32_t* idx_dev, int n_rows, int n_envs, void* stream);
/* Optional global-norm clip and one Adam step on the gradient the handle holds, written to the student's weights. */
int go2sim_distill_apply(go2sim_distill_t* h, void* stream);
/* The whole update over obs [T][N][Ds] and teacher_actions [T][N][A]: resets the running sums, then every window of (T, N, E, G) as above followed by
 * go2sim_distill_apply, then the loss-only pass over the dropped tail.  No host synchronisation; the windows' row-index list is built on the device by
 * one launch the first time a shape (T, N, E) is seen and kept in the handle.  gradient_length x n_envs must not exceed max_window_rows. */
int go2sim_distill_update(go2sim_distill_t* h, const float* obs, const float* teacher_actions, int n_steps, int n_envs, int n_epochs, int gradient_length,
                          void* stream);

/* One of the handle's vectors as a flat device vector in unpadded state-dict order: student W0, b0, W1, b1, ...  (std is not part of it). */
int go2sim_distill_n_params(go2sim_distill_t* h, size_t* out);
int go2sim_distill_export(go2sim_distill_t* h, int which, float* flat_dev, void* stream);
int go2sim_distill_import(go2sim_distill_t* h, int which, const float* flat_dev, void* stream);
/* Test access to a padded buffer as the kernels hold it (PARAMS, GRADS, ADAM_M, ADAM_V): go2sim_distill_n_padded floats. */
int go2sim_distill_n_padded(go2sim_distill_t* h, size_t* out);
int go2sim_distill_export_padded(go2sim_distill_t* h, int which, float* padded_dev, void* stream);

/* Optimizer state that is not a vector: the step count (host side) and the learning rate (device scalar, set in stream order). */
int go2sim_distill_set_step(go2sim_distill_t* h, long long step, double learning_rate, void* stream);
int go2sim_distill_reset_stats(go2sim_distill_t* h, void* stream);
/* out_dev: GO2SIM_DISTILL_N_STATS float64 on the device, written in stream order */
int go2sim_distill_stats(go2sim_distill_t* h, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
