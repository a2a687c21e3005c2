/* go2sim_rdistill.h -- C ABI of teacher-student distillation with a recurrent student: an LSTM memory in front of the student's MLP (and, optionally, in
 * front of the teacher's), the collection step and the behaviour-cloning update as truncated backpropagation through time.  It restates
 * `rsl_rl.modules.StudentTeacherRecurrent` and the recurrent branch of `rsl_rl.algorithms.Distillation.update` (rsl_rl 2.3) on the memory cell of
 * include/go2sim_rnn.h, the fused MLP of include/go2sim_policy.h, the behaviour loss of include/go2sim_distill.h and the backward kernels of
 * include/go2sim_train.h.  Conventions follow those headers: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is
 * ordered on the given stream, no call synchronises with the host.  There is no CPU twin: the checker is torch float64 (tests/rdistill_ref.py).
 *
 * The law.
 *   Modules: memory_s = LSTM(num_student_obs -> H), one layer, gates and cell law of go2sim_rnn.h; student = MLP(H -> student_hidden_dims -> A).  With a
 *   recurrent teacher memory_t = LSTM(num_teacher_obs -> Ht) and teacher = MLP(Ht -> teacher_hidden_dims -> A), otherwise teacher = MLP(num_teacher_obs ->
 *   teacher_hidden_dims -> A).  std[A] = init_noise_std gets no gradient and sits outside the optimizer.
 *   Collection, per env step: memory_s steps on obs from the live state; mean = student(h_s'); actions = mean + std n with n from the Philox stream of
 *   go2sim_policy_act (same key, purpose 11, same counter layout); teacher_actions = teacher(h_t') after a memory_t step on teacher_obs, or
 *   teacher(teacher_obs).  The env steps on the student's actions; after it h and c of the done envs are 0 in every memory (the next step's `reset`).
 *   At the rollout's first act the student's state S = (h_s, c_s), [N][H] each, is saved.  Stored per step: obs [T][N][Ds], teacher_actions [T][N][A],
 *   dones [T][N].
 *   Update: cnt = 0; for each epoch e < E the student's state becomes S; for each step t < T: the cell steps on obs[t], mean = student(h'), l_t as in
 *   go2sim_distill.h (mse or huber, mean over N envs and A actions), cnt += 1 and the pair (e, t) joins the open window; when cnt % G == 0 the window
 *   closes: gradient of the sum of its l_t, optional global-norm clip over student and memory_s together, one Adam step, a new window opens; the state
 *   entering t + 1 is 0 for envs with dones[t].  Parameters are constant inside a window.  The gradient flows back through the cell from pair to pair
 *   within the window; the carried dh and dc are zero into the window's first pair, into the first step of an epoch (S is a constant) and, for an env,
 *   across a step with dones[t] set.  The forward state is not cut by a window close: it is carried on as computed under the parameters that were in
 *   force.  Pairs left in an open window at the end are a dropped tail: forward, head and loss statistic run for them and the state advances, they get
 *   no backward.  mean_behavior_loss = sum of all E T l_t / (E T).  After the update the student's state is the one left by the last epoch's last step
 *   with dones[T - 1] applied; the next rollout starts from it and saves it as its S.
 *   DEVIATION from rsl_rl: the update leaves memory_t's state alone (rsl_rl rewinds the teacher's memory to a stale copy at every epoch, which wipes a
 *   recurrent teacher's memory at the first update).
 *   Clip, Adam, float64 scalars, fixed-order sums, no floating-point atomics: as in go2sim_distill.h and go2sim_train.h.  bias_ih and bias_hh are two
 *   parameters with equal gradients and their own Adam moments.
 *
 * Segments.  A window is a list of segments; a segment is a run of consecutive steps t0 .. t0 + n_steps - 1 of one epoch.  A segment with t0 = 0 starts
 * from S; a segment with t0 > 0 continues the carried state and can only be a window's first.  Inside a segment the backward pass carries dh and dc from
 * step to step (cut, per env, by dones[t]); at a segment's last step nothing is carried in.  (T, E, G) = (3, 2, 4): one window of the segments
 * (t0 = 0, 3 steps), (t0 = 0, 1 step) and a tail of one segment (t0 = 1, 2 steps).  At most GO2SIM_RDISTILL_MAX_SEGS segments per window.
 *
 * Memory.  A window at the training shape (G N = 15 x 4096 rows, H = 256) would store 0.5 GB of gates and states.  The handle WALKS THE WINDOW IN ENV
 * BLOCKS of sub_envs envs (default GO2SIM_RDISTILL_SUB_ENVS = 1024: 0.30 GB of row workspaces and 64 MB of chunk slabs at that shape): for each block the forward through the window's steps with the gates kept, the head, the
 * MLP's backward, the walk back through time and the weight gradients reuse one set of row workspaces; the block's chunk slabs are added, in block and
 * chunk order, onto a float64 accumulator that is rounded once after the last block.  The carried state [N][H] lives in the caller's arrays.  The bits
 * may depend on sub_envs (a block boundary moves rows between chunks); for a fixed value they are the same on every run.
 * A cell step over a block is a latency chain, not throughput (36 us at 512 envs, 70 us at 4096 on the MI355X), so the update's time goes with the number of
 * blocks: 15.5 / 9.8 / 5.8 ms at sub_envs = 512 / 1024 / 4096 for 4096 envs x 24 steps, G = 15 (DESIGN.md "Recurrent student").
 *
 * Numerics: against torch float64 (nn.LSTM + autograd), per parameter tensor, max|g - g64| <= C_GRAD max(max|g32 - g64|, 2^-24 max|g64|), after whole
 * updates max|p - p64| <= C_UPD max|p32 - p64|, the final state and the means under C_MLP (C_GRAD = 16, C_UPD = 8 of go2sim_train.h, C_MLP = 7 of
 * go2sim_policy.h; float32 torch is the yardstick).
 * Worst measured over tests/test_rdistill_gpu.py on the MI355X: 3.15 against C_GRAD (the student's last weight in the window that opens inside an epoch,
 * 3 steps x 37 envs, H = 48; the worst LSTM tensor is weight_ih of the same window at 2.15), 4.53 against C_UPD (weight_hh after
 * the two windows of (T, E, G) = (4, 2, 4) at 37 envs walked in three blocks of 16; most tensors sit at 1.00: one or two Adam steps of size lr land on
 * the float32 yardstick's own values), 2.53 against C_MLP (h after the 3-step window at H = 256, 16 envs; the means 1.36); the loss statistic agrees with
 * a float64 evaluation on the library's own means to 2.6e-16 relative.
 */
#ifndef GO2SIM_RDISTILL_H
#define GO2SIM_RDISTILL_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim_distill.h"
#include "go2sim_policy.h"
#include "go2sim_rnn.h"
#include "go2sim_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_RDISTILL_SUB_ENVS 1024
#define GO2SIM_RDISTILL_MAX_SEGS 32
#define GO2SIM_RDISTILL_N_STATS 6

typedef struct go2sim_rdistill go2sim_rdistill_t;

enum go2sim_rdistill_loss { GO2SIM_RDISTILL_MSE = 0, GO2SIM_RDISTILL_HUBER };
enum go2sim_rdistill_vec { GO2SIM_RDISTILL_PARAMS = 0, GO2SIM_RDISTILL_GRADS, GO2SIM_RDISTILL_ADAM_M, GO2SIM_RDISTILL_ADAM_V };
/* go2sim_rdistill_stats writes GO2SIM_RDISTILL_N_STATS float64, the six of go2sim_distill_stats */
enum go2sim_rdistill_stat { GO2SIM_RDISTILL_ST_LOSS = 0, GO2SIM_RDISTILL_ST_LR, GO2SIM_RDISTILL_ST_GRAD_NORM, GO2SIM_RDISTILL_ST_STEP, GO2SIM_RDISTILL_ST_PAIRS,
                            GO2SIM_RDISTILL_ST_WINDOWS };

typedef struct go2sim_rdistill_cfg {
  double learning_rate;
  double max_grad_norm;       /* <= 0: no clip */
  double beta1, beta2, eps;   /* Adam; 0.9, 0.999, 1e-8 */
  int loss_type;              /* enum go2sim_rdistill_loss */
  int sub_envs;               /* envs of a block; 0: GO2SIM_RDISTILL_SUB_ENVS */
} go2sim_rdistill_cfg_t;

/* one rollout as the update reads it */
typedef struct go2sim_rdistill_roll {
  const float* obs;              /* [T][N][Ds] */
  const float* teacher_actions;  /* [T][N][A] */
  const uint8_t* dones;          /* [T][N] */
  const float *h0, *c0;          /* S: the student's state at the rollout's first act, [N][H]; never written */
  float *h, *c;                  /* the carried state [N][H]: read by a window whose first segment has t0 > 0, written by every window */
  int n_steps, n_envs;           /* T, N */
} go2sim_rdistill_roll_t;

typedef struct go2sim_rdistill_seg { int t0, n_steps; } go2sim_rdistill_seg_t;

/* The collection step in three launches: ONE k_lstm_cell launch for memory_s and (mem_t given) memory_t, whose `reset` (u8 [n_rows] or NULL: the previous
 * step's dones) zeroes the state the done rows enter with; both MLPs side by side, the student on h_s', the teacher on h_t' (or on teacher_obs when mem_t
 * is NULL); the sampling kernel of go2sim_policy_act on the student's mean.  Writes the new states and actions, mean, teacher_actions [n_rows][A]; they
 * equal go2sim_lstm_step followed by go2sim_distill_act on h' bit for bit.  h_out must not be h_in (c_out may be c_in).  The *_t state arrays are read
 * only with mem_t.  mem_s->H must be the student's first width, mem_t->H the teacher's. */
int go2sim_rdistill_act(go2sim_lstm_t* mem_s, go2sim_mlp_t* student, go2sim_lstm_t* mem_t, go2sim_mlp_t* teacher, const float* obs, const float* teacher_obs,
                        const float* std_dev, const uint8_t* reset, const float* h_in_s, const float* c_in_s, float* h_out_s, float* c_out_s, const float* h_in_t,
                        const float* c_in_t, float* h_out_t, float* c_out_t, int n_rows, uint64_t seed, uint32_t step, int deterministic, float* actions, float* mean,
                        float* teacher_actions, void* stream);

/* The trainer handle over memory_s + student: workspaces, gradients, Adam's m and v, the step count and the learning rate; the optimizer writes the arrays
 * go2sim_rdistill_act reads.  n_actions must equal the student's last width and mem_s->H its first; max_window_rows is the workspace: a window of P pairs
 * over N envs needs P x min(sub_envs, N) rows. */
int go2sim_rdistill_create(go2sim_lstm_t* mem_s, go2sim_mlp_t* student, int n_actions, const go2sim_rdistill_cfg_t* cfg, int max_window_rows, go2sim_rdistill_t** out);
int go2sim_rdistill_destroy(go2sim_rdistill_t* h);

/* One window: the segments' pairs in order (host array, read before the call returns).  Leaves the gradient on the device, adds the pairs to the running
 * loss sum and writes the carried state: the state after the window's last step t with dones[t] applied.  go2sim_rdistill_loss_only: forward, head and
 * state alone (the dropped tail): the gradient does not move. */
int go2sim_rdistill_window_grad(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, const go2sim_rdistill_seg_t* segs, int n_segs, void* stream);
int go2sim_rdistill_loss_only(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, const go2sim_rdistill_seg_t* segs, int n_segs, void* stream);
/* Optional global-norm clip over student and memory_s together and one Adam step on the gradient the handle holds. */
int go2sim_rdistill_apply(go2sim_rdistill_t* h, void* stream);
/* The whole update: resets the running sums, then every window of (T, N, E, G) followed by go2sim_rdistill_apply, then the loss-only pass over the
 * dropped tail.  roll->h / roll->c end as the final state.  No host synchronisation. */
int go2sim_rdistill_update(go2sim_rdistill_t* h, const go2sim_rdistill_roll_t* roll, int n_epochs, int gradient_length, void* stream);

/* One of the handle's vectors as a flat device vector in unpadded state-dict order: student W0, b0, W1, b1, ..., memory_s weight_ih, weight_hh, bias_ih,
 * bias_hh (std is not part of it).  The padded layout is student | memory_s. */
int go2sim_rdistill_n_params(go2sim_rdistill_t* h, size_t* out);
int go2sim_rdistill_export(go2sim_rdistill_t* h, int which, float* flat_dev, void* stream);
int go2sim_rdistill_import(go2sim_rdistill_t* h, int which, const float* flat_dev, void* stream);
int go2sim_rdistill_n_padded(go2sim_rdistill_t* h, size_t* out);
int go2sim_rdistill_export_padded(go2sim_rdistill_t* h, int which, float* padded_dev, void* stream);

int go2sim_rdistill_set_step(go2sim_rdistill_t* h, long long step, double learning_rate, void* stream);
int go2sim_rdistill_reset_stats(go2sim_rdistill_t* h, void* stream);
/* out_dev: GO2SIM_RDISTILL_N_STATS float64 on the device, written in stream order */
int go2sim_rdistill_stats(go2sim_rdistill_t* h, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
