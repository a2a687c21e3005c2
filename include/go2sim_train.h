/* go2sim_train.h -- C ABI of the PPO update that follows a rollout: the other half of a training iteration next to
 * include/go2sim_policy.h (act / rollout storage).  It replaces `rsl_rl.algorithms.PPO.update` (rsl-rl-lib==2.2.4) as the train scripts
 * configure it (examples/locomotion/final/go2_train_walk.py:23-65): clipped surrogate + clipped value loss + entropy bonus, adaptive learning
 * rate from the KL divergence, global gradient-norm clip, Adam.
 *
 * Conventions follow go2sim_policy.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call synchronises with the host.  There is no CPU twin of these calls: the checker is torch float64 autograd (tests/ppo_ref.py).
 *
 * The law, per mini-batch of n rows selected through idx (all means over the n rows):
 *   mu = actor(obs);  sigma = std (used as is);  v = critic(critic_obs)
 *   logp    = sum_a( -(a - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi) )
 *   entropy = sum_a( 0.5 + 0.5 log(2 pi) + log sigma )
 *   kl      = sum_a( log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mu)^2) / (2 sigma^2) - 0.5 )
 *   adaptive schedule, before the optimizer step: kl_mean > 2 desired_kl: lr = max(1e-5, lr / 1.5); 0 < kl_mean < desired_kl / 2: lr = min(1e-2, 1.5 lr)
 *   ratio = exp(logp - old_log_prob);  surrogate = mean(max(-adv ratio, -adv clamp(ratio, 1 - clip, 1 + clip)))
 *   v_clipped = target_values + clamp(v - target_values, -clip, clip);  value_loss = mean(max((v - returns)^2, (v_clipped - returns)^2))
 *   loss = surrogate + value_loss_coef value_loss - entropy_coef mean(entropy)
 *   grads *= min(1, max_grad_norm / (||grads|| + 1e-6));  Adam(lr, betas, eps), bias corrections from the step count in float64
 * Gradients at the ties of the two max() are torch's: inside the clip range both arms are the same function and the full gradient flows, outside
 * it the clipped arm contributes nothing when it is the larger one.
 *
 * Numerics: fp32 on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains), float64 for every scalar reduction and for the sums over row chunks; no
 * floating-point atomics, every sum in a fixed order: the same inputs give the same bits on every run.  Against torch float64 autograd, per
 * parameter tensor,  max|g - g64| <= C_GRAD max(max|g32 - g64|, 2^-24 max|g64|)  with g32 the torch float32 CPU evaluation of the same
 * expressions, and after whole updates  max|p - p64| <= C_UPD max|p32 - p64|.
 *   C_GRAD = 16   (worst measured over tests/ppo_cases.py on the MI355X: 6.76, on the single entry of the six-layer critic's last bias at 17 rows --
 *                  a sum of 17 signed d loss / d v whose float32 torch value happens to land close to float64; the worst tensor with more
 *                  than one entry is at 2.79)
 *   C_UPD  = 8    (worst measured: 3.79, 2 epochs x 2 mini-batches of 37 rows)
 * Rows are reduced in chunks of GO2SIM_PPO_ROW_CHUNK: a chain of the matrix instruction never runs over more than a quarter of a chunk.
 *
 * Mirror symmetry (go2sim_ppo_set_mirror; rsl_rl 2.2.4's symmetry_cfg with the mirror given as tables).  A mirror is three signed permutations
 * M_o, M_c, M_a for the actor input, the critic input and the actions, each acting as (M x)[j] = sign[j] x[src[j]].  A mini-batch of n rows read
 * through idx becomes 2 n rows: rows 0 .. n-1 are the originals, row n + r is the mirror of row r: obs M_o obs_r, critic obs M_c cobs_r, actions
 * M_a a_r, and old_log_prob, advantages, returns and target_values of row r unchanged.  The 2 n rows run through the row chunks as one sequence.
 *   use_data_augmentation: surrogate and value_loss are means over all 2 n rows (row weight 1 / (2 n)), d loss / d sigma takes both halves;
 *     kl_mean, and the learning-rate rule that reads it, over the n original rows only; entropy does not depend on rows.
 *   use_mirror_loss: L_sym = mean over r < n, a < A of (mu(M_o obs_r)[a] - (M_a mu(obs_r))[a])^2;  loss += mirror_loss_coeff L_sym.  The target
 *     M_a mu(obs_r) is detached: the gradient enters through the mirrored rows' mu only, coeff 2 (mu' - target) / (n A).
 *   mirror loss without augmentation: forward and backward still run on 2 n rows, the mirrored rows carry no PPO weight, the originals weigh 1 / n;
 *     surrogate, value_loss and kl are means over n.
 *   both flags off: gradients, statistics and parameters have the bits of a handle without tables.
 * L_sym is computed and reported (go2sim_ppo_symmetry_loss) whenever a mirror is set; it is added to the loss only under use_mirror_loss.
 * No mirrored copy of a batch array is written anywhere and the batch arrays are never modified: the signed gather sits where rows are read
 * through idx already.  All sums stay float64 in a fixed order.  The bounds above hold with the mirror on; worst measured over
 * tests/test_ppo_sym_gpu.py on the MI355X: 1.77 against C_GRAD (17 rows, mirror loss only; sharded 1.29), 1.00 against C_UPD (2 epochs x 2 mini-batches of
 * 37 rows, both flags).
 */
#ifndef GO2SIM_TRAIN_H
#define GO2SIM_TRAIN_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_PPO_ROW_CHUNK 512
#define GO2SIM_PPO_N_STATS 8

typedef struct go2sim_ppo go2sim_ppo_t;

typedef struct go2sim_ppo_cfg {
  double clip_param, desired_kl, entropy_coef, learning_rate, max_grad_norm, value_loss_coef;
  double beta1, beta2, eps;   /* Adam; 0.9, 0.999, 1e-8 in the reference */
  double lr_min, lr_max;      /* bounds of the adaptive schedule; 1e-5, 1e-2 in the reference */
  int use_clipped_value_loss;
  int adaptive;               /* 1: schedule "adaptive", 0: "fixed" */
} go2sim_ppo_cfg_t;

/* The rollout as flat row arrays (device pointers, T * B rows, row-major); a mini-batch reads its rows through an index array, no gathered copy is made. */
typedef struct go2sim_ppo_batch {
  const float* obs;            /* [rows][actor input width] */
  const float* critic_obs;     /* [rows][critic input width] */
  const float* actions;        /* [rows][A] */
  const float* target_values;  /* [rows] values stored at collection */
  const float* returns;        /* [rows] */
  const float* advantages;     /* [rows] already normalised */
  const float* old_log_prob;   /* [rows] */
  const float* old_mu;         /* [rows][A] */
  const float* old_sigma;      /* [rows][A] */
} go2sim_ppo_batch_t;

/* Three signed permutations as device tables (int32 src, float sign of +1 or -1) of the actor's input width, the critic's input width and
 * n_actions entries, the two flags and the coefficient of the law above. */
typedef struct go2sim_ppo_mirror {
  const int32_t* obs_src;
  const float* obs_sign;
  const int32_t* critic_src;
  const float* critic_sign;
  const int32_t* action_src;
  const float* action_sign;
  int use_data_augmentation;
  int use_mirror_loss;
  double mirror_loss_coeff;
} go2sim_ppo_mirror_t;

enum go2sim_ppo_vec { GO2SIM_PPO_PARAMS = 0, GO2SIM_PPO_GRADS, GO2SIM_PPO_ADAM_M, GO2SIM_PPO_ADAM_V };
/* go2sim_ppo_stats writes GO2SIM_PPO_N_STATS float64: means of value loss, surrogate loss and entropy over the mini-batches since the last reset,
 * kl_mean of the last mini-batch, learning rate, total gradient norm of the last apply, optimizer step count, mini-batches since the last reset */
enum go2sim_ppo_stat { GO2SIM_PPO_ST_VALUE_LOSS = 0, GO2SIM_PPO_ST_SURROGATE, GO2SIM_PPO_ST_ENTROPY, GO2SIM_PPO_ST_KL, GO2SIM_PPO_ST_LR,
                       GO2SIM_PPO_ST_GRAD_NORM, GO2SIM_PPO_ST_STEP, GO2SIM_PPO_ST_COUNT };

/* The handle owns the workspaces (activations, row-chunk partials), the gradients and Adam's m, v, step count and learning rate.  It does not own the
 * two networks: the optimizer writes into the weight arrays the two go2sim_mlp_t handles serve go2sim_policy_act from.  n_actions must equal the
 * actor's last width, the critic's last width must be 1. */
int go2sim_ppo_create(go2sim_mlp_t* actor, go2sim_mlp_t* critic, int n_actions, const go2sim_ppo_cfg_t* cfg, int max_rows_per_minibatch, go2sim_ppo_t** out);
int go2sim_ppo_destroy(go2sim_ppo_t* h);

/* Sets (or, with NULL, removes) the mirror.  A set-up call like go2sim_ppo_create: it reads the tables back to validate them on the host (indices in
 * range, each src a permutation, signs +1 or -1; GO2SIM_E_BADARG otherwise, the handle unchanged), copies them into the handle and sizes the
 * workspaces for 2 x max_rows_per_minibatch, so it waits for the device.  The optimizer state, the learning rate and the running sums are kept.
 * Every call below honours the mirror.  With a mirror set a shard record grows by one entry (go2sim_ppo_shard_len). */
int go2sim_ppo_set_mirror(go2sim_ppo_t* h, const go2sim_ppo_mirror_t* mirror, void* stream);
/* out_dev: one float64 on the device, the mean of L_sym over the mini-batches since the last reset (0 without a mirror), written in stream order */
int go2sim_ppo_symmetry_loss(go2sim_ppo_t* h, double* out_dev, void* stream);

/* Forward, loss head and backward of one mini-batch: rows idx[0 .. n_rows) of `batch` (int32 device indices).  Leaves the gradients on the device,
 * applies the learning-rate rule to the device-side learning rate and adds this mini-batch to the running sums of the three reported means. */
int go2sim_ppo_minibatch_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* batch, const float* std_dev, const int32_t* idx_dev, int n_rows, void* stream);
/* One policy trained across ranks (data parallel): every rank runs go2sim_ppo_shard_grad on its shard of the mini-batch, the ranks exchange the
 * records (one all-gather, distributed.allgather_records), every rank runs go2sim_ppo_shard_reduce on the same records in the same order, then
 * go2sim_ppo_apply.  All ranks add the same float64 numbers in the same (record) order and round once, so they hold bit-identical gradients,
 * learning rates and, after the step, parameters; no parameter is ever re-broadcast.
 *
 * A record is go2sim_ppo_shard_len float64 (= go2sim_ppo_n_padded + 4), in the padded layout actor | critic | std of the gradient vector:
 *   [0, nA + nC)             the shard's chunk slabs of dW / db added in chunk order, not rounded; every row weighted 1 / n_rows_global
 *   [nA + nC, + Apad)        d loss / d sigma[a] summed over the head's workgroups in workgroup order, WITHOUT the entropy term (it does not depend on
 *                            rows: the reduction adds it once); entries a >= n_actions are zero
 *   [nA + nC + Apad, + 4)    the shard's unnormalised sums over rows of surrogate, value loss and kl, then n_rows as a double
 *   with a mirror set, one more entry: the shard's unnormalised sum over mirrored rows and actions of (mu' - target)^2; under augmentation the sums
 *   of surrogate and value loss run over originals and mirrors (divided by twice the row count), n_rows stays the count of original rows
 * Padded entries are exact zeros.  With one record and n_rows_global = n_rows, shard_grad + shard_reduce leave the handle in the state of
 * go2sim_ppo_minibatch_grad bit for bit.
 *
 * go2sim_ppo_shard_grad: forward, head and backward of rows idx[0 .. n_rows) with weight 1 / n_rows_global (n_rows <= n_rows_global); writes
 * record_dev and nothing else the other calls read: the learning rate, kl_mean, the running sums and the gradient vector are left alone. */
int go2sim_ppo_shard_len(go2sim_ppo_t* h, size_t* out);
int go2sim_ppo_shard_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* batch, const float* std_dev, const int32_t* idx_dev, int n_rows,
                          long long n_rows_global, double* record_dev, void* stream);
/* records_dev [n_records][shard_len], added entry by entry in record order in float64 and rounded once into the gradient vector; the std block gets
 * - entropy_coef / std; the three sums are divided by the records' total row count, the learning-rate rule is applied to that global kl_mean, and the
 * mini-batch is added to the running sums of the reported means, as go2sim_ppo_minibatch_grad does for its own rows. */
int go2sim_ppo_shard_reduce(go2sim_ppo_t* h, const double* records_dev, int n_records, const float* std_dev, void* stream);
/* Global-norm clip and one Adam step on the gradients the handle holds, written to the two networks' weights and to std_dev[A]. */
int go2sim_ppo_apply(go2sim_ppo_t* h, float* std_dev, void* stream);
/* The whole update: resets the running sums, then for every epoch and mini-batch i the two calls above on perm_dev[i * mbs .. (i + 1) * mbs),
 * mbs = n_rows_total / n_mini_batches (rows beyond n_mini_batches * mbs are dropped). */
int go2sim_ppo_update(go2sim_ppo_t* h, const go2sim_ppo_batch_t* batch, float* std_dev, const int32_t* perm_dev, int n_rows_total, int n_epochs,
                      int n_mini_batches, void* stream);

/* One of the handle's vectors as a flat device vector in unpadded state-dict order: actor W0, b0, ..., critic W0, b0, ..., std.
 * std_dev is read / written for GO2SIM_PPO_PARAMS only (may be NULL otherwise).  go2sim_ppo_n_params gives the length. */
int go2sim_ppo_n_params(go2sim_ppo_t* h, size_t* out);
int go2sim_ppo_export(go2sim_ppo_t* h, int which, float* flat_dev, const float* std_dev, void* stream);
int go2sim_ppo_import(go2sim_ppo_t* h, int which, const float* flat_dev, float* std_dev, void* stream);
/* Test access to a padded buffer as the kernels hold it (GRADS, ADAM_M, ADAM_V): actor | critic | std, go2sim_ppo_n_padded floats. */
int go2sim_ppo_n_padded(go2sim_ppo_t* h, size_t* out);
int go2sim_ppo_export_padded(go2sim_ppo_t* h, int which, float* padded_dev, void* stream);

/* Optimizer state that is not a vector: the step count (host side) and the learning rate (device scalar, set in stream order). */
int go2sim_ppo_set_step(go2sim_ppo_t* h, long long step, double learning_rate, void* stream);
int go2sim_ppo_reset_stats(go2sim_ppo_t* h, void* stream);
/* out_dev: GO2SIM_PPO_N_STATS float64 on the device, written in stream order */
int go2sim_ppo_stats(go2sim_ppo_t* h, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
