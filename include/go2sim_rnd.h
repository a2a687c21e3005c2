/* go2sim_rnd.h -- C ABI of random network distillation (RND), the curiosity bonus of `rsl_rl.algorithms.PPO` (`rnd_cfg`,
 * `rsl_rl.modules.RandomNetworkDistillation`): the per-env-step intrinsic reward and the update of the predictor.  It stands on the fused MLP of
 * include/go2sim_policy.h, the backward kernels of the PPO update (include/go2sim_train.h; csrc/go2sim_train_dev.h), the MSE head of distillation
 * (csrc/go2sim_distill_dev.h) and the float64 chunked moments of the observation normaliser (include/go2sim_norm.h; csrc/go2sim_norm_dev.h).
 * rsl_rl is a third-party package that is not part of the reference tree; the law is stated here.
 *
 * Conventions follow go2sim_train.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given stream,
 * no call synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is torch / numpy float64
 * (tests/rnd_ref.py).
 *
 * The law.
 *   Modules: predictor = MLP(num_states -> predictor_hidden_dims -> E), target = MLP(num_states -> target_hidden_dims -> E), E = num_outputs; both with
 *   the configured activation (any of include/go2sim_activation.h) after every layer but the last; depths and widths independent of each other within
 *   GO2SIM_MLP_MAX_LAYERS / _WIDTH.  The target is never trained.
 *   Per env step, on the N rows the env returned, in this order:
 *     1. counter += 1 (a host integer; the caller's, it is saved in the checkpoint).
 *     2. s = norm_step(state_normalizer, rnd_state, update) if a state normaliser is given (the law of go2sim_norm.h; the runner uses eps = 1e-2,
 *        until = 1e8), otherwise s = rnd_state.  s is what the update later reads.
 *     3. t = target(s), p = predictor(s): each bit-equal to go2sim_mlp_forward of that network on s.
 *     4. r[n] = sqrt(sum_e (t[n][e] - p[n][e])^2): differences, squares, the sum (in the order of e) and the root in float64 from the float32
 *        embeddings, rounded to float32 once.
 *     5. The reward normaliser, if on (rsl_rl's EmpiricalDiscountedVariationNormalization, gamma = 0.99, until = 1e8): avg[n] = 0.99f * avg[n] + r[n] in
 *        float32, one multiply and one add, each rounded (no fma); avg starts at 0 and is NOT reset on dones.  If count < until, the N values of avg are folded into a one-column (mean, var, std, count) state with exactly the update
 *        law of go2sim_norm.h: float64 two-pass moments per chunk of GO2SIM_NORM_ROW_CHUNK rows in row order, the chunks in chunk order, the state
 *        stored as float32, each entry rounded once.  With the state as it is after the fold: r[n] = r[n] / std if std > 0, else unchanged.  There is
 *        no eps; the division is a correctly rounded float32 division.
 *     6. The weight w(counter) is computed in float64 on the host and passed as an argument (w0 = rnd_cfg["weight"] as the runner scaled it):
 *          None or {"mode": "constant"}:                                            w0
 *          {"mode": "step", "final_step": S, "final_value": v}:                     v if counter >= S, else w0
 *          {"mode": "linear", "initial_step": a, "final_step": b, "final_value": v}: w0 for counter < a; v for counter > b;
 *                                                                                   w0 + (v - w0) (counter - a) / (b - a) between
 *        intrinsic[n] = float32(w) * r[n].
 *     7. rewards_total[n] = rewards[n] + intrinsic[n], into the caller's buffer: the env's reward array is not written.  rewards_total is what the
 *        rollout storage takes; its time-out bootstrap comes after the bonus, as in rsl_rl.
 *   Update, on the stored s [rows][num_states]: for every epoch and mini-batch the same row list the policy's update uses (slices of the update's one
 *   permutation for the MLP policy; env blocks with all their steps, t-major, for the recurrent policy):
 *     L = mean over the mini-batch's rows and the E outputs of (predictor(s) - target(s))^2;  d L / d p[row][e] = 2 (p - t) / (n_rows E)
 *   then one Adam step, Adam(learning_rate, 0.9, 0.999, 1e-8): fixed learning rate, NO gradient clip, bias corrections in float64 from the step count.
 *   Reported rnd_loss = mean of L over the mini-batches since the last reset.
 *   The predictor's parameters and optimizer are disjoint from the policy's and neither loss reads the other's parameters, so the predictor's
 *   mini-batch steps run as a loop of their own next to go2sim_ppo_update / go2sim_ppo_rnn_update; the results are those of rsl_rl's interleaving.
 *
 * Numerics follow go2sim_train.h: fp32 fma chains on v_mfma_f32_16x16x4_f32, float64 for every scalar and every sum over chunks or workgroups, no
 * floating-point atomics, every sum in a fixed order (equal calls on equal states give equal bits), padded entries exact zeros.  Against torch float64
 * autograd, per predictor tensor,  max|g - g64| <= C_GRAD max(max|g32 - g64|, 2^-24 max|g64|)  and after whole updates
 * max|p - p64| <= C_UPD max|p32 - p64|  with the constants of go2sim_train.h (C_GRAD = 16, C_UPD = 8).
 * Worst measured over tests/test_rnd_gpu.py on the MI355X: 1.73 against C_GRAD (the 49-272-20 predictor's last bias, a mini-batch of 17 rows), 2.22 against C_UPD
 * (the same predictor's last bias after 5 epochs x 4 mini-batches; most update cases sit at 1.00: Adam steps of size lr land on the float32 yardstick's own
 * values); the distance reaches 1.000 of its bound 2^-24 r64; the reward normaliser's state stays within 0.83 of the bounds of tests/norm_ref.py; the loss
 * statistic agrees with a float64 evaluation on the library's own embeddings to 3.3e-16 relative.
 *
 * Launches (csrc/go2sim_rnd.hip).  go2sim_rnd_step, after the state normaliser's own launches (go2sim_norm_step, the caller's):
 *   k_mlp_forward   target and predictor side by side (blockIdx.y), as go2sim_policy_act runs actor and critic
 *   k_rnd_reward    one workgroup of GO2SIM_NORM_ROW_CHUNK lanes per chunk of rows, one row per lane: r, avg, the chunk's float64 moments of avg;
 *                   the workgroup that finishes last (an integer ticket, no floating-point atomic) folds the chunks in chunk order, applies the
 *                   law of go2sim_norm.h to the one-column state and writes intrinsic and rewards_total of every row.  Without the reward
 *                   normaliser every workgroup writes its own rows and there is no ticket.
 * A mini-batch of the update: k_train_forward with predictor and target side by side, rows through the index list (the predictor's activations are
 * kept for the backward pass; the target runs the layer loop of k_mlp_forward, so its embedding has go2sim_mlp_forward's bits), the MSE head
 * k_distill_head with weight 1 / (n_rows E), then k_bwd_dw / k_bwd_db / k_bwd_da per layer, k_reduce_partials, k_distill_finalize, and k_sumsq + k_adam.
 */
#ifndef GO2SIM_RND_H
#define GO2SIM_RND_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim_norm.h"
#include "go2sim_policy.h"
#include "go2sim_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_RND_N_STATS 6

typedef struct go2sim_rnd go2sim_rnd_t;

enum go2sim_rnd_vec { GO2SIM_RND_PARAMS = 0, GO2SIM_RND_GRADS, GO2SIM_RND_ADAM_M, GO2SIM_RND_ADAM_V };
/* go2sim_rnd_stats writes GO2SIM_RND_N_STATS float64: mean of L over the mini-batches since the last reset, learning rate, gradient norm of the last
 * apply, optimizer steps, mini-batches counted since the last reset, Adam steps since the last reset */
enum go2sim_rnd_stat { GO2SIM_RND_ST_LOSS = 0, GO2SIM_RND_ST_LR, GO2SIM_RND_ST_GRAD_NORM, GO2SIM_RND_ST_STEP, GO2SIM_RND_ST_MINIBATCHES, GO2SIM_RND_ST_APPLIES };

typedef struct go2sim_rnd_cfg {
  double learning_rate;
  double beta1, beta2, eps;   /* Adam; 0.9, 0.999, 1e-8 */
  int reward_normalization;   /* item 5 of the law on / off */
} go2sim_rnd_cfg_t;

/* The handle over the predictor's and the target's go2sim_mlp_t: it owns the embeddings, the reward normaliser's state and avg[max_rows], the update's
 * workspaces, the gradients, Adam's m and v, the step count and the learning rate; the optimizer writes the predictor's weight arrays.  max_rows bounds
 * the rows of a step and of a mini-batch.  GO2SIM_E_BADARG for a NULL pointer, max_rows < 1, networks whose first or last widths differ or that live
 * on different devices, or predictor == target.  Waits for the device. */
int go2sim_rnd_create(go2sim_mlp_t* predictor, go2sim_mlp_t* target, const go2sim_rnd_cfg_t* cfg, int max_rows, go2sim_rnd_t** out);
int go2sim_rnd_destroy(go2sim_rnd_t* h);

/* Items 3 to 7 of the law on s [n_rows][num_states] (item 2 is go2sim_norm_step, called by the owner of the state normaliser before this): writes
 * intrinsic [n_rows] and rewards_total [n_rows]; rewards [n_rows] is read only.  With the reward normaliser on, n_rows must be the same in every call
 * since the last go2sim_rnd_set_reward_state (avg has one entry per row).  Two launches; none for n_rows == 0 (success, nothing moves).
 * GO2SIM_E_BADARG for a NULL pointer, n_rows < 0 or n_rows > max_rows. */
int go2sim_rnd_step(go2sim_rnd_t* h, const float* s, const float* rewards, int n_rows, double weight, float* intrinsic, float* rewards_total, void* stream);
/* Test access to what the last go2sim_rnd_step computed: the embeddings t and p [n_rows][E] and r [n_rows] as it was before the reward normaliser. */
int go2sim_rnd_last_step(go2sim_rnd_t* h, float* target_emb_dev, float* predictor_emb_dev, float* r_dev, int n_rows, void* stream);

/* One mini-batch: rows idx[0 .. n_rows) of s [.][num_states] (int32 device indices; a row may appear more than once), every row weighted
 * 1 / (n_rows E).  Leaves the gradient on the device and adds L to the running loss sum. */
int go2sim_rnd_minibatch_grad(go2sim_rnd_t* h, const float* s, const int32_t* idx_dev, int n_rows, void* stream);
/* One Adam step (no clip) on the gradient the handle holds, written to the predictor's weights. */
int go2sim_rnd_apply(go2sim_rnd_t* h, void* stream);
/* The whole update: resets the running loss, then for every epoch e < n_epochs and mini-batch i < n_mini_batches, with mbs = n_rows_total /
 * n_mini_batches, go2sim_rnd_minibatch_grad on idx[i mbs .. (i + 1) mbs) followed by go2sim_rnd_apply.  No host synchronisation. */
int go2sim_rnd_update(go2sim_rnd_t* h, const float* s, const int32_t* idx_dev, int n_rows_total, int n_epochs, int n_mini_batches, void* stream);

/* One of the handle's vectors as a flat device vector in unpadded state-dict order: predictor W0, b0, W1, b1, ... */
int go2sim_rnd_n_params(go2sim_rnd_t* h, size_t* out);
int go2sim_rnd_export(go2sim_rnd_t* h, int which, float* flat_dev, void* stream);
int go2sim_rnd_import(go2sim_rnd_t* h, int which, const float* flat_dev, void* stream);
/* Test access to a padded buffer as the kernels hold it (PARAMS, GRADS, ADAM_M, ADAM_V): go2sim_rnd_n_padded floats. */
int go2sim_rnd_n_padded(go2sim_rnd_t* h, size_t* out);
int go2sim_rnd_export_padded(go2sim_rnd_t* h, int which, float* padded_dev, void* stream);

/* Optimizer state that is not a vector: the step count (host side) and the learning rate (device scalar, set in stream order). */
int go2sim_rnd_set_step(go2sim_rnd_t* h, long long step, double learning_rate, void* stream);
int go2sim_rnd_reset_stats(go2sim_rnd_t* h, void* stream);
/* out_dev: GO2SIM_RND_N_STATS float64 on the device, written in stream order */
int go2sim_rnd_stats(go2sim_rnd_t* h, double* out_dev, void* stream);

/* The reward normaliser's state: mean, var, std as float32 and count as int64 in host memory, avg [n_avg] float32 in host memory (n_avg <= max_rows;
 * get: the first n_avg entries, set: those entries, the others become 0).  Initial state: mean 0, var 1, std 1, count 0, avg 0.  Bit-exact both ways.
 * Both wait for the stream. */
int go2sim_rnd_get_reward_state(go2sim_rnd_t* h, float* mean, float* var, float* std, int64_t* count, float* avg, int n_avg, void* stream);
int go2sim_rnd_set_reward_state(go2sim_rnd_t* h, float mean, float var, float std, int64_t count, const float* avg, int n_avg, void* stream);

#ifdef __cplusplus
}
#endif
#endif
