/* go2sim_rnn.h -- C ABI of the recurrent (LSTM) actor-critic: the memory cell next to the policy step (include/go2sim_policy.h) and the
 * backpropagation-through-time form of the PPO update (include/go2sim_train.h).  It replaces `rsl_rl.modules.ActorCriticRecurrent`
 * (rsl-rl-lib==2.2.4, rnn_type "lstm", one layer) and the recurrent mini-batch generator of `rsl_rl.storage.RolloutStorage` as `PPO.update`
 * uses it.  rsl_rl is a third-party package that is not part of the reference tree; the law is stated here.
 *
 * Conventions follow go2sim_train.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the
 * given stream, no call below synchronises with the host unless it says so.  There is no CPU twin: the checker is torch float64
 * (nn.LSTM + autograd, tests/ppo_rnn_ref.py).
 *
 * The law.  Two memories, memory_a = LSTM(num_actor_obs -> H) and memory_c = LSTM(num_critic_obs -> H); the actor MLP reads h_a, the critic
 * MLP reads h_c (both have first width H).  One cell step, gates in torch's order i, f, g, o:
 *   z = W_ih x + b_ih + W_hh h + b_hh          W_ih [4H][I], W_hh [4H][H], two separate bias vectors [4H]
 *   i, f, o = sigmoid(z_i), sigmoid(z_f), sigmoid(z_o);  g = tanh(z_g)
 *   c' = f c + i g;   h' = o tanh(c')
 * State-dict keys beside actor.*, critic.*, std:  memory_{a,c}.rnn.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}; initial values
 * uniform(-1/sqrt(H), 1/sqrt(H)) as nn.LSTM draws them.  b_ih and b_hh are two parameters: equal gradients, their own Adam moments.
 *
 * Collection: act(obs) steps memory_a, evaluate(critic_obs) steps memory_c, reset(dones) zeroes h and c of the done envs after every env
 * step.  PPO.compute_returns evaluates the last critic observation and so advances memory_c once more, as rsl_rl does.  At the rollout's
 * first act the four state arrays (h_a, c_a, h_c, c_c), [B][H] each, are saved: with dones [T][B] they are all the update needs.
 *
 * Update: no shuffle.  Mini-batch m of every epoch is the env block [m B / nmb, (m + 1) B / nmb) with all T steps.  The cell runs over the
 * fixed [T][block] grid from the saved state, with h, c <- 0 entering step t + 1 wherever dones[t] is set (this equals rsl_rl's
 * split-and-pad of trajectories: within 1e-15 in float64 against nn.LSTM run over the pieces).  Every loss is a mean over all T x block rows; losses, KL rule, clip and
 * Adam are those of go2sim_train.h; the global gradient norm runs over MLP, LSTM and std parameters together.
 *
 * Launches of one recurrent mini-batch (csrc/go2sim_lstm_dev.h, csrc/go2sim_train.hip):
 *   T x k_lstm_cell      both memories per launch.  A workgroup owns 32 rows and 4 x 16 hidden units, a wavefront one 16-unit column tile with
 *                        its four gate accumulators per row tile: [x | h] . [W_ih | W_hh]^T on v_mfma_f32_16x16x4_f32, the gates from dm_exp
 *                        (include/go2sim_detmath.h) on the accumulators.  The training forward keeps i, f, g, o, the masked c and h entering
 *                        the step, c' and h' per step.
 *   k_train_forward, k_ppo_head, k_ppo_finalize as in go2sim_train.h on the T x block rows of h' (row t block + j is batch row t B + e0 + j)
 *   the MLP backward as in go2sim_train.h; the first layer also writes d loss / d h (k_bwd_da without the ELU factor)
 *   T x k_lstm_bptt      t = T-1 .. 0, both memories per launch: dh = dh_mlp[t] + dz[t+1] W_hh (matrix instruction), dc = dc_carried +
 *                        dh o (1 - tanh^2 c'), both carried terms zero where dones[t] cut the sequence; writes dz[t] [block][4 Hpad] and the
 *                        carried dc f.  The gradient into the saved initial state is discarded.
 *   k_bwd_dw / k_bwd_db  dW_ih = sum dz^T x, dW_hh = sum dz^T h_prev (the masked h entering the step), db_ih = db_hh = sum dz over all T x
 *                        block rows: the 512-row chunk partials and their float64 fixed-order reduction of go2sim_train.h.
 * Numerics as in go2sim_train.h: fp32 fma chains on the matrix instruction, float64 for every sum over chunks and workgroups, no
 * floating-point atomics, every sum in a fixed order: equal inputs give equal bits.  Widths are padded to 16 with zeros; padded entries of
 * the gates' derivatives and of every gradient are exactly zero.  Bounds (tests/test_ppo_rnn_gpu.py), the forms of go2sim_policy.h and go2sim_train.h:
 *   cell step and T-step unroll:  max|y - y64| <= C_MLP max(max|y32 - y64|, 2^-24 max|y64|),  C_MLP = 7
 *   gradients per tensor (MLP, LSTM, std) with C_GRAD = 16, parameters after whole updates with C_UPD = 8.
 * Worst measured over tests/ppo_rnn_cases.py on the MI355X (H 16 .. 512, the further column groups of the two kernels included): 4.23 against C_MLP
 * (the critic memory's c after 2 steps of one env at H = 512, case h512-t2-n1-none; the worst h' is at 3.22, the actor memory of the same case; within
 * the first column group the worst stays 3.07, the actor memory's c after 8 steps of one env, H = 16, random dones; the product widths H = 256, I = 49 and
 * 104 are at 1.30, two memories of unequal H in one launch at 2.10); 4.25 against C_GRAD (the single entry of a one-layer critic's bias at T = 1 x 70 envs
 * -- a sum of 70 signed d loss / d v, the kind of entry go2sim_train.h records at 6.76), the worst tensor of a memory at 2.56 (memory_c's two biases,
 * H = 48, 8 steps x 17 envs; 1.68 at H = 68, 1.54 at H = 80, 1.41 at H = 256, 1.25 at H = 512); 2.65 against C_UPD (2 epochs x 2 mini-batches of 3 steps x
 * 17 envs, H = 20; 1.77 at H = 80, 2 steps x 17 envs, memory_c's bias_hh).  The LSTM tensors stay inside the project's constants: they have none of their own.
 *
 * Padded layout of the handle's vectors (gradients, Adam's m and v) with memories: actor | critic | memory_a | memory_c | std, a memory being
 * W_ih [4 Hpad][Ipad], W_hh [4 Hpad][Hpad], b_ih [4 Hpad], b_hh [4 Hpad] with gate q's unit j in row q Hpad + j.  Flat (state-dict) order of
 * go2sim_ppo_export / import: actor W0, b0, ..., critic W0, b0, ..., memory_a weight_ih, weight_hh, bias_ih, bias_hh, memory_c the same, std.
 * A handle without memories (go2sim_ppo_create) runs the launches of go2sim_train.h and keeps its layouts.
 */
#ifndef GO2SIM_RNN_H
#define GO2SIM_RNN_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim_train.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct go2sim_lstm go2sim_lstm_t;

/* One LSTM layer n_in -> n_hidden (both 1 .. GO2SIM_MLP_MAX_WIDTH).  `params` (host memory): weight_ih [4H][I], weight_hh [4H][H], bias_ih [4H],
 * bias_hh [4H], row-major, torch's gate order: n_params = 4 H (I + H + 2).  Waits for the device. */
int go2sim_lstm_create(int device, int n_in, int n_hidden, const float* params, size_t n_params, go2sim_lstm_t** out);
int go2sim_lstm_destroy(go2sim_lstm_t* h);
int go2sim_lstm_set_params(go2sim_lstm_t* h, const float* params, size_t n_params, void* stream);
/* the parameters as they are on the device, in the order of go2sim_lstm_create, to host memory; waits for the stream */
int go2sim_lstm_get_params(go2sim_lstm_t* h, float* params, size_t n_params, void* stream);

/* One cell step of one or two memories in one launch (mem_c and its arrays may all be NULL).  Per memory: x [n_rows][I], h_in, c_in, h_out, c_out
 * [n_rows][H], row-major device arrays.  h_out must not alias h_in (every workgroup reads whole rows of h_in); c_out may be c_in.
 * reset (u8 [n_rows], may be NULL): rows with a non-zero entry take h = c = 0 as the state entering the step. */
int go2sim_lstm_step(go2sim_lstm_t* mem_a, const float* x_a, const float* h_in_a, const float* c_in_a, float* h_out_a, float* c_out_a,
                     go2sim_lstm_t* mem_c, const float* x_c, const float* h_in_c, const float* c_in_c, float* h_out_c, float* c_out_c,
                     const uint8_t* reset, int n_rows, void* stream);

/* The saved state of the rollout's first act and the rollout's dones (device pointers). */
typedef struct go2sim_ppo_rnn_state {
  const float* h_a;       /* [B][H] */
  const float* c_a;
  const float* h_c;
  const float* c_c;
  const uint8_t* dones;   /* [T][B] */
} go2sim_ppo_rnn_state_t;

/* go2sim_ppo_create with the two memories in front of the two MLPs (whose first width must be the memories' H).  The handle's vectors grow by the
 * memories' segments (layout above); the optimizer writes the arrays go2sim_lstm_step reads.  Workspaces are sized for n_steps x
 * max_envs_per_minibatch rows.  Sharded records (go2sim_ppo_shard_*), go2sim_ppo_minibatch_grad, go2sim_ppo_update and go2sim_ppo_set_mirror refuse such a
 * handle (GO2SIM_E_BADARG). */
int go2sim_ppo_create_recurrent(go2sim_mlp_t* actor, go2sim_mlp_t* critic, go2sim_lstm_t* mem_a, go2sim_lstm_t* mem_c, int n_actions,
                                const go2sim_ppo_cfg_t* cfg, int n_steps, int max_envs_per_minibatch, go2sim_ppo_t** out);
/* Forward, loss head and backward through time of the env block [env0, env0 + n_block) of a rollout of n_steps x n_envs rows (batch arrays
 * [n_steps * n_envs] rows, row t * n_envs + e).  Leaves the gradients on the device, applies the learning-rate rule and adds the mini-batch to the
 * running sums, as go2sim_ppo_minibatch_grad does. */
int go2sim_ppo_rnn_minibatch_grad(go2sim_ppo_t* h, const go2sim_ppo_batch_t* batch, const go2sim_ppo_rnn_state_t* state, const float* std_dev,
                                  int n_envs, int env0, int n_block, void* stream);
/* The whole update: resets the running sums, then for every epoch and mini-batch m the call above on the env block [m n_envs / n_mini_batches,
 * (m + 1) n_envs / n_mini_batches) followed by go2sim_ppo_apply.  n_envs must be a multiple of n_mini_batches. */
int go2sim_ppo_rnn_update(go2sim_ppo_t* h, const go2sim_ppo_batch_t* batch, const go2sim_ppo_rnn_state_t* state, float* std_dev, int n_envs,
                          int n_epochs, int n_mini_batches, void* stream);

#ifdef __cplusplus
}
#endif
#endif
