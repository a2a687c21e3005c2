/* go2sim_evalstats.h -- C ABI and law of the EVALUATION STATISTICS: what a trained policy does with its commands, per env and per bin of envs, kept on
 * the device by one launch after the env step's own.  The reference answers the question with its keyboard teleop scripts (examples/locomotion/
 * go2_eval_*.py), which need a viewer; here 4096 envs evaluate 4096 command / terrain cells at once and the bookkeeping is a law, so that two
 * evaluations of one checkpoint give the same bits.
 *
 * Conventions follow go2sim_cterms.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call below synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is the numpy float64
 * restatement tests/evalstats_ref.py.
 *
 * ---- The records ----
 * Every env b has two records of the same shape: `run`, the episode in progress, and `tot`, the sum of its closed episodes.  A record is
 * GO2SIM_ES_M float64 values (SoA [GO2SIM_ES_M][n_envs]) and GO2SIM_EI_K int32 counters (SoA [GO2SIM_EI_K][n_envs]):
 *   float64   ES_N  ES_LIN_ERR2  ES_YAW_ERR2  ES_VX  ES_VY  ES_WZ  ES_ABS_POWER  ES_TORQUE2  ES_TILT2  ES_SPEED      the GO2SIM_ES_NSUMS sums
 *             ES_PEAK_TORQUE  ES_PEAK_DOF_VEL  ES_PEAK_FOOT_FORCE                                                   the running maxima
 *   int32     EI_EPISODES  EI_FALLS  EI_LENGTH_STEPS  EI_OVER_TORQUE  EI_OVER_DOF_VEL
 * In `run`, EI_LENGTH_STEPS counts the calls since the episode began (settle steps included) and EI_EPISODES / EI_FALLS stay 0.  Everything starts at 0.
 *
 * ---- The law of one call (go2sim_evalstats_step), per env b ----
 * Inputs, float32: commands c = (cx, cy, cyaw), base linear velocity v = (vx, vy, vz) in the body frame, base angular velocity w = (wx, wy, wz),
 * projected gravity g = (gx, gy, gz), dof velocity qd_j and torque tau_j for j = 0 .. 11, the links' net contact forces F_l (go2sim_cterms.h's
 * numbering: link 0 is the ground, bit l of foot_mask selects link l); reset uint8; time_out float32.
 *
 *   tot.EI_EPISODES[b] >= max_episodes:  nothing is read of the inputs and nothing is written -- the env contributed its first max_episodes episodes.
 *
 *   otherwise, reset[b] == 0 -- A STEP OF THE EPISODE.  With k = run.EI_LENGTH_STEPS[b]:  run.EI_LENGTH_STEPS[b] = k + 1, and if k >= settle_steps
 *   THE SAMPLE is taken.  Every input is widened to float64 first (exact); `+`, `*` are IEEE float64 operations in the written order, no
 *   contraction; |x| clears the sign bit:
 *     ES_N         += 1
 *     ES_LIN_ERR2  += (cx - vx) (cx - vx) + (cy - vy) (cy - vy)            two differences, two products, one sum, then the add to the record
 *     ES_YAW_ERR2  += (cyaw - wz) (cyaw - wz)
 *     ES_VX += vx;  ES_VY += vy;  ES_WZ += wz
 *     ES_ABS_POWER += P,  P = (..((0 + |tau_0 qd_0|) + |tau_1 qd_1|) + ..) + |tau_11 qd_11|          j ascending
 *     ES_TORQUE2   += T,  T = (..((0 + tau_0 tau_0) + tau_1 tau_1) + ..) + tau_11 tau_11
 *     ES_TILT2     += gx gx + gy gy
 *     ES_SPEED     += f64(s),  s = dm_sqrt(vx vx + vy vy) in FLOAT32 (two rounded products, one rounded sum, the correctly rounded root), as
 *                                  go2sim_cterms.h takes its norm
 *     maxima, by  m = (x > m) ? x : m  -- a NaN compares false and never enters:
 *       ES_PEAK_TORQUE over x = |tau_j|, ES_PEAK_DOF_VEL over x = |qd_j|, j ascending;
 *       ES_PEAK_FOOT_FORCE over x = f64(n_l), n_l = dm_sqrt((Fx Fx + Fy Fy) + Fz Fz) in float32, over the links l of foot_mask, ascending
 *     EI_OVER_TORQUE  += 1 if any |tau_j| > torque_limit;   EI_OVER_DOF_VEL += 1 if any |qd_j| > dof_vel_limit      (float64 compares; NaN: false)
 *   The sums propagate NaN and infinity as IEEE addition does.
 *
 *   otherwise, reset[b] != 0 -- THE EPISODE CLOSES.  The buffers hold the new episode's first state, so no sample is taken.  For every sum
 *   tot.x[b] = tot.x[b] + run.x[b];  for every maximum tot.m[b] = (run.m[b] > tot.m[b]) ? run.m[b] : tot.m[b];  tot.EI_OVER_* += run.EI_OVER_*;
 *   tot.EI_LENGTH_STEPS += run.EI_LENGTH_STEPS;  tot.EI_EPISODES += 1;  tot.EI_FALLS += (time_out[b] == 0) ? 1 : 0  (a NaN time_out: no fall);
 *   then run[b] := 0.  An episode that closes with ES_N == 0 (a reset on the first call, an episode shorter than settle_steps) still counts as an
 *   episode and as a fall or a time-out.
 *
 * settle_steps covers the spawn transient, and the one observation after a reset that still carries the command the reset drew, before the
 * evaluator writes its own (Go2Env.set_commands before every step).
 *
 * ---- The law of go2sim_evalstats_reduce ----
 * bins[b] in [0, n_bins) assigns every env to a bin (held by the handle: go2sim_evalstats_create / set_bins).  For bin k and every entry x of `tot`:
 *   lane i = 0 .. 255 forms  p_i = (..(0 (+) x[e_0]) (+) x[e_1]) ..  over the envs e = i, i + 256, i + 512, .. < n_envs ascending, an env of another bin
 *   contributing nothing (not even a + 0);  then for stride s = 128, 64, .. 1:  p_i = p_i (+) p_(i+s)  for i < s;  the bin's value is p_0.
 *   (+) is float64 addition for the sums, (b > a) ? b : a for the maxima (a the left operand), int64 addition for the counters.
 * The per-bin counters are GO2SIM_EBIN_K int64: the five EI_* totals, then EBIN_ENVS, the envs of the bin, and EBIN_COMPLETE, those of them with
 * EI_EPISODES >= max_episodes.  An empty bin gives zeros.
 *
 * CONSEQUENCES.  Equal inputs give equal bits on any stream and at any launch time: no LDS or atomics in the step, a fixed tree in the reduce, no
 * data-dependent trip counts.  The per-bin value depends on the assignment of envs to lanes, i.e. on n_envs and bins, which is why command_grid's
 * assignment (env b -> cell b mod n_cells) is part of the Python interface's contract.  The float64 sums are exact for the counts and lose at most
 * 2^-53 relative per addition elsewhere; only ES_SPEED and ES_PEAK_FOOT_FORCE carry float32 roundings (3 and 6 of them, as in go2sim_cterms.h).
 *
 * Safety.  The step reads, per env, component i of a view at p[i * comp_stride + b * env_stride] for i below the view's width (3, or 12 for
 * dof_vel and torque), component i of link l of foot_mask at cf[i * cf_comp_stride + l * cf_link_stride + b * cf_env_stride], reset[b] and
 * time_out[b], and nothing else of the caller's memory: the caller's strides and n_links bound the reads.  It writes the handle's records alone.
 *
 * Launches (csrc/go2sim_evalstats.hip): k_evalstats_step, one per step call: one lane per env, 256-lane workgroups; in the env pool's layout
 * (comp_stride = n_envs, env_stride = 1) every load is coalesced over the wavefront.  k_evalstats_reduce, one per reduce call: one 256-lane
 * workgroup per bin.  k_evalstats_clear, one per clear call.
 */
#ifndef GO2SIM_EVALSTATS_H
#define GO2SIM_EVALSTATS_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_EVALSTATS_LINKS_MAX 32 /* links foot_mask can name */
#define GO2SIM_EVALSTATS_NDOF 12      /* motor dofs: the width of dof_vel and torque */

/* float64 entries of a record */
#define GO2SIM_ES_N 0
#define GO2SIM_ES_LIN_ERR2 1
#define GO2SIM_ES_YAW_ERR2 2
#define GO2SIM_ES_VX 3
#define GO2SIM_ES_VY 4
#define GO2SIM_ES_WZ 5
#define GO2SIM_ES_ABS_POWER 6
#define GO2SIM_ES_TORQUE2 7
#define GO2SIM_ES_TILT2 8
#define GO2SIM_ES_SPEED 9
#define GO2SIM_ES_NSUMS 10 /* entries below this index are sums, the others maxima */
#define GO2SIM_ES_PEAK_TORQUE 10
#define GO2SIM_ES_PEAK_DOF_VEL 11
#define GO2SIM_ES_PEAK_FOOT_FORCE 12
#define GO2SIM_ES_M 13

/* int32 counters of a record */
#define GO2SIM_EI_EPISODES 0
#define GO2SIM_EI_FALLS 1
#define GO2SIM_EI_LENGTH_STEPS 2
#define GO2SIM_EI_OVER_TORQUE 3
#define GO2SIM_EI_OVER_DOF_VEL 4
#define GO2SIM_EI_K 5

/* int64 counters of a bin: the five above, then */
#define GO2SIM_EBIN_ENVS 5
#define GO2SIM_EBIN_COMPLETE 6
#define GO2SIM_EBIN_K 7

typedef struct go2sim_evalstats go2sim_evalstats_t;

typedef struct {
  double dt;                          /* the env step, > 0 (kept for the host's derived values; the launches do not use it) */
  double torque_limit, dof_vel_limit; /* N m, rad / s */
  int n_envs, n_bins;                 /* >= 1 each */
  int settle_steps, max_episodes;     /* >= 0, >= 1 */
  int n_links;                        /* in [1, 32] */
  uint32_t foot_mask;                 /* bit l: link l */
} go2sim_evalstats_cfg_t;

/* float32 device memory: component i of env b at p[i * comp_stride + b * env_stride] (elements) */
typedef struct {
  const float* p;
  long long comp_stride, env_stride;
} go2sim_evalstats_view_t;

/* the inputs of one step; the env pool's SoA buffers are (n_envs, 1) views (go2sim_env_buffer_dev), a row-major [n][k] tensor is (1, k); cf as
 * go2sim_cterms_step takes it: the pool's field is (n, 3 n, 1), a row-major [n][n_links][3] tensor (1, 3, 3 n_links) */
typedef struct {
  go2sim_evalstats_view_t commands, base_lin_vel, base_ang_vel, projected_gravity; /* 3 components each */
  go2sim_evalstats_view_t dof_vel, torque;                                         /* GO2SIM_EVALSTATS_NDOF components each */
  const float* cf;
  long long cf_comp_stride, cf_link_stride, cf_env_stride;
  const uint8_t* reset;  /* [n] */
  const float* time_out; /* [n] */
} go2sim_evalstats_in_t;

/* bins: int32 [n_envs], host memory, or NULL: every env in bin 0.  GO2SIM_E_BADARG: n_envs < 1, n_bins < 1, settle_steps < 0, max_episodes < 1,
 * n_links outside [1, 32], a mask bit at or above n_links, dt <= 0, a NaN constant, a bin outside [0, n_bins).  Waits for the device. */
int go2sim_evalstats_create(int device, const go2sim_evalstats_cfg_t* cfg, const int32_t* bins, go2sim_evalstats_t** out);
int go2sim_evalstats_destroy(go2sim_evalstats_t* h);

/* A new assignment of envs to bins (int32 [n_envs], host memory); the records stay.  GO2SIM_E_BADARG -- nothing changes -- for a bin outside
 * [0, n_bins).  Waits for the stream. */
int go2sim_evalstats_set_bins(go2sim_evalstats_t* h, const int32_t* bins, void* stream);

/* One step of all n == n_envs envs: one launch.  GO2SIM_E_BADARG -- nothing is launched -- for a NULL handle, `in` or member pointer of it,
 * n != n_envs and a negative stride. */
int go2sim_evalstats_step(go2sim_evalstats_t* h, int n, const go2sim_evalstats_in_t* in, void* stream);

/* run := 0 and tot := 0 for the n_sel envs of envs_idx (int32, device memory; entries outside [0, n_envs) are passed over) or for all envs when
 * envs_idx is NULL.  One launch. */
int go2sim_evalstats_clear(go2sim_evalstats_t* h, const int* envs_idx, int n_sel, void* stream);

/* The per-bin totals of `tot` by the law above, into the handle's own device memory (go2sim_evalstats_get_state reads them).  One launch. */
int go2sim_evalstats_reduce(go2sim_evalstats_t* h, void* stream);

/* Host memory, each array optional (NULL: not copied): run_f, tot_f float64 [GO2SIM_ES_M][n_envs]; run_i, tot_i int32 [GO2SIM_EI_K][n_envs];
 * bin_f float64 [n_bins][GO2SIM_ES_M] and bin_i int64 [n_bins][GO2SIM_EBIN_K] as the last go2sim_evalstats_reduce left them (zeros before the
 * first).  Waits for the stream. */
int go2sim_evalstats_get_state(go2sim_evalstats_t* h, double* run_f, int32_t* run_i, double* tot_f, int32_t* tot_i, double* bin_f, int64_t* bin_i,
                               void* stream);

/* device address of tot's EI_EPISODES row, int32 [n_envs]: the host loop tests (episodes >= max_episodes).all() on it without a per-step wait */
int go2sim_evalstats_episodes(go2sim_evalstats_t* h, const int32_t** episodes_dev);

/* Implemented by the env core (csrc/go2sim.hip; declared here because only the product library has it): the device address and the strides, in
 * elements, of the core's own env buffer `env_buf` (GO2SIM_EB_COMMANDS, BASE_LIN_VEL, BASE_ANG_VEL, PROJECTED_GRAVITY, DOF_VEL or TORQUE of
 * include/go2sim.h; any other: GO2SIM_E_BADARG), to be read in place after go2sim_env_step, the way go2sim_lidar_env_pose hands out the pose.
 * The links' contact forces come through go2sim_field_ptr(GO2SIM_F_CONTACT_FORCE). */
int go2sim_env_buffer_dev(go2sim_t* env, int env_buf, const float** ptr, long long* comp_stride, long long* env_stride);

#ifdef __cplusplus
}
#endif
#endif
