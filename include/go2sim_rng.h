/* go2sim_rng.h -- the purposes of the library's one random stream.
 *
 * Every random number of the product build is a word of Philox4x32-10 (include/go2sim_detmath.h, dm_philox):
 *
 *     dm_philox(c0 = env word, c1 = key, c2 = purpose, c3 = block; k0 = low word of the seed, k1 = high word)  ->  four words w0..w3
 *
 * A PURPOSE names one stream; within it the env word, the key and the block number say which counter a draw takes, and the word index which of the
 * four words.  This header is the one list of the purposes: csrc/go2sim.hip, csrc/go2sim_mlp_dev.h and oracle/go2sim_cpu.cpp include it, the Python
 * side reads it into capi.C, and tests/env_rng_ref.py restates every line below as a table (STREAMS) that tests/test_env_rng_ref.py holds the
 * libraries to.  No two purposes may share a number: two streams with one number, one seed and one key draw the same words.
 *
 * Keys:  "step"        the handle's step count (go2sim_env_globals_t.step_count: env steps since go2sim_env_configure)
 *        "reset call"  the number of reset calls before this one (reset_calls: a reset call is one env_reset / env_reset_idx, or one env step in
 *                      which at least one env reset)
 *        "sync call"   the number of go2sim_env_sync_apply calls that drew before this one (sync_calls): the global DR with GO2SIM_IC_SHARED_GLOBALS
 * Transforms: rand_float(lo, hi, w) = f32(hi - lo) * u01(w) + f32(lo), u01(w) = (w >> 8) * 2^-24;  rand_int(lo, hi, w) = lo + w % (hi - lo + 1);
 *        normals: dm_normal2(w0, w1) and dm_normal2(w2, w3), two Box-Muller pairs per block.
 */
#ifndef GO2SIM_RNG_H
#define GO2SIM_RNG_H

/* Action noise (env_pre).  env word: env index.  key: step.  blocks 0..2: motors 4 blk .. 4 blk + 3 take the normals of (w0, w1), (w2, w3). */
#define GO2SIM_RNG_ACTION_NOISE 1

/* Push (env_pre, _apply_push).  env word: env index.  key: step.  block 0: w0 force x, w1 force y (rand_float), w2 duration in steps (rand_int). */
#define GO2SIM_RNG_PUSH 2

/* Command resampling inside an episode (env_post_a).  env word: env index.  key: step.  block 0: w0 x, w1 y, w2 yaw (rand_float); w3 the one axis
 * kept when commands are not compound (rand_int(0, 2)). */
#define GO2SIM_RNG_CMD 3

/* Observation noise (env_post_b).  env word: env index.  key: step.  block i / 4: observation i takes normal i % 4 of the block's two pairs. */
#define GO2SIM_RNG_OBS_NOISE 4

/* Per-env domain randomisation of a reset (env_reset_one).  env word: env index.  key: reset call.  blocks 0..2: kp factors 4 blk + w;  3..5: kd
 * factors;  6: w0..w2 gravity offset;  7..9: motor strength;  10: w0 per-env friction, w1 per-env base mass (GO2SIM_IC_PER_ENV_GLOBAL_DR).  All
 * rand_float. */
#define GO2SIM_RNG_RESET_DR 5

/* Global domain randomisation (globals_draws).  env word: 0xffffffff.  key: reset call, or sync call when the globals are shared.  block 0: w0 the
 * mix decision of sample_level (u01 < mix_prob_current), w1 the mixed level, w2 friction, w3 base mass;  block 1: w0..w2 COM shift;  block 2:
 * w0..w3 leg masses. */
#define GO2SIM_RNG_GLOBAL_DR 6

/* Commands of a reset (env_reset_one).  env word: env index.  key: reset call.  block 0: as GO2SIM_RNG_CMD. */
#define GO2SIM_RNG_RESET_CMD 7

/* Pose and delay of a reset (env_reset_one).  env word: env index.  key: reset call.  block 0: w0 init z, w1 roll, w2 pitch (rand_float), w3
 * delay steps (rand_int).  The stairwell spawn reads w1 and w2 again for the same roll and pitch (include/go2sim_wells.h). */
#define GO2SIM_RNG_RESET_POSE 8

/* Terrain row of a reset env (assign_terrain_rows).  env word: the env's rank p in the shuffle (not its index).  key: reset call.  block 0: w0 the
 * row of a "near" env, w1 the row of an "easy" env (rand_int); a frontier env draws nothing. */
#define GO2SIM_RNG_TERRAIN_ROW 9

/* Shuffle of the reset envs (assign_terrain_rows).  env word: env index.  key: reset call.  block 0: w0 the sort key; the rank of an env is the
 * number of reset envs with a smaller key, ties by env index. */
#define GO2SIM_RNG_TERRAIN_PERM 10

/* Action noise of the policy step (include/go2sim_policy.h; csrc/go2sim_mlp_dev.h).  env word: row.  key: the policy's step.  block a / 4: action
 * a takes normal a % 4.  Not an env stream; listed here because it shares the seed with the env in every training run. */
#define GO2SIM_RNG_POLICY_NOISE 11

/* 12: GO2SIM_LIDAR_RNG_PURPOSE (include/go2sim_lidar.h)         13: GO2SIM_STAIRINFO_RNG_PURPOSE (include/go2sim_stairinfo.h)
 * 14: GO2SIM_TILES_RNG_PURPOSE (include/go2sim_tiles.h)         15: GO2SIM_WELLS_RNG_PURPOSE (include/go2sim_wells.h) */

/* Per-env gains with per-leg stiffness off (env_reset_one, _randomize_kp_kd).  env word: env index.  key: reset call.  block 0: w0 kp_val, w1
 * kd_val (rand_float).  Product library only.  (It was 11 until it was found to draw the policy noise's words.) */
#define GO2SIM_RNG_RESET_KPKD 16

#endif
