/* go2sim_stairinfo.h -- C ABI of the four-value stair info of the reference's later exteroceptive stair env (examples/locomotion/
 * go2_env_stair_lidar_2.py: StairInfoConfig :331, _get_terrain_height :836, _compute_edge_detection :848, _update_stair_info :908, the row assembly
 * :1561 / :1623, the reset lines :1705-1707).  Instead of a terrain grid the actor gets what a real Go2 can deliver:
 *   [0] distance to the next height change along the body's forward axis (0 .. max_range; max_range = none in range)      edge detector on the L1
 *   [1] riser height and [2] tread depth of the stairs the robot is on                                                     measured by the user
 *   [3] direction: +1 up, -1 down, 0 none                                                                                   edge detector
 * In simulation [0] and [3] come from the heightfield, [1] and [2] from two per-row tables indexed by the env's current terrain row.  Only the
 * actor's copy is degraded (noise, direction flips, stale data, blackouts, scaled by the DR level); the critic gets the clean four.
 *
 * Conventions follow go2sim_lidar.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call below synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is numpy float64
 * (tests/stairinfo_ref.py), itself pinned to the reference's own methods (tests/golden/ref_stair_info.npz, tools/make_ref_stairinfo_fixtures.py).
 *
 * A handle holds on the device its own copy of the heightfield (float [rows][cols] = float32(hf) * float32(vertical_scale); origin and horizontal
 * scale as float32), the samples x_k (float32 [n_samples]: the float32 torch.linspace(0, max_range, n_samples) the host hands over), the two per-row
 * tables (float32 [n_rows] each) and the STORED ACTOR ROW float [n_envs][4] (initially 0); on the host the constants, the seed and the step counter
 * (initially 0).
 *
 * The law.  Everything is float32 (IEEE operations in the written order, no contraction) unless it says float64.  For env b with base position p,
 * base quaternion (w, x, y, z) and terrain row r (clamped to [0, n_rows - 1]):
 *   yaw = dm_atan2(2 (w z + x y), 1 - 2 (y y + z z));   (s, c) = dm_sincos(yaw)                     once per env, as in go2sim_lidar.h
 *   wx_k = p.x + c x_k;   wy_k = p.y + s x_k                                                         the centre line only
 *   col = clamp(trunc((wx_k - origin_x) / h_scale), 0, rows - 1);   row = clamp(trunc((wy_k - origin_y) / h_scale), 0, cols - 1)
 *   h_k = hf[col][row]                                                                               absolute, not relative to the base
 *   dh_k = h_{k+1} - h_k                                                                             k = 0 .. n_samples - 2
 *   an edge is the first k with |dh_k| > f32(threshold):   edge = (x_k + x_{k+1}) / 2,  dir = sign(dh_k);   none:  edge = f32(max_range),  dir = 0
 *   height = row_heights[r];   depth = row_depths[r]
 * A riser that equals the threshold is decided by the float32 values h_k = f32(units * f32(v_scale)): with 4 units of 0.005 m the first step is
 * 4 f32(0.005) = f32(0.02), not greater, no edge; higher steps of the same flight differ by the roundings of both heights and fall on either side.
 *   clean four:  edge s_e,  height s_h,  depth s_d,  dir s_dir                                      the four scales as float32
 *   actor four:  with L the DR level (below); a step runs only if its parameter is > 0 and L > 0
 *     1. edge += (z_e * f32(edge_noise_std)) * f32(L);   edge = clamp(edge, 0, f32(max_range))      the clamp belongs to this step
 *     2. height += (z_h * f32(height_noise_std)) * f32(L)
 *     3. depth += (z_d * f32(depth_noise_std)) * f32(L)
 *     4. dir = -dir                  where u_flip < f32(direction_flip_prob * L)                     the product in float64
 *     5. edge = stored[b][0] / s_e;  dir = stored[b][3] / s_dir      where u_lat < f32(latency_prob * L)
 *        -- last step's STORED actor row, divided by the scale it was stored with and multiplied by it again in step 7: a divide followed by a
 *        multiply, not the identity (with s_e = 3.7 a stale edge can move by an ulp).  A scale of 0 gives what IEEE gives (0 / 0).
 *     6. edge = f32(max_range);  dir = 0     where u_black < f32(full_blackout_prob * L)
 *     7. stored[b] = (edge s_e, height s_h, depth s_d, dir s_dir)
 *   Height and depth are never stale or blacked out.
 * An env whose reset flag is set gets zeros in both fours and its stored row becomes 0 (reset_idx zeroes the three buffers after the update).
 *
 * DR level.  L = dr_level(curriculum_enabled ? *level : 1.0) in float64, evaluated on the device from the level pointer of the call: the two-phase
 * mapping of go2sim_lidar.h (`_get_dr_level`; `_stair_noise_level` of go2_env_stair_lidar_2.py:1188).
 *
 * Random numbers.  Philox4x32-10 (include/go2sim_detmath.h) with counter (env, step, purpose 13, idx) and key (seed low word, seed high word);
 * purposes 1-12 belong to the env, the policy and the LIDAR scan.  dm_u01 makes a uniform of a word, dm_normal2 two normals of two words.
 *   idx 0:   words 0, 1 -> dm_normal2 -> z_e, z_h;   words 2, 3 -> dm_normal2, whose first normal is z_d
 *   idx 1:   word 0 -> u_flip,  word 1 -> u_lat,  word 2 -> u_black                                  (word 3 is not used)
 * `step` is the handle's own counter: the value it has when go2sim_stairinfo_step is called, which then increments it.
 *
 * Rows.  With inner rows obs [n][n_in] and priv [n][n_in + 56] (the env's observations; the 55 privileged entries and the terrain row):
 *   obs_out  [n][n_in + 4]             = obs | actor four
 *   priv_out [n][n_in + 4 + 56 + 4]    = priv[0 .. n_in) | actor four | priv[n_in .. n_in + 56) | clean four
 * Without inner rows (obs == priv == NULL, n_in == 0):  obs_out [n][4] = actor four,  priv_out [n][8] = actor four | clean four.
 *
 * Safety and determinism.  Both indices are clamped before the load by comparisons that a NaN fails, and the terrain row is clamped before the
 * table loads: a pose of any finite value, an infinity or a NaN cannot read outside the field.  Heights are field values, so all eight outputs
 * stay finite whatever the pose.  No atomics, no LDS, no data-dependent trip counts: the result is a function of (state, inputs, step) alone,
 * equal calls give equal bits on any stream.
 *
 * Launch (csrc/go2sim_stairinfo.hip): k_stairinfo_step, one per call: one wavefront per env (4 per workgroup).  Lane k owns the neighbouring
 * samples (k, k + 1) and looks both heights up itself; the first edge is the lowest set bit of the wavefront's ballot of |dh_k| > threshold, its
 * direction the same bit of the ballot of dh_k > 0 -- no loop over samples, no cross-lane data but the two masks.  Lane j < 4 owns entry j of the
 * stored row; consecutive lanes write consecutive columns of the rows.  A wavefront per env, not a 16-lane group: the ballot is the 64-lane mask the
 * hardware forms in one instruction, up to 63 pairs need no loop, and the 53 + 113 copied columns leave as 64-lane rows of consecutive floats.
 */
#ifndef GO2SIM_STAIRINFO_H
#define GO2SIM_STAIRINFO_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_STAIRINFO_RNG_PURPOSE 13
#define GO2SIM_STAIRINFO_N 4             /* edge distance, riser height, tread depth, direction */
#define GO2SIM_STAIRINFO_PRIV_EXTRA 56   /* the 55 privileged entries and the terrain row between the actor four and the clean four */
#define GO2SIM_STAIRINFO_MAX_SAMPLES 64
#define GO2SIM_STAIRINFO_MAX_ROWS 16

typedef struct go2sim_stairinfo go2sim_stairinfo_t;

typedef struct {
  double max_range, threshold;                                                                      /* env_cfg["stair_info"]["edge_detection"] */
  double edge_dist_scale, height_scale, depth_scale, direction_scale;
  double edge_noise_std, height_noise_std, depth_noise_std, direction_flip_prob, latency_prob, full_blackout_prob;   /* ["noise"] */
  double dr_phase1_level, dr_terrain_gate;                                                          /* env_cfg["dr_schedule"] */
  double origin_x, origin_y, horizontal_scale, vertical_scale;                                      /* the terrain's placement */
  int dr_schedule, curriculum_enabled;
  int n_envs, n_samples, n_rows, hf_rows, hf_cols;
} go2sim_stairinfo_cfg_t;

/* hf: int16 [hf_rows][hf_cols] (rows along x), sample_x: float32 [n_samples], row_heights and row_depths: float32 [n_rows]; host memory, copied.
 * GO2SIM_E_BADARG: n_envs < 1, n_samples < 2 or > 64, n_rows < 1 or > 16, a field of fewer than 1 x 1 cells, horizontal_scale <= 0, max_range or
 * threshold negative or not finite, any other constant a NaN, a NULL array.  Waits for the device. */
int go2sim_stairinfo_create(int device, const go2sim_stairinfo_cfg_t* cfg, const int16_t* hf, const float* sample_x, const float* row_heights,
                            const float* row_depths, uint64_t seed, go2sim_stairinfo_t** out);
int go2sim_stairinfo_destroy(go2sim_stairinfo_t* h);
/* the step counter (host side, no device work) */
int go2sim_stairinfo_get_step(go2sim_stairinfo_t* h, uint32_t* step);
int go2sim_stairinfo_set_step(go2sim_stairinfo_t* h, uint32_t step);
/* stored actor row := 0 for the n_sel envs of envs_idx (int32, device memory; entries outside [0, n_envs) are passed over), or for all envs when
 * envs_idx is NULL.  One launch. */
int go2sim_stairinfo_clear(go2sim_stairinfo_t* h, const int* envs_idx, int n_sel, void* stream);
/* the stored actor rows float32 [n_envs][4], host memory; bit-exact both ways.  Both wait for the stream. */
int go2sim_stairinfo_get_state(go2sim_stairinfo_t* h, float* rows4, void* stream);
int go2sim_stairinfo_set_state(go2sim_stairinfo_t* h, const float* rows4, void* stream);

/* One step of all n == n_envs envs: one launch.  Poses and their strides as in go2sim_lidar_step.  terrain_row: int32 [n], device memory, read at
 * step time (NULL: row 0 for every env; allowed only with n_rows == 1).  reset: uint8 [n] or NULL (no env was reset).  level: the curriculum level
 * (double, device memory); may be NULL when curriculum_enabled == 0.  obs, priv, n_in and the outputs: "Rows" above.
 * GO2SIM_E_BADARG -- nothing is launched, the step counter stays -- for a NULL handle, n != n_envs, a NULL pos, quat, obs_out or priv_out, a negative
 * stride, a NULL terrain_row with more than one row, a NULL level with the curriculum enabled, n_in < 0, inner rows of which exactly one is NULL or
 * that disagree with n_in (NULL with n_in > 0, given with n_in == 0), and an output that is one of the inner rows or the other output. */
int go2sim_stairinfo_step(go2sim_stairinfo_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                          long long quat_comp_stride, long long quat_env_stride, const int* terrain_row, const uint8_t* reset, const double* level,
                          const float* obs, const float* priv, int n_in, float* obs_out, float* priv_out, void* stream);

/* The terrain-row buffer of an env handle as the step kernels leave it (csrc/go2sim.hip): int32 [n_envs], for go2sim_stairinfo_step to read in
 * place; go2sim_env_set_terrain_rows and the row lock act on this buffer.  The pose buffers: go2sim_lidar_env_pose. */
int go2sim_stairinfo_env_rows(go2sim_t* env, const int** terrain_row);

#ifdef __cplusplus
}
#endif
#endif
