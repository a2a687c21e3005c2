/* go2sim_lidar.h -- C ABI of the LIDAR terrain scan of the reference's exteroceptive stair env (examples/locomotion/go2_env_stair_lidar.py:
 * LidarScanConfig :304, _get_terrain_height :883, _compute_lidar_scan :895, _update_actor_lidar_scan :939, _update_critic_lidar_scan :1004, the row
 * assembly :1615-1692, the reset lines :1777-1781).  The "LIDAR" is a heightfield lookup on a body-frame grid: a noisy, sparse scan for the actor (what
 * the robot's L1 delivers after projection) and a clean, dense one for the critic.
 *
 * Conventions follow go2sim_norm.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call below synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is numpy float64
 * (tests/lidar_ref.py), itself pinned to the reference's own methods (tests/golden/ref_lidar_scan.npz, tools/make_ref_lidar_fixtures.py).
 *
 * A handle holds on the device its own copy of the heightfield (float [rows][cols] = hf * vertical_scale; origin and horizontal scale as float32),
 * the two lists of body-frame sample points, and the STORED ACTOR SCAN float [n_envs][n_actor] (initially 0); on the host the constants, the seed
 * and the step counter (initially 0).
 *
 * The law.  Everything is float32 (IEEE operations in the written order, no contraction) unless it says float64.  For env b with base position p,
 * base quaternion (w, x, y, z) and sample point (lx, ly):
 *   yaw = dm_atan2(2 (w z + x y), 1 - 2 (y y + z z));   (s, c) = dm_sincos(yaw)                     once per env
 *   wx = p.x + c lx - s ly;   wy = p.y + s lx + c ly
 *   col = clamp(trunc((wx - origin_x) / h_scale), 0, rows - 1);   row = clamp(trunc((wy - origin_y) / h_scale), 0, cols - 1)
 *   raw = hf[col][row] - p.z
 * -- the expression order of the privileged height scan of the env kernel (csrc/go2sim.hip, `_compute_height_scan`), so that with clip out of reach
 * and scale 1 the critic scan on the same grid is that scan bit for bit.
 *   critic scan:  clamp(raw, -clip, clip) * scale
 *   actor scan:   with L the DR level (below); a step runs only if its parameter is > 0 and L > 0
 *     1. raw_k += (z_k * f32(height_noise_std)) * f32(L)                       every point k
 *     2. raw_k = 0                where u_k < f32(dropout_prob * L)            the product in float64
 *     3. raw_k += (z_b * f32(vertical_offset_std)) * f32(L)                    one draw per env: dropped cells read the offset
 *     4. raw_k = stored[b][k]     where u_lat < f32(latency_prob * L)          the whole row: last step's STORED scan, already clipped and scaled
 *     5. raw_k = 0                where u_black < f32(full_blackout_prob * L)  the whole row
 *     stored[b][k] = clamp(raw_k, -clip, clip) * scale                         a stale row is clipped and scaled a second time
 * An env whose reset flag is set gets zeros in both scans and its stored scan becomes 0 (reset_idx zeroes the buffers before the rows are built).
 *
 * DR level.  L = dr_level(curriculum_enabled ? *level : 1.0) in float64, evaluated on the device from the level pointer of the call:
 *   dr_schedule == 0: L = t;   else t < gate: L = phase1;   else L = phase1 + (1 - phase1) clamp01((t - gate) / max(1e-6, 1 - gate))
 * (_get_dr_level, go2_env_stair_lidar.py:1197-1220; the mapping of csrc/go2sim.hip `dr_level`).
 *
 * Random numbers.  Philox4x32-10 (include/go2sim_detmath.h) with counter (env, step, purpose 12, idx) and key (seed low word, seed high word);
 * purposes 1-11 belong to the env and the policy.  dm_u01 makes a uniform of a word, dm_normal2 two normals of two words.
 *   idx 0:       word 0 -> u_lat, word 1 -> u_black, words 2, 3 -> dm_normal2, whose first normal is z_b
 *   idx 1 + j:   words 0, 1 -> dm_normal2 -> z_{2j}, z_{2j+1};  words 2, 3 -> u_{2j}, u_{2j+1}            j = 0 .. ceil(n_actor / 2) - 1
 * `step` is the handle's own counter: the value it has when go2sim_lidar_step is called, which then increments it.
 *
 * Rows.  With inner rows obs [n][n_in] and priv [n][n_in + 56] (the env's observations; the privileged entries and the terrain row):
 *   obs_out  [n][n_in + n_actor]                    = obs | actor scan
 *   priv_out [n][n_in + n_actor + 56 + n_critic]    = priv[0 .. n_in) | actor scan | priv[n_in .. n_in + 56) | critic scan
 * Without inner rows (obs == priv == NULL, n_in == 0):  obs_out [n][n_actor] = actor scan,  priv_out [n][n_actor + n_critic] = actor | critic scan.
 *
 * Safety and determinism.  Both indices are clamped before the load by comparisons that a NaN fails: a pose of any finite value, an infinity or a NaN
 * cannot read outside the field.  A NaN in p.x, p.y or the quaternion selects index 0 on the axes it reaches and the scan stays finite; a NaN p.z
 * gives NaN scans (a dropped, stale or blacked-out cell and a reset env stay finite); the stored scan takes what the row takes.  No atomics, no LDS,
 * no data-dependent trip counts: the result is a function of (state, inputs, step) alone, equal calls give equal bits on any stream.
 *
 * Launch (csrc/go2sim_lidar.hip): k_lidar_step, one per call: one wavefront per env (4 per workgroup); every lane of the wavefront holds the env's
 * yaw, sine, cosine and env-level draws, the points are spread over the lanes (a loop for grids of more than 64 points), and consecutive lanes write
 * consecutive columns of the output rows.  The heightfield is read with plain global loads.
 */
#ifndef GO2SIM_LIDAR_H
#define GO2SIM_LIDAR_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_LIDAR_RNG_PURPOSE 12
#define GO2SIM_LIDAR_PRIV_EXTRA 56   /* the 55 privileged entries and the terrain row between the actor scan and the critic scan */

typedef struct go2sim_lidar go2sim_lidar_t;

typedef struct {
  double height_noise_std, dropout_prob, vertical_offset_std, latency_prob, full_blackout_prob;   /* env_cfg["lidar"]["noise"] */
  double height_clip, height_scale;
  double dr_phase1_level, dr_terrain_gate;                                                         /* env_cfg["dr_schedule"] */
  double origin_x, origin_y, horizontal_scale, vertical_scale;                                     /* the terrain's placement */
  int dr_schedule, curriculum_enabled;
  int n_envs, n_actor, n_critic, hf_rows, hf_cols;
} go2sim_lidar_cfg_t;

/* hf: int16 [hf_rows][hf_cols] (rows along x), actor_xy: float32 [2][n_actor] (all x, then all y), critic_xy likewise; host memory, copied.
 * GO2SIM_E_BADARG: n_envs < 1, n_actor < 0, n_critic < 0, n_actor + n_critic == 0, a field of fewer than 1 x 1 cells, horizontal_scale <= 0,
 * height_clip < 0 or a NaN constant.  Waits for the device. */
int go2sim_lidar_create(int device, const go2sim_lidar_cfg_t* cfg, const int16_t* hf, const float* actor_xy, const float* critic_xy, uint64_t seed,
                        go2sim_lidar_t** out);
int go2sim_lidar_destroy(go2sim_lidar_t* h);
/* the step counter (host side, no device work) */
int go2sim_lidar_get_step(go2sim_lidar_t* h, uint32_t* step);
int go2sim_lidar_set_step(go2sim_lidar_t* h, uint32_t step);
/* stored actor scan := 0 for the n_sel envs of envs_idx (int32, device memory; entries outside [0, n_envs) are passed over), or for all envs when
 * envs_idx is NULL.  One launch. */
int go2sim_lidar_clear(go2sim_lidar_t* h, const int* envs_idx, int n_sel, void* stream);
/* the stored actor scan float32 [n_envs][n_actor], host memory; bit-exact both ways.  Both wait for the stream. */
int go2sim_lidar_get_scan(go2sim_lidar_t* h, float* scan, void* stream);
int go2sim_lidar_set_scan(go2sim_lidar_t* h, const float* scan, void* stream);

/* One scan step of all n == n_envs envs: one launch.  Component i of env b's position is pos[i * pos_comp_stride + b * pos_env_stride] (3
 * components), of its quaternion quat[i * quat_comp_stride + b * quat_env_stride] (w, x, y, z): [n][3] rows have strides (1, 3), the env's own
 * [3][n] field has (n, 1).  reset: uint8 [n] or NULL (no env was reset).  level: the curriculum level (double, device memory); may be NULL when
 * curriculum_enabled == 0.  obs, priv, n_in and the outputs: "Rows" above.
 * GO2SIM_E_BADARG -- nothing is launched, the step counter stays -- for a NULL handle, n != n_envs, a NULL pos, quat, obs_out or priv_out, a NULL
 * level with the curriculum enabled, n_in < 0, inner rows of which exactly one is NULL or that disagree with n_in (NULL with n_in > 0, given with
 * n_in == 0), and an output that is one of the inner rows or the other output. */
int go2sim_lidar_step(go2sim_lidar_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                      long long quat_comp_stride, long long quat_env_stride, const uint8_t* reset, const double* level, const float* obs,
                      const float* priv, int n_in, float* obs_out, float* priv_out, void* stream);

/* The base pose buffers of an env handle as the step kernels leave them (csrc/go2sim.hip): float32 [3][n_envs] and [4][n_envs], i.e. component
 * stride n_envs and env stride 1, for go2sim_lidar_step to read in place. */
int go2sim_lidar_env_pose(go2sim_t* env, const float** pos, const float** quat, long long* comp_stride);

#ifdef __cplusplus
}
#endif
#endif
