/* go2sim_wells.h -- C ABI and law of the stairwell env: the reference's omnidirectional stair env (examples/locomotion/go2_env_stair6_Omni.py:
 * build_stairwell_terrain :45, _get_terrain_height :712, _compute_height_scan :720, _assign_wells :739, _get_spawn_pos :769, the reset lines
 * :1308-1325, _reward_alive :1471).  It is the stair env on a grid of stairwells -- inverted square pyramids with stairs on all four sides, one per
 * difficulty level -- with a spawn at the bottom of the env's well, a yaw drawn at every reset, an 11 x 11 privileged height scan and an `alive`
 * reward term.
 *
 * Conventions follow go2sim_lidar.h: extern "C", int status (0 = ok, GO2SIM_E_*), device pointers are caller-owned, work is ordered on the given
 * stream, no call below synchronises with the host unless it says so.  Product library only: there is no CPU twin, the checker is the numpy
 * restatement tests/wells_ref.py, itself pinned to the reference's own methods (tests/golden/ref_wells.npz, tools/make_ref_stairwell_fixtures.py).
 *
 * Two parts: the WELL SPAWN, a mode of the env handle (GO2SIM_IC_WELL_SPAWN, csrc/go2sim.hip), and the SCAN HANDLE of this header, which owns the
 * height scan (the env runs with GO2SIM_IC_SCAN_N = 0 and the inner rows of the LIDAR layout) and the alive term.
 *
 * ---- The well spawn ----
 * GO2SIM_IC_WELL_SPAWN = 1 needs GO2SIM_IC_USE_TERRAIN and excludes GO2SIM_IC_TILE_MODE (go2sim_env_configure refuses otherwise).  The row-centre
 * table GO2SIM_FC_ROW_CENTER0 then holds the well centres (x, y, bottom_z) of at most 16 levels, and the "terrain row" of an env is its well level:
 * the row assignment (k_env_terrain_rows: the 40 / 30 / 30 split of _assign_wells), go2sim_env_set_terrain_rows and go2sim_env_lock_terrain_rows
 * are used as they are.  The core's reset (env_reset_one) puts a reset env on the centre of its well with yaw 0, as it puts a stair env on its row's
 * centre; k_env_well_spawn then moves it.  For every env whose reset flag is set it draws ONE Philox4x32-10 block (include/go2sim_detmath.h) with
 * counter (env, reset call, purpose 15, 0) and key (seed low word, seed high word); "reset call" is the number of reset calls before this one, the key
 * of every other draw of a reset (env_reset_one); purposes 1-14 belong to the env, the policy, the LIDAR scan, the stair info and the tiles:
 *   x   = f32(cx + (-0.3 + (0.3 - (-0.3)) f64(dm_u01(word0))))      float64: cx is the centre as configured (a host double), the bracket is
 *   y   = f32(cy + (-0.3 + (0.3 - (-0.3)) f64(dm_u01(word1))))      python's random.uniform(-0.3, 0.3); one rounding to float32 at the end
 *   yaw = rand_float(lo_rad, hi_rad, word2)                         gs_rand_float: f32(hi - lo) dm_u01(word2) + f32(lo), float32; init_euler_range only
 *   word3 is not used.
 * The 0.3 is a literal of the law.  z is the stair env's: (bottom_z + base_init_pos.z), with init_pos_z_range ((z + u) - init_z) + init_z from word 0
 * of the pose block; roll and pitch keep words 1 and 2 of the pose block, and every other draw of a reset keeps its words.  The kernel rewrites base
 * x and y, and with init_euler_range the base quaternion euler_to_quat_wxyz(roll, pitch, yaw) -- roll and pitch formed again from their words, in
 * env_reset_one's expressions -- and keeps (x, y, yaw) in the env's spawn record (GO2SIM_EB_SPAWN_POS); envs that are not reset keep theirs.
 * k_env_well_spawn, one lane per env, runs after the reset and before the kinematics of the reset envs are refreshed: in go2sim_env_reset /
 * go2sim_env_reset_idx between k_env_reset_tail and the kinematics launch; in the step's chain after k_env_post_b_team, followed by one kinematics
 * launch (k_fk_team) that, like the spawn, returns at once on a step without resets.  The observations of the reset step, which k_env_post_b_team has
 * written by then, do not read x, y or yaw: angular velocity and velocities are zero, gravity in the body frame is taken from the roll-pitch quaternion
 * (equal to the yawed one's up to rounding), and the scan is the wells launch's, which runs after.  The reset code inside k_env_post_b_team is left as
 * it is on purpose: with the spawn written into it, the walk env's step measured 0.4 % slower (DESIGN.md "Stairwell env").  On -DGO2SIM_RNG_CONST
 * builds the words come from the constant schedule like every other draw.  With the flag off a handle runs the launches it ran before.
 *
 * ---- The scan handle ----
 * It holds on the device its own copy of the heightfield (float [rows][cols] = f32(hf) * f32(vertical_scale); origin and cell size as float32), the
 * body-frame sample points (lx_i, ly_j) of an nx x ny grid, nx, ny <= 16, formed from the two axes the host hands over (the float32 values of
 * torch.linspace), point k = i * ny + j, a per-env float32 alive sum with its int32 step count (both initially 0) and a per-env float32 record of
 * the last finished episode's alive term; on the host the level count and inc = f32(alive_scale * dt) (the product in float64).
 *
 * The scan.  Everything is float32 (IEEE operations in the written order, no contraction).  For env b with base position p, quaternion (w, x, y, z):
 *   yaw = dm_atan2(2 (w z + x y), 1 - 2 (y y + z z));   (s, c) = dm_sincos(yaw)                     once per env
 *   wx = p.x + c lx_i - s ly_j;   wy = p.y + s lx_i + c ly_j
 *   col = clamp(trunc((wx - origin_x) / h_scale), 0, rows - 1);   row = clamp(trunc((wy - origin_y) / h_scale), 0, cols - 1)
 *   scan[k] = hf[col][row] - p.z
 * -- the privileged height scan of the env kernel (csrc/go2sim.hip, `_compute_height_scan`; the lookup law of go2sim_stairinfo.h), so that on a grid
 * the core can hold (at most 80 points) the values are the core's bit for bit, also for envs that were reset in the step (the pose is the one the
 * step leaves: a reset env is scanned at its spawn pose; nothing is zeroed).
 *
 * Rows.  With the inner privileged row priv [n][n_in + 56] (the env's observations, the 55 privileged entries, the terrain row, whose entry
 * n_in + 55 = well_level / max(1, n_levels - 1) the core writes):
 *   priv_out [n][n_in + 56 + nx ny] = priv | scan
 * Without it (priv == NULL, n_in == 0): priv_out [n][nx ny] = scan.  The actor row needs no copy: the core writes it where it is read.
 *
 * The alive term (_reward_alive: ones, times its scale and dt).  With rew != NULL, for every env b:
 *   rew[b] = rew[b] + inc;   alive_sum[b] = alive_sum[b] + inc;   alive_steps[b] += 1
 * and for an env whose reset flag is set, after that:
 *   alive_ep[b] = alive_sum[b] / (f32(max(alive_steps[b], 1)) * f32(dt));   alive_sum[b] = 0;   alive_steps[b] = 0
 * (reset_idx order: the sum is read for the episode statistics, then cleared).  extras["episode"]["rew_alive"] is the mean of alive_ep over the envs of
 * the last reset, as the core's terms are reported.  CONSEQUENCE: alive is added after the core's sum, whatever its place in reward_scales, while the
 * reference adds the terms in dictionary order (alive third in its train script).  With alive last in the dictionary the float32 sums agree to the
 * bit; otherwise they can differ in the last place.  The term lives here because the core's reward ids are pinned (GO2SIM_R_COUNT).
 *
 * Safety and determinism.  Both indices are clamped before the load by comparisons that a NaN fails: a pose of any finite value, an infinity or a NaN
 * cannot read outside the field.  A NaN in p.x, p.y or the quaternion selects index 0 on the axes it reaches and the scan stays finite; a NaN p.z
 * gives NaN scans.  No atomics, no LDS, no data-dependent trip counts: equal calls give equal bits on any stream.
 *
 * Launch (csrc/go2sim_wells.hip): k_wells_step, one per call: one wavefront per env (4 per workgroup).  Every lane of the wavefront holds the env's
 * pose, yaw, sine and cosine.  Lane t owns the columns t, t + 64, t + 128, ... of the output row: a column below n_in + 56 is a copy of the inner
 * row, column n_in + 56 + k is point k.  So consecutive lanes write consecutive floats, and the 226-wide training row (105 copied columns, 121
 * points) leaves as three whole 64-lane rows and one of 34; only the row that holds column 105 mixes copies and points.  Lane 0 runs the alive term.
 * The heightfield is read with plain global loads.
 */
#ifndef GO2SIM_WELLS_H
#define GO2SIM_WELLS_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_WELLS_RNG_PURPOSE 15
#define GO2SIM_WELLS_PRIV_EXTRA 56    /* the 55 privileged entries and the terrain row between the observations and the scan */
#define GO2SIM_WELLS_AXIS_MAX 16      /* points per axis of the scan grid */
#define GO2SIM_WELLS_LEVELS_MAX 16    /* well levels: the length of the env's row-centre table */
#define GO2SIM_WELLS_SPAWN_JITTER 0.3 /* half-width of the spawn offset in x and in y, metres: a literal of _get_spawn_pos */

typedef struct go2sim_wells go2sim_wells_t;

typedef struct {
  double origin_x, origin_y, horizontal_scale, vertical_scale;   /* the terrain's placement */
  double alive_scale, dt;                                        /* reward_scales["alive"] (0: no alive term) and the env step */
  int n_envs, nx, ny, hf_rows, hf_cols, n_levels;
} go2sim_wells_cfg_t;

/* hf: int16 [hf_rows][hf_cols] (rows along x), xs: float32 [nx], ys: float32 [ny]; host memory, copied.
 * GO2SIM_E_BADARG: n_envs < 1, nx or ny outside [1, 16], n_levels outside [1, 16], a field of fewer than 1 x 1 cells, horizontal_scale <= 0,
 * dt <= 0 or a NaN constant.  Waits for the device. */
int go2sim_wells_create(int device, const go2sim_wells_cfg_t* cfg, const int16_t* hf, const float* xs, const float* ys, go2sim_wells_t** out);
int go2sim_wells_destroy(go2sim_wells_t* h);

/* The episode hand-over of the law above without a step, for the n_sel envs of envs_idx (int32, device memory; entries outside [0, n_envs) are passed
 * over) or for all envs when envs_idx is NULL: alive_ep := the per-second value, alive sum and step count := 0 (Go2Env.reset / reset_idx).  One launch. */
int go2sim_wells_clear(go2sim_wells_t* h, const int* envs_idx, int n_sel, void* stream);
/* alive sum float32 [n_envs] and step count int32 [n_envs], host memory; bit-exact both ways.  Both wait for the stream. */
int go2sim_wells_get_alive(go2sim_wells_t* h, float* sum, int32_t* steps, void* stream);
int go2sim_wells_set_alive(go2sim_wells_t* h, const float* sum, const int32_t* steps, void* stream);
/* device address of alive_ep float32 [n_envs], for the host to reduce in place; inc as the kernel adds it */
int go2sim_wells_alive_ep(go2sim_wells_t* h, const float** alive_ep_dev, float* inc);

/* One step of all n == n_envs envs: one launch.  Component i of env b's position is pos[i * pos_comp_stride + b * pos_env_stride] (3 components), of
 * its quaternion quat[i * quat_comp_stride + b * quat_env_stride] (w, x, y, z), as for go2sim_lidar_step (go2sim_lidar_env_pose gives an env handle's
 * own buffers).  reset: uint8 [n] or NULL (no env was reset).  priv, n_in, priv_out: "Rows" above.  rew: float32 [n], updated in place, or NULL: the
 * alive term does not run (sums, counts and records stay).
 * GO2SIM_E_BADARG -- nothing is launched -- for a NULL handle, n != n_envs, a NULL pos, quat or priv_out, negative strides, n_in < 0, an inner row that
 * disagrees with n_in (NULL with n_in > 0, given with n_in == 0) and priv_out == priv. */
int go2sim_wells_step(go2sim_wells_t* h, int n, const float* pos, long long pos_comp_stride, long long pos_env_stride, const float* quat,
                      long long quat_comp_stride, long long quat_env_stride, const uint8_t* reset, const float* priv, int n_in, float* priv_out,
                      float* rew, void* stream);

#ifdef __cplusplus
}
#endif
#endif
