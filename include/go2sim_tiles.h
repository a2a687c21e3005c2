/* go2sim_tiles.h -- C ABI and law of the rough-terrain walk env: the reference's terrain fine-tuning env
 * (examples/locomotion/go2_env_Omni_kplearn_varied_terrain.py with examples/locomotion/terrain_manager.py: _query_height_batch :354, check_boundary
 * :338, _sample_spawn_grid :308, _sample_spawn_heightmap :285).  It is the 16-action walk env on a heightfield, with a bilinear ground height under
 * the base feeding _reward_base_height, a termination when the base wanders further than max_wander from its spawn point, and a random spawn tile at
 * every reset.  The reference answers the height query on the host with numpy every step; here all of it runs inside the step's launch chain.
 *
 * Conventions follow go2sim_lidar.h: extern "C", int status (0 = ok, GO2SIM_E_*), work is ordered on the given stream.  Product library only: there
 * is no CPU twin, the checker is the numpy float32 restatement tests/tiles_ref.py, itself pinned to the reference's own methods
 * (tests/golden/ref_tiles_manager.npz, tools/make_ref_tiles_fixtures.py).
 *
 * The mode.  GO2SIM_IC_TILE_MODE = 1 (with GO2SIM_IC_TILE_N_ROWS x GO2SIM_IC_TILE_N_COLS tiles, GO2SIM_FC_TILE_*) on a handle whose ground is a
 * heightfield (go2sim_set_terrain or go2sim_set_terrain_f32).  The heightmap mode of the reference is a 1 x 1 grid whose tile is the whole field.
 * GO2SIM_IC_USE_TERRAIN stays 0: the stair env's rows, height scan, row curriculum and terrain-relative foot terms are off.  With the mode off no
 * kernel computes anything differently.
 *
 * The field.  H = float32 [rows][cols] metres on the device (go2sim_set_terrain: f32(hf) * f32(vertical_scale) per cell; go2sim_set_terrain_f32:
 * the values given), rows along world x; (ox, oy) = world position of cell (0, 0), hs = cell size, both float32, as handed to the set call.
 *
 * The law.  Everything is float32: IEEE operations in the written order, one per line, no contraction.
 *
 * Ground height g(wx, wy):
 *   qx = (wx - ox) / hs                               (two operations)
 *   lx = 0 unless qx > 0;  rows - 2 if qx >= rows - 2;  else qx            likewise qy, ly with oy and cols
 *   ix = trunc(lx);  fx = lx - ix;  gx = 1 - fx                             likewise iy, fy, gy
 *   h00 = H[ix][iy], h10 = H[ix + 1][iy], h01 = H[ix][iy + 1], h11 = H[ix + 1][iy + 1]
 *   h = (h00 gx) gy
 *   h = h + (h10 fx) gy
 *   h = h + (h01 gx) fy
 *   h = h + (h11 fx) fy
 * -- _query_height_batch with the field already in metres (the reference interpolates raw units in float64 or float32, depending on the numpy
 * version, and multiplies by vertical_scale last; the difference is a few ulp of the heights).
 *
 * Every step, after the physics (k_env_post_a), for base position p and the env's spawn record s:
 *   ground_height = g(p.x, p.y)
 *   reset |= sqrt((p.x - s.x)^2 + (p.y - s.y)^2) > max_wander                 dx dx + dy dy, then a correctly rounded sqrt; strictly greater
 *   _reward_base_height = ((p.z - ground_height) - base_height_target)^2
 * The boundary reset is not a time-out.  The curriculum counters and the reset see it like a fall.
 *
 * Spawn, for every env whose reset flag is set (k_env_tile_spawn), from ONE Philox4x32-10 block (include/go2sim_detmath.h) with counter
 * (env, reset call, purpose 14, 0) and key (seed low word, seed high word); "reset call" is the number of reset calls before this one, the key
 * of every other draw of a reset (csrc/go2sim.hip, env_reset_one); purposes 1-13 belong to the env, the policy, the LIDAR scan and the stair info:
 *   tile_row = word0 mod n_rows;  tile_col = word1 mod n_cols                 the integer mapping of the stair env's rows (rand_int)
 *   x = ox + (f32(tile_row) + 0.5) size_x                                     two operations, then one addition
 *   x = x + ((dm_u01(word2) 2) - 1) jitter_x        only if jitter_x > 0      likewise y with tile_col, size_y, word3, jitter_y
 *   z = (g(x, y) + base_init_pos.z) + spawn_height_offset
 *   spawn_pos = (x, y, z)
 * and the reset that follows puts the base at spawn_pos (init_pos_z_range is ignored on terrain, as in the reference).  Envs that are not reset keep
 * their spawn record.  The tile centre is formed in float32 here and in float64 in the reference: at most an ulp of the coordinate apart.
 *
 * Safety and determinism.  Both cell indices are clamped before any load by comparisons that a NaN fails: a NaN coordinate and -inf give l = 0
 * on their axis, +inf gives l = n - 2, each with f = 0, so a pose of any value reads inside the field and the height of a finite field is finite.
 * A NaN distance fails the boundary comparison (no termination).  No atomics on floats, no LDS, no data-dependent trip counts: equal calls give
 * equal bits.
 *
 * Launches (csrc/go2sim.hip): the ground height and the boundary test are part of k_env_post_a (a branch on the mode, uniform over the launch);
 * k_env_tile_spawn, one lane per env, sits between k_env_post_a and k_env_post_b_team, where k_env_terrain_rows sits on stairs, and in the same
 * place of go2sim_env_reset / go2sim_env_reset_idx; the step's list stays a strict chain.  csrc/go2sim_tiles.hip: k_tiles_query, one lane per point.
 */
#ifndef GO2SIM_TILES_H
#define GO2SIM_TILES_H
#include <stddef.h>
#include <stdint.h>

#include "go2sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO2SIM_TILES_RNG_PURPOSE 14

/* go2sim_set_terrain with the heights given as float32 metres [rows][cols] (host memory): gs.morphs.Terrain(height_field=<float array>,
 * vertical_scale=1.0).  Everything after the int16 -> float conversion is shared with go2sim_set_terrain.  GO2SIM_E_BADARG also for a NaN or
 * infinite height. */
int go2sim_set_terrain_f32(go2sim_t* h, const float* hf_host, int rows, int cols, float horizontal_scale, const float* origin3_host, void* stream);

/* Ground height at n arbitrary points: xy_dev float32 [n][2] -> out_dev float32 [n] (device memory), by the device function the env step runs
 * (TerrainManager.get_height_at_robot; the kernel-level test entry).  Needs a heightfield on the handle, not the tile mode.  One launch, no
 * synchronisation.  GO2SIM_E_BADARG for a NULL pointer with n > 0, n < 0 or a handle without a heightfield. */
int go2sim_tiles_query(go2sim_t* h, const float* xy_dev, int n, float* out_dev, void* stream);

/* The heightfield of an env handle as the kernels read it: device pointer to float32 [rows][cols] metres, its shape, origin (x, y) and cell
 * size.  GO2SIM_E_BADARG without a heightfield. */
int go2sim_tiles_env_field(go2sim_t* h, const float** hf_dev, int* rows, int* cols, float* origin_xy2, float* horizontal_scale);

#ifdef __cplusplus
}
#endif
#endif
