// go2sim_tiles_dev.h -- the device functions of the rough-terrain walk env (include/go2sim_tiles.h states the law; the names here follow it): the
// bilinear ground height, the boundary test and the spawn of one env.  Shared by csrc/go2sim.hip (k_env_post_a, k_env_tile_spawn) and
// csrc/go2sim_tiles.hip (the query on arbitrary points), so that the env step and the test entry run the same code.
#ifndef GO2SIM_TILES_DEV_H
#define GO2SIM_TILES_DEV_H
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/go2sim_detmath.h"

// what the device functions see of the heightfield and of the tile grid
struct TileField {
  const float* hf;          // [rows][cols] metres, rows along world x
  int rows, cols;           // >= 2 each
  float ox, oy, hs;         // world position of cell (0, 0), cell size
};
struct TileGrid {
  int n_rows, n_cols;       // >= 1 each
  float size_x, size_y;     // tile size
  float jitter_x, jitter_y; // spawn jitter half-width per axis; <= 0 (or NaN): none
  float base_z, spawn_offset;
};

// l = clip(q, 0, n - 2) by comparisons a NaN fails (NaN and everything below 0 select 0, +inf selects n - 2): the cell index is inside the field
// before anything is loaded
__device__ __forceinline__ float tile_clip(float q, int n) {
  if (!(q > 0.0f)) return 0.0f;
  const float top = (float)(n - 2);
  if (q >= top) return top;
  return q;
}

// the law of include/go2sim_tiles.h, "Ground height": one IEEE binary32 operation per line of the header
__device__ __forceinline__ float tile_ground_height(const TileField& T, float wx, float wy) {
  const float lx = tile_clip((wx - T.ox) / T.hs, T.rows);
  const float ly = tile_clip((wy - T.oy) / T.hs, T.cols);
  const int ix = (int)lx, iy = (int)ly;                      // 0 <= ix <= rows - 2, 0 <= iy <= cols - 2
  const float fx = lx - (float)ix, fy = ly - (float)iy;
  const float* p = T.hf + (size_t)ix * T.cols + iy;
  const float h00 = p[0], h01 = p[1], h10 = p[T.cols], h11 = p[T.cols + 1];
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  float h = (h00 * gx) * gy;
  h = h + (h10 * fx) * gy;
  h = h + (h01 * gx) * fy;
  h = h + (h11 * fx) * fy;
  return h;
}

// "Boundary": strictly greater; a NaN anywhere fails the comparison (no termination)
__device__ __forceinline__ bool tile_out_of_bounds(float bx, float by, float sx, float sy, float max_wander) {
  const float dx = bx - sx, dy = by - sy;
  return dm_sqrt(dx * dx + dy * dy) > max_wander;
}

struct TileSpawn { float x, y, z; int row, col; };
// "Spawn": r = the Philox block of the env (words 0, 1: tile row, tile column; words 2, 3: the jitter uniforms of x, y)
__device__ __forceinline__ TileSpawn tile_spawn(const TileField& T, const TileGrid& G, const dm_u4& r) {
  TileSpawn s;
  s.row = (int)(r.v[0] % (uint32_t)G.n_rows);
  s.col = (int)(r.v[1] % (uint32_t)G.n_cols);
  float x = T.ox + ((float)s.row + 0.5f) * G.size_x;
  float y = T.oy + ((float)s.col + 0.5f) * G.size_y;
  if (G.jitter_x > 0.0f) x = x + (dm_u01(r.v[2]) * 2.0f - 1.0f) * G.jitter_x;
  if (G.jitter_y > 0.0f) y = y + (dm_u01(r.v[3]) * 2.0f - 1.0f) * G.jitter_y;
  s.x = x; s.y = y;
  s.z = (tile_ground_height(T, x, y) + G.base_z) + G.spawn_offset;
  return s;
}

#endif
