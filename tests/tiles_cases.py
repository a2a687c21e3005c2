"""Cases of the rough-terrain env's tests: two small non-square heightfields (an axis swap shows on them), the query points of the kernel-level test,
the tile grids of the spawn test, and the env configurations the GPU tests build.  Imports numpy only at module level."""
import numpy as np

# name -> (rows, cols, horizontal scale, vertical scale, origin); rows run along world x
FIELDS = {"6x5": (6, 5, 0.25, 0.005, (-0.75, -0.5, 0.0)), "9x4": (9, 4, 0.5, 0.01, (-2.0, -1.0, 0.0))}


def field(name):
    """int16 raw units [rows][cols]: a seeded bumpy field, every cell different from its neighbours."""
    rows, cols = FIELDS[name][:2]
    rng = np.random.default_rng(rows * 100 + cols)
    return rng.integers(-40, 41, size=(rows, cols)).astype(np.int16)


def query_points(name):
    """float32 [n][2]: cell corners, edge midpoints, interior points, points outside on all four sides and the corners beyond, l exactly n - 2 on
    either axis, and the non-finite ones (kept last: `n_finite` of them are finite)."""
    rows, cols, hs, _, org = FIELDS[name]
    xs = org[0] + hs * np.arange(rows)
    ys = org[1] + hs * np.arange(cols)
    pts = [(x, y) for x in xs for y in ys]                                                  # corners
    pts += [(x + hs / 2, y) for x in xs[:-1] for y in ys] + [(x, y + hs / 2) for x in xs for y in ys[:-1]]   # edge midpoints
    rng = np.random.default_rng(7)
    pts += [(org[0] + hs * (rows - 1) * u, org[1] + hs * (cols - 1) * v) for u, v in rng.random((40, 2))]      # interior
    far = 3.0 * hs
    pts += [(xs[0] - far, ys[1]), (xs[-1] + far, ys[1]), (xs[1], ys[0] - far), (xs[1], ys[-1] + far),             # outside: clamp
            (xs[0] - far, ys[0] - far), (xs[-1] + far, ys[-1] + far), (xs[0] - far, ys[-1] + far), (xs[-1] + far, ys[0] - far), (1e30, -1e30)]
    pts += [(xs[rows - 2], ys[1] + 0.3 * hs), (xs[1] + 0.3 * hs, ys[cols - 2]), (xs[rows - 2], ys[cols - 2])]    # l == n - 2
    n_finite = len(pts)
    inf, nan = np.inf, np.nan
    pts += [(inf, ys[1]), (-inf, ys[1]), (xs[1], inf), (xs[1], -inf), (nan, ys[1]), (xs[1], nan), (nan, nan), (inf, -inf), (nan, inf)]
    return np.asarray(pts, np.float32), n_finite


# ---- spawn grids: name -> (n_rows, n_cols, tile size, boundary margin).  The field is flat tiles of 0.25 m cells with a bumpy overlay ------------
GRIDS = {"1x1": (1, 1, (4.0, 4.0), 0.5), "2x2": (2, 2, (4.0, 4.0), 0.5), "3x1": (3, 1, (4.0, 6.0), 0.5),
         "narrow": (2, 2, (3.0, 4.0), 1.0)}            # 3 / 2 - 1 - 0.5 = 0: no jitter along x only
GRID_HS, GRID_VS = 0.25, 0.005


def grid_terrain_cfg(name, seed=11):
    """A terrain dictionary in heightmap form whose field covers the grid `name` (the grid's tiles lie on it); -> (cfg, grid constants)"""
    n_rows, n_cols, size, margin = GRIDS[name]
    r, c = int(size[0] / GRID_HS) * n_rows + 1, int(size[1] / GRID_HS) * n_cols + 1
    hf = np.random.default_rng(seed).integers(-30, 31, size=(r, c)).astype(np.int16)
    return hf, dict(n_rows=n_rows, n_cols=n_cols, size=size, margin=margin,
                    origin=(-n_rows * size[0] / 2.0, -n_cols * size[1] / 2.0, 0.0),
                    jitter=(size[0] / 2.0 - margin - 0.5, size[1] / 2.0 - margin - 0.5), max_wander=min(size) / 2.0 - margin)


def tile_env_cfg(n_envs, grid, base_z=0.45, spawn_offset=0.05, mutate=None, tile=True):
    """(fcfg, icfg, reward names) of the walk configuration in tile mode on `grid` (the dict of grid_terrain_cfg): flatten_walk_cfg of the walk
    cfgs, then the tile entries written directly, so that the kernel-level tests control every constant."""
    from go2_sim2real_locomotion_rl_amd.capi import C
    from go2_sim2real_locomotion_rl_amd.configs import flatten_walk_cfg, get_walk_cfgs

    cfgs = get_walk_cfgs()
    cfgs[0]["base_init_pos"] = [0.0, 0.0, base_z]
    if mutate is not None:
        mutate(*cfgs)
    f, i, names = flatten_walk_cfg(n_envs, *cfgs)
    if tile:
        i[C["GO2SIM_IC_TILE_MODE"]], i[C["GO2SIM_IC_TILE_N_ROWS"]], i[C["GO2SIM_IC_TILE_N_COLS"]] = 1, grid["n_rows"], grid["n_cols"]
        f[C["GO2SIM_FC_TILE_SIZE_X"]], f[C["GO2SIM_FC_TILE_SIZE_Y"]] = grid["size"]
        f[C["GO2SIM_FC_TILE_JITTER_X"]], f[C["GO2SIM_FC_TILE_JITTER_Y"]] = grid["jitter"]
        f[C["GO2SIM_FC_TILE_MAX_WANDER"]], f[C["GO2SIM_FC_TILE_SPAWN_OFFSET"]] = grid["max_wander"], spawn_offset
    return f, i, names
