"""Procedural heightfields of ``gs.morphs.Terrain(n_subterrains=..., subterrain_types=...)`` (genesis/utils/terrain.py `parse_terrain`,
genesis/ext/isaacgym/terrain_utils.py `random_uniform_terrain`) for the two tile kinds the reference's terrain fine-tuning uses, written from
their law in numpy (imports neither torch nor the library, so the CPU tests run it):

  * a tile's raster is ``int(size / horizontal_scale + EPS) + 1`` vertices per axis, neighbouring tiles share their edge row / column;
  * the field starts at -inf and every tile is stitched in with a maximum, tiles visited row by row;
  * ``flat_terrain`` is zeros;
  * ``random_uniform_terrain`` draws ``np.random.choice(arange(min, max + step, step), (int(w / d), int(l / d)))`` in raw units (``int(metres /
    vertical_scale)``; w, l = raster x horizontal_scale, d = downsampled_scale), upsamples it to the raster with a not-a-knot cubic spline along y,
    then along x (both on ``linspace(0, w or l, n)`` knots), and rounds with ``rint``;
  * ``randomize=False`` generates every tile under ``np.random.seed(0)`` and puts the global state back afterwards.

The draws come from numpy's GLOBAL generator, as in the reference, so ``np.random.seed(s)`` ahead of the call reproduces the reference's field for
the same seed.  The reference evaluates the spline in float32 with its own banded solver, this module in float64 with scipy: a cell can differ by
one raw unit where the spline value lies on a rounding boundary of ``rint`` (tests/test_tiles_ref.py bounds exactly that)."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)     # gs.EPS at precision "32"
SUPPORTED = ("flat_terrain", "random_uniform_terrain")
# the subterrain names of the reference this module does not generate (genesis/options/morphs.py): refused by name
UNSUPPORTED = ("fractal_terrain", "sloped_terrain", "pyramid_sloped_terrain", "discrete_obstacles_terrain", "wave_terrain", "stairs_terrain",
               "pyramid_stairs_terrain", "stepping_stones_terrain")
DEFAULT_PARAMS = {"flat_terrain": {}, "random_uniform_terrain": {"min_height": -0.1, "max_height": 0.1, "step": 0.1, "downsampled_scale": 0.5}}


class TerrainError(ValueError):
    pass


def check_subterrain_types(subterrain_types, n_subterrains=None):
    """-> the types as a list of lists; TerrainError for a ragged table, a shape other than `n_subterrains` or a name that is not generated."""
    if isinstance(subterrain_types, str):
        if n_subterrains is None:
            raise TerrainError("a single subterrain type needs `n_subterrains`")
        subterrain_types = [[subterrain_types] * int(n_subterrains[1]) for _ in range(int(n_subterrains[0]))]
    rows = [list(r) for r in subterrain_types]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise TerrainError(f"`subterrain_types` should be a 2D list of strings with rows of one length, got rows of {[len(r) for r in rows]}")
    if n_subterrains is not None and (len(rows), len(rows[0])) != (int(n_subterrains[0]), int(n_subterrains[1])):
        raise TerrainError(f"`subterrain_types` has shape {(len(rows), len(rows[0]))}, `n_subterrains` is {tuple(n_subterrains)}")
    for r in rows:
        for name in r:
            if name in UNSUPPORTED:
                raise TerrainError(f"subterrain type {name!r} is not generated here: go2sim generates {list(SUPPORTED)}")
            if name not in SUPPORTED:
                raise TerrainError(f"Unsupported subterrain type: {name!r}, should be one of {list(SUPPORTED)}")
    return rows


def tile_raster(subterrain_size, horizontal_scale):
    return (int(subterrain_size[0] / horizontal_scale + EPS) + 1, int(subterrain_size[1] / horizontal_scale + EPS) + 1)


def _spline(x, y, xv):
    """not-a-knot cubic spline through (x, y[:, k]) evaluated at xv -> [len(xv), m], float64"""
    from scipy.interpolate import CubicSpline

    return CubicSpline(np.asarray(x, np.float64), np.asarray(y, np.float64), axis=0, bc_type="not-a-knot")(np.asarray(xv, np.float64))


def random_uniform_tile(rows, cols, horizontal_scale, vertical_scale, min_height=-0.1, max_height=0.1, step=0.1, downsampled_scale=0.5,
                        return_unrounded=False):
    """One ``random_uniform_terrain`` tile in raw units, float64 [rows][cols] of integers (and the values before ``rint`` on request)."""
    w, l = rows * horizontal_scale, cols * horizontal_scale
    lo, hi, st = int(min_height / vertical_scale), int(max_height / vertical_scale), int(step / vertical_scale)
    if st < 1:
        raise TerrainError(f"random_uniform_terrain: step {step} is below one raw unit (vertical_scale {vertical_scale})")
    shape = (int(w / downsampled_scale), int(l / downsampled_scale))
    if min(shape) < 4:
        raise TerrainError(f"random_uniform_terrain: a {shape} coarse grid is too small for the not-a-knot spline")
    coarse = np.random.choice(np.arange(lo, hi + st, st), shape)
    x, y = np.linspace(0, w, shape[0]), np.linspace(0, l, shape[1])
    xu, yu = np.linspace(0, w, rows), np.linspace(0, l, cols)
    z = _spline(x, _spline(y, coarse.T, yu).T, xu)
    return (np.rint(z), z) if return_unrounded else np.rint(z)


def generate_tiles(subterrain_types, subterrain_size, horizontal_scale, vertical_scale, randomize=True, subterrain_parameters=None,
                   n_subterrains=None, return_unrounded=False):
    """The stitched field in raw units, float32 [n_rows (r - 1) + 1][n_cols (c - 1) + 1] (heights = field x vertical_scale).  With
    `return_unrounded` also the float64 field of the values before ``rint`` (flat tiles: 0), stitched the same way."""
    types = check_subterrain_types(subterrain_types, n_subterrains)
    params = {k: dict(v) for k, v in DEFAULT_PARAMS.items()}
    for k, v in (subterrain_parameters or {}).items():
        params.setdefault(k, {}).update(v)
    r, c = tile_raster(subterrain_size, horizontal_scale)
    n0, n1 = len(types), len(types[0])
    field = np.full((n0 * (r - 1) + 1, n1 * (c - 1) + 1), -np.inf, np.float32)
    raw = np.full(field.shape, -np.inf, np.float64)
    for i in range(n0):
        for j in range(n1):
            if not randomize:
                saved = np.random.get_state()
                np.random.seed(0)
            try:
                if types[i][j] == "flat_terrain":
                    data, z = np.zeros((r, c)), np.zeros((r, c))
                else:
                    data, z = random_uniform_tile(r, c, horizontal_scale, vertical_scale, return_unrounded=True, **params["random_uniform_terrain"])
            finally:
                if not randomize:
                    np.random.set_state(saved)
            sl = (slice(i * (r - 1), (i + 1) * (r - 1) + 1), slice(j * (c - 1), (j + 1) * (c - 1) + 1))
            field[sl] = np.maximum(field[sl], data.astype(np.float32))
            raw[sl] = np.maximum(raw[sl], z)
    return (field, raw) if return_unrounded else field


# ---- the terrain dictionary of the rough-terrain env (env_cfg["terrain"]; examples/locomotion/terrain_manager.py) ---------------------------------
def is_tile_terrain_cfg(terrain_cfg):
    """A terrain dictionary that selects the rough-terrain (tile) mode: enabled, and carrying `subterrain_types` or a `height_field`.  The stair
    dictionaries carry neither."""
    t = terrain_cfg or {}
    return bool(t.get("enabled", False)) and (t.get("height_field") is not None or "subterrain_types" in t)


def install_terrain(sim, height_field, horizontal_scale, vertical_scale, origin):
    """The heightfield of a gs.morphs.Terrain on a Go2Sim handle: integer raw units through go2sim_set_terrain, a float field as float32 metres
    (f32(field) * f32(vertical_scale), the product go2sim_set_terrain forms per cell) through go2sim_set_terrain_f32."""
    hf = np.asarray(height_field)
    if np.issubdtype(hf.dtype, np.integer):
        sim.set_terrain(hf.astype(np.int16), horizontal_scale, vertical_scale, origin)
    else:
        sim.set_terrain_f32(hf.astype(np.float32) * np.float32(vertical_scale), horizontal_scale, origin)


def tile_layout(terrain_cfg):
    """The numbers of terrain_manager.py:38-132, 153-183, 290-291, 323-324 as python floats."""
    t = terrain_cfg
    hs, vs = float(t.get("horizontal_scale", 0.25)), float(t.get("vertical_scale", 0.005))
    margin = float(t.get("boundary_margin", 1.0))
    out = {"horizontal_scale": hs, "vertical_scale": vs, "boundary_margin": margin, "spawn_height_offset": float(t.get("spawn_height_offset", 0.05))}
    if t.get("height_field") is not None:
        hf = np.array(t["height_field"], dtype=np.float32)
        if hf.ndim != 2:
            raise TerrainError("`height_field` should be a 2D array.")
        size = (hf.shape[0] * hs, hf.shape[1] * hs)
        out.update(mode="heightmap", n_rows=1, n_cols=1, subterrain_types=None, height_field=hf)
    else:
        types = check_subterrain_types(t["subterrain_types"])
        size = tuple(float(v) for v in t.get("subterrain_size", (8.0, 8.0)))
        out.update(mode="grid", n_rows=len(types), n_cols=len(types[0]), subterrain_types=types, height_field=None,
                   randomize=bool(t.get("randomize", True)), subterrain_parameters=t.get("subterrain_parameters", None))
    out["subterrain_size"] = size
    out["origin"] = (-out["n_rows"] * size[0] / 2.0, -out["n_cols"] * size[1] / 2.0, 0.0)
    out["max_wander"] = min(size) / 2.0 - margin
    out["jitter"] = (size[0] / 2.0 - margin - 0.5, size[1] / 2.0 - margin - 0.5)
    return out
