"""Golden fixtures of the rough-terrain env from the reference's OWN code (needs a checkout of the reference project; nothing of it is stored here,
the outputs are data only).

    GO2SIM_REFERENCE_DIR=<reference checkout> python tools/make_ref_tiles_fixtures.py
        -> tests/golden/ref_tiles_manager.npz, tests/golden/ref_tiles_generator.npz

1. ref_tiles_manager.npz.  examples/locomotion/terrain_manager.py is loaded where it lies (importlib, on the repository's `genesis` alias package).  Its
   `TerrainManager` is built on the CPU for both modes of tests/tiles_cases.py -- a heightmap (the 6 x 5 field as a float array) and a 2 x 2 grid whose
   field is handed to `post_build` -- and its own `_query_height_batch`, `check_boundary` and `sample_spawn` are called.  The module's global `torch` is
   replaced by a forwarder whose `rand` / `randint` hand out, in the order the reference calls them (rows, columns, x jitter, y jitter), the draws that
   include/go2sim_tiles.h assigns to (seed, reset call 0): the words of tests/tiles_ref.spawn_words.  Recorded: heights at the finite query points,
   boundary flags, spawn positions and tiles, and every input.  The tool asserts that no boundary point lies within the height bound of max_wander and
   that both flags occur.

2. ref_tiles_generator.npz.  genesis/ext/isaacgym/terrain_utils.py is loaded the same way, with `genesis.utils.geom.cubic_spline_1d` taken from the
   reference's genesis/utils/geom.py (that one function is compiled from its source text at run time: the module itself needs packages that are not
   part of this project's environment).  `random_uniform_terrain` makes every random tile.  The tile loop of genesis/utils/terrain.py `parse_terrain`
   (:63-162: raster size, -inf fill, the seed-0 state of `randomize=False`, the maximum on shared edges) sits inside a function that builds meshes;
   THIS TOOL RESTATES THAT LOOP around the reference's tile function.  Recorded for numpy seeds 1 and 2, `randomize` on and off: the stitched fields."""
import ast
import importlib.util
import io
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("GO2SIM_REFERENCE_DIR")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 0x5EED0123456
N_SPAWN = 70
BASE_Z = 0.45


class DrawTorch:
    """Stands in for the global `torch` of the loaded module: rand / randint hand out the queued draws, every other attribute is torch's."""

    def __init__(self):
        self.queue = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand(self, n, **kw):
        kind, arr = self.queue.pop(0)
        assert kind == "rand" and arr.shape == (n,)
        return torch.from_numpy(arr.astype(np.float32))

    def randint(self, lo, hi, size, **kw):
        kind, (arr, want_hi) = self.queue.pop(0)
        assert kind == "randint" and lo == 0 and hi == want_hi and tuple(size) == arr.shape
        return torch.from_numpy(arr.astype(np.int64))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    with redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def manager_cases():
    import tiles_cases as TC

    rows, cols, hs, vs, _ = TC.FIELDS["6x5"]
    hm = {"enabled": True, "height_field": TC.field("6x5").astype(np.float32), "horizontal_scale": hs, "vertical_scale": vs, "spawn_height_offset": 0.05,
          "boundary_margin": 0.1}
    hf, grid = TC.grid_terrain_cfg("2x2")
    gr = {"enabled": True, "subterrain_types": [["flat_terrain", "random_uniform_terrain"], ["random_uniform_terrain", "flat_terrain"]],
          "subterrain_size": grid["size"], "horizontal_scale": TC.GRID_HS, "vertical_scale": TC.GRID_VS, "randomize": True, "spawn_height_offset": 0.05,
          "boundary_margin": grid["margin"]}
    return {"heightmap": (hm, hm["height_field"]), "grid": (gr, hf.astype(np.float32))}


def points_for(origin, hs, shape, rng):
    rows, cols = shape
    xs, ys = origin[0] + hs * np.arange(rows), origin[1] + hs * np.arange(cols)
    pts = [(x, y) for x in xs[:6] for y in ys[:5]] + [(xs[1] + hs / 2, ys[1]), (xs[1], ys[2] + hs / 2)]
    pts += [(origin[0] + hs * (rows - 1) * u, origin[1] + hs * (cols - 1) * v) for u, v in rng.random((60, 2))]
    pts += [(xs[0] - 1.0, ys[1]), (xs[-1] + 1.0, ys[1]), (xs[1], ys[0] - 1.0), (xs[1], ys[-1] + 1.0), (xs[rows - 2], ys[cols - 2])]
    return np.asarray(pts, np.float32)


def make_manager(mod):
    import tiles_ref as R

    fake = mod.torch = DrawTorch()
    data = {"seed": np.int64(SEED), "base_z": np.float64(BASE_Z), "n_spawn": np.int64(N_SPAWN)}
    for mode, (cfg, field_raw) in manager_cases().items():
        with redirect_stdout(io.StringIO()):
            mgr = mod.TerrainManager(cfg, N_SPAWN, device="cpu")
            mgr.build_terrain_morph()
            mgr.post_build(types.SimpleNamespace(height_field=field_raw))
        origin, hs, vs = np.asarray(mgr._terrain_origin, np.float64), float(mgr.horizontal_scale), float(mgr.vertical_scale)
        rng = np.random.default_rng(5)
        pts = points_for(origin, hs, field_raw.shape, rng)
        heights = mgr._query_height_batch(torch.from_numpy(pts[:, 0].copy()), torch.from_numpy(pts[:, 1].copy())).numpy()
        # spawn: the header's words for reset call 0, handed out in the reference's order
        w = R.spawn_words(N_SPAWN, SEED, 0)
        fake.queue = []
        if mode == "grid":
            fake.queue += [("randint", ((w[:, 0] % np.uint32(mgr.n_rows)).astype(np.int64), mgr.n_rows)),
                           ("randint", ((w[:, 1] % np.uint32(mgr.n_cols)).astype(np.int64), mgr.n_cols))]
        fake.queue += [("rand", R.u01(w[:, 2])), ("rand", R.u01(w[:, 3]))]
        spawn = mgr.sample_spawn(list(range(N_SPAWN)), base_init_z=BASE_Z).numpy()
        assert not fake.queue, "the reference did not consume the spawn's draws"
        # boundary: points around the spawn points at distances on both sides of max_wander, kept away from it by more than the height bound
        mw = float(mgr.max_wander)
        ang = rng.random(N_SPAWN) * 2 * np.pi
        dist = np.where(np.arange(N_SPAWN) % 2 == 0, mw * (0.3 + 0.65 * rng.random(N_SPAWN)), mw * (1.05 + rng.random(N_SPAWN)))
        base_xy = (spawn[:, :2].astype(np.float64) + dist[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
        flags = mgr.check_boundary(torch.from_numpy(base_xy)).numpy()
        d64 = np.linalg.norm(base_xy.astype(np.float64) - spawn[:, :2].astype(np.float64), axis=1)
        gap = 16.0 * R.ulp32(np.abs(base_xy).max() + mw)
        assert (np.abs(d64 - mw) > gap).all() and flags.any() and not flags.all(), "a boundary point is too close to max_wander, or one flag never occurs"
        data.update({f"{mode}_field_raw": field_raw, f"{mode}_origin": origin, f"{mode}_hs": np.float64(hs), f"{mode}_vs": np.float64(vs),
                     f"{mode}_points": pts, f"{mode}_heights": heights.astype(np.float32), f"{mode}_spawn": spawn.astype(np.float32),
                     f"{mode}_tile_row": mgr._env_tile_row.numpy().astype(np.int32), f"{mode}_tile_col": mgr._env_tile_col.numpy().astype(np.int32),
                     f"{mode}_base_xy": base_xy, f"{mode}_flags": flags.astype(np.uint8), f"{mode}_max_wander": np.float64(mw),
                     f"{mode}_margin": np.float64(cfg["boundary_margin"]), f"{mode}_spawn_offset": np.float64(cfg["spawn_height_offset"]),
                     f"{mode}_size": np.asarray(mgr.subterrain_size, np.float64), f"{mode}_n": np.asarray([mgr.n_rows, mgr.n_cols], np.int64)})
        print(f"manager {mode}: {len(pts)} heights, {int(flags.sum())} of {N_SPAWN} out of bounds, max_wander {mw}")
    return data


def reference_spline():
    """cubic_spline_1d of the reference's genesis/utils/geom.py, compiled from its source at run time with numpy and the alias's gs.np_float."""
    path = os.path.join(REF_ROOT, "genesis", "utils", "geom.py")
    tree = ast.parse(open(path).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "cubic_spline_1d")
    fn.decorator_list = []                                     # (its numba decorator: plain Python computes the same values)
    ns = {"np": np, "gs": types.SimpleNamespace(np_float=np.float32)}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["cubic_spline_1d"]


GEN = {"types": [["flat_terrain", "random_uniform_terrain"], ["random_uniform_terrain", "random_uniform_terrain"]], "size": (4.0, 6.0), "hs": 0.25, "vs": 0.005,
       "params": {"min_height": -0.08, "max_height": 0.08, "step": 0.1, "downsampled_scale": 0.5}}


def make_generator():
    import genesis as gs_alias
    import genesis.utils.geom as alias_geom

    had = hasattr(alias_geom, "cubic_spline_1d")
    alias_geom.cubic_spline_1d = reference_spline()
    if not hasattr(gs_alias._shim, "np_float"):
        gs_alias._shim.np_float = np.float32
    tu = load(os.path.join(REF_ROOT, "genesis", "ext", "isaacgym", "terrain_utils.py"), "ref_terrain_utils")
    eps = float(np.finfo(np.float32).eps)
    r, c = int(GEN["size"][0] / GEN["hs"] + eps) + 1, int(GEN["size"][1] / GEN["hs"] + eps) + 1
    n0, n1 = len(GEN["types"]), len(GEN["types"][0])
    data = {"types": np.array(GEN["types"]), "size": np.asarray(GEN["size"]), "hs": np.float64(GEN["hs"]), "vs": np.float64(GEN["vs"]),
            "param_names": np.array(sorted(GEN["params"])), "param_values": np.array([GEN["params"][k] for k in sorted(GEN["params"])])}
    for seed in (1, 2):
        for randomize in (True, False):
            np.random.seed(seed)
            field = np.full((n0 * (r - 1) + 1, n1 * (c - 1) + 1), -np.inf, np.float32)          # parse_terrain :63-162, restated (module docstring)
            for i in range(n0):
                for j in range(n1):
                    sub = tu.SubTerrain(width=r, length=c, vertical_scale=GEN["vs"], horizontal_scale=GEN["hs"])
                    if not randomize:
                        saved = np.random.get_state()
                        np.random.seed(0)
                    tile = np.zeros((r, c), np.float32) if GEN["types"][i][j] == "flat_terrain" else tu.random_uniform_terrain(sub, **GEN["params"]).height_field_raw
                    if not randomize:
                        np.random.set_state(saved)
                    sl = (slice(i * (r - 1), (i + 1) * (r - 1) + 1), slice(j * (c - 1), (j + 1) * (c - 1) + 1))
                    field[sl] = np.maximum(field[sl], tile)
            data[f"field_s{seed}_{'rand' if randomize else 'fixed'}"] = field
            print(f"generator seed {seed} randomize {randomize}: {field.shape}, range [{field.min()}, {field.max()}]")
    if not had:
        del alias_geom.cubic_spline_1d
    return data


def main():
    if not REF_ROOT:
        raise SystemExit("set GO2SIM_REFERENCE_DIR to a checkout of the reference project")
    mod = load(os.path.join(REF_ROOT, "examples", "locomotion", "terrain_manager.py"), "ref_terrain_manager")
    for name, data in (("ref_tiles_manager.npz", make_manager(mod)), ("ref_tiles_generator.npz", make_generator())):
        out = os.path.join(GOLDEN, name)
        np.savez_compressed(out, **data)
        print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
