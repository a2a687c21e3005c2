"""CPU checks of the rough-terrain env's host side and of the law's restatement.

1. tests/tiles_ref.py against the reference's own TerrainManager (tests/golden/ref_tiles_manager.npz, tools/make_ref_tiles_fixtures.py), both modes:
   heights within the per-case bound  4 ulp32(max |w - origin|) / hs x D + 8 ulp32(max |h|)  (D: the largest difference between adjacent cells) -- the
   reference interpolates raw units in a float32 / float64 mix that depends on the numpy version and scales last, which is what the bound absorbs;
   boundary flags and tiles exactly (the tool keeps the boundary points away from max_wander); spawn x, y within 2 ulp32 of the largest coordinate
   (the tile centre is formed in float64 there, in float32 here; the jitter product and the sum round once each) and z within the height bound, moved by
   the x, y difference times the steepest slope, plus 2 ulp32 of z.  The package's TerrainManager, fed the same draws, must give the restatement's
   bits (it states the same operations in torch).
2. terrain_tiles.generate_tiles against the reference's generator (tests/golden/ref_tiles_generator.npz): flat tiles and stitching equal; a
   random_uniform cell may differ by at most one raw unit, and only where this module's float64 value before rint lies within 1e-3 of a half-integer
   (the reference's float32 spline at magnitudes of about 16 units errs far below 1e-3).
3. get_rough_cfgs against the reference train script's dictionaries (tests/golden/ref_cfgs_rough_*.json), and the refusals."""
import json
import os

import numpy as np
import pytest

import tiles_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("heightmap", "grid")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "ref_tiles_manager.npz"))


def case(fx, mode):
    g = {k[len(mode) + 1:]: fx[k] for k in fx.files if k.startswith(mode + "_")}
    g["H"] = R.metres(g["field_raw"], float(g["vs"]))
    size = g["size"]
    margin = float(g["margin"])
    g["grid"] = dict(n_rows=int(g["n"][0]), n_cols=int(g["n"][1]), size=(float(size[0]), float(size[1])),
                     jitter=(float(size[0]) / 2.0 - margin - 0.5, float(size[1]) / 2.0 - margin - 0.5), base_z=float(fx["base_z"]),
                     spawn_offset=float(g["spawn_offset"]))
    return g


@pytest.mark.parametrize("mode", MODES)
def test_heights_within_the_bound_of_the_reference(fx, mode):
    g = case(fx, mode)
    pts = g["points"]
    got = R.ground_height(g["H"], g["origin"], float(g["hs"]), pts[:, 0], pts[:, 1])
    bound = R.height_bound(g["H"], g["origin"], float(g["hs"]), pts[:, 0], pts[:, 1])
    err = np.abs(got.astype(np.float64) - g["heights"].astype(np.float64)).max()
    print(f"{mode}: worst |restatement - reference| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(g["heights"]).max() > 100 * bound, "the heights are not trivially small against the bound"


@pytest.mark.parametrize("mode", MODES)
def test_boundary_flags_are_the_reference_s(fx, mode):
    g = case(fx, mode)
    got = R.out_of_bounds(g["base_xy"][:, 0], g["base_xy"][:, 1], g["spawn"][:, 0], g["spawn"][:, 1], float(g["max_wander"]))
    assert np.array_equal(got.astype(np.uint8), g["flags"]) and 0 < g["flags"].sum() < len(g["flags"])
    # strictly greater: a point at exactly max_wander stays in
    mw = np.float32(g["max_wander"])
    assert not R.out_of_bounds([mw], [0.0], [0.0], [0.0], mw)[0] and R.out_of_bounds([np.nextafter(mw, np.float32(np.inf))], [0.0], [0.0], [0.0], mw)[0]


@pytest.mark.parametrize("mode", MODES)
def test_spawn_tiles_exact_and_positions_within_rounding(fx, mode):
    g = case(fx, mode)
    n, seed = int(fx["n_spawn"]), int(fx["seed"])
    pos, row, col = R.spawn(g["H"], g["origin"], float(g["hs"]), g["grid"], R.spawn_words(n, seed, 0))
    assert np.array_equal(row, g["tile_row"]) and np.array_equal(col, g["tile_col"])
    if mode == "grid":
        assert set(row) == {0, 1} and set(col) == {0, 1}
    tol_xy = 2.0 * R.ulp32(np.abs(g["spawn"][:, :2]).max())
    err_xy = np.abs(pos[:, :2].astype(np.float64) - g["spawn"][:, :2]).max()
    H64 = g["H"].astype(np.float64)
    slope = max(np.abs(np.diff(H64, axis=0)).max(), np.abs(np.diff(H64, axis=1)).max()) / float(g["hs"])
    tol_z = R.height_bound(g["H"], g["origin"], float(g["hs"]), pos[:, 0], pos[:, 1]) + 2.0 * slope * tol_xy + 2.0 * R.ulp32(np.abs(g["spawn"][:, 2]).max())
    err_z = np.abs(pos[:, 2].astype(np.float64) - g["spawn"][:, 2]).max()
    print(f"{mode}: spawn xy err {err_xy:.3e} (tol {tol_xy:.3e}), z err {err_z:.3e} (tol {tol_z:.3e})")
    assert err_xy <= tol_xy and err_z <= tol_z


@pytest.mark.parametrize("mode", MODES)
def test_the_package_manager_states_the_same_law(fx, mode, monkeypatch):
    """TerrainManager (stand-alone, CPU tensors) fed the fixture's draws: the restatement's bits."""
    import types

    import torch

    from go2_sim2real_locomotion_rl_amd import terrain_manager as TM

    g = case(fx, mode)
    n, seed = int(fx["n_spawn"]), int(fx["seed"])
    cfg = {"enabled": True, "horizontal_scale": float(g["hs"]), "vertical_scale": float(g["vs"]), "spawn_height_offset": float(g["spawn_offset"]),
           "boundary_margin": float(g["margin"])}
    if mode == "heightmap":
        cfg["height_field"] = g["field_raw"]
    else:
        cfg.update(subterrain_types=[["flat_terrain", "random_uniform_terrain"], ["random_uniform_terrain", "flat_terrain"]], subterrain_size=tuple(g["size"]))
    mgr = TM.TerrainManager(cfg, n, device="cpu")
    assert mgr.enabled and mgr.max_wander == float(g["max_wander"]) and np.allclose(mgr._terrain_origin, g["origin"], atol=0)
    mgr.post_build(types.SimpleNamespace(height_field=g["field_raw"]))
    pts = g["points"]
    h = mgr.get_height_at_robot(torch.from_numpy(pts.copy())).numpy()
    want = R.ground_height(g["H"], g["origin"], float(g["hs"]), pts[:, 0], pts[:, 1])
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    w = R.spawn_words(n, seed, 0)
    queue = []
    if mode == "grid":
        queue += [torch.from_numpy((w[:, 0] % np.uint32(2)).astype(np.int64)), torch.from_numpy((w[:, 1] % np.uint32(2)).astype(np.int64))]
    queue += [torch.from_numpy(R.u01(w[:, 2])), torch.from_numpy(R.u01(w[:, 3]))]
    monkeypatch.setattr(TM.torch, "randint", lambda *a, **k: queue.pop(0))
    monkeypatch.setattr(TM.torch, "rand", lambda *a, **k: queue.pop(0))
    pos = mgr.sample_spawn(list(range(n)), base_init_z=float(fx["base_z"])).numpy()
    monkeypatch.undo()
    assert not queue
    wpos, wrow, wcol = R.spawn(g["H"], g["origin"], float(g["hs"]), g["grid"], w)
    assert np.array_equal(mgr.get_env_tile_rows().numpy(), wrow) and np.array_equal(mgr._env_tile_col.numpy(), wcol)
    # the manager's tile centre is the reference's (float64, then rounded): x, y within one rounding of the restatement, which forms it in float32
    assert np.abs(pos[:, :2].astype(np.float64) - wpos[:, :2]).max() <= 2.0 * R.ulp32(np.abs(wpos[:, :2]).max())
    flags = mgr.check_boundary(torch.from_numpy(g["base_xy"].copy()) - torch.from_numpy(g["spawn"][:, :2].copy()) + mgr._env_spawn_pos[:, :2]).numpy()
    assert np.array_equal(flags.astype(np.uint8), g["flags"])
    assert mgr.get_terrain_type_string(0) == ("custom_heightmap" if mode == "heightmap" else cfg["subterrain_types"][wrow[0]][wcol[0]])
    assert TM.TerrainManager({"enabled": False}, 4, device="cpu").enabled is False


# ---- 2. the generator ------------------------------------------------------------------------------------------------------------------------------
def test_generator_against_the_reference_s_fields():
    from go2_sim2real_locomotion_rl_amd import terrain_tiles as TT

    fx = np.load(os.path.join(GOLDEN, "ref_tiles_generator.npz"))
    types_, size, hs, vs = [list(r) for r in fx["types"]], tuple(fx["size"]), float(fx["hs"]), float(fx["vs"])
    params = {"random_uniform_terrain": dict(zip([str(k) for k in fx["param_names"]], [float(v) for v in fx["param_values"]]))}
    r, c = TT.tile_raster(size, hs)
    assert (r, c) == (17, 25)
    fields = {}
    for seed in (1, 2):
        for randomize in (True, False):
            ref = fx[f"field_s{seed}_{'rand' if randomize else 'fixed'}"]
            np.random.seed(seed)
            before = np.random.get_state()[1].copy()
            got, raw = TT.generate_tiles(types_, size, hs, vs, randomize=randomize, subterrain_parameters=params, return_unrounded=True)
            if not randomize:
                assert np.array_equal(np.random.get_state()[1], before), "randomize=False leaves the global state as it was"
            assert got.shape == ref.shape == (2 * (r - 1) + 1, 2 * (c - 1) + 1) and got.dtype == np.float32
            assert np.array_equal(got[:r - 1, :c - 1], ref[:r - 1, :c - 1]) and not got[:r - 1, :c - 1].any(), "the flat tile (inside its shared edges)"
            diff = got.astype(np.float64) - ref
            off = np.abs(diff) > 0
            frac = np.abs(raw - np.floor(raw) - 0.5)
            print(f"seed {seed} randomize {randomize}: {int(off.sum())} of {off.size} cells differ, worst {np.abs(diff).max()}, their distance to a half-integer <= {frac[off].max() if off.any() else 0:.2e}")
            assert np.abs(diff).max() <= 1.0 and (frac[off] <= 1e-3).all()
            assert len(np.unique(got)) > 10
            fields[(seed, randomize)] = got
    assert not np.array_equal(fields[(1, True)], fields[(2, True)]) and np.array_equal(fields[(1, False)], fields[(2, False)])
    # stitching: a shared edge holds the maximum of its two tiles, so the flat tile's border is never below 0
    f = fields[(1, True)]
    assert (f[:r, c - 1] >= 0).all() and (f[r - 1, :c] >= 0).all()
    # randomize=False: every random tile is the same tile
    g = fields[(1, False)]
    assert np.array_equal(g[r:, 1:c - 1], g[r:, c:-1][:, :c - 2])


def test_refusals():
    from go2_sim2real_locomotion_rl_amd import genesis_shim as gs
    from go2_sim2real_locomotion_rl_amd import terrain_tiles as TT

    with pytest.raises(gs.GenesisException, match="pyramid_stairs_terrain"):
        gs.morphs.Terrain(n_subterrains=(1, 2), subterrain_types=[["flat_terrain", "pyramid_stairs_terrain"]], subterrain_size=(4.0, 4.0))
    with pytest.raises(gs.GenesisException, match="moon_terrain"):
        gs.morphs.Terrain(n_subterrains=(1, 1), subterrain_types=[["moon_terrain"]], subterrain_size=(4.0, 4.0))
    with pytest.raises(gs.GenesisException, match="rows of one length"):
        gs.morphs.Terrain(n_subterrains=(2, 2), subterrain_types=[["flat_terrain", "flat_terrain"], ["flat_terrain"]], subterrain_size=(4.0, 4.0))
    with pytest.raises(TT.TerrainError, match="rows of one length"):
        TT.tile_layout({"enabled": True, "subterrain_types": [["flat_terrain"], []]})
    with pytest.raises(gs.GenesisException, match="2D"):
        gs.morphs.Terrain(height_field=np.zeros(5, np.float32))
    m = gs.morphs.Terrain(height_field=np.zeros((4, 3)), horizontal_scale=0.5, vertical_scale=1.0, pos=(-1.0, -0.75, 0.0))
    assert m.height_field.dtype == np.float32 and m.kind == "terrain"
    assert gs.morphs.Terrain(height_field=np.zeros((4, 3), np.int16)).height_field.dtype == np.int16
    # the stair dictionaries carry neither key: they keep going to the stair builder
    from go2_sim2real_locomotion_rl_amd.configs import get_stair_cfgs

    assert not TT.is_tile_terrain_cfg(get_stair_cfgs()[0]["terrain"]) and not TT.is_tile_terrain_cfg(None) and not TT.is_tile_terrain_cfg({"enabled": False, "subterrain_types": []})


# ---- 3. the cfgs -------------------------------------------------------------------------------------------------------------------------------------
def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


@pytest.mark.parametrize("mode", MODES)
def test_rough_cfgs_are_the_train_script_s(mode):
    import hashlib

    from go2_sim2real_locomotion_rl_amd.capi import C
    from go2_sim2real_locomotion_rl_amd.configs import flatten_walk_cfg, get_rough_cfgs

    ref = json.load(open(os.path.join(GOLDEN, f"ref_cfgs_rough_{mode}.json")))
    env_cfg, obs_cfg, reward_cfg, command_cfg = get_rough_cfgs(mode, seed=ref["numpy_seed"])
    terrain = dict(env_cfg["terrain"])
    hf = terrain.pop("height_field", None)
    ref_terrain = dict(ref["env_cfg"]["terrain"])
    ref_hf = ref_terrain.pop("height_field", None)
    assert _plain(terrain) == ref_terrain
    if mode == "heightmap":
        assert list(hf.shape) == ref_hf["shape"] and hf.dtype == np.float32 and hashlib.sha256(np.ascontiguousarray(hf).tobytes()).hexdigest() == ref_hf["sha256"]
        assert not hf[:, :150].any() and hf[:, 150:].any()
    assert _plain({k: v for k, v in env_cfg.items() if k != "terrain"}) == {k: v for k, v in ref["env_cfg"].items() if k != "terrain"}
    assert list(reward_cfg["reward_scales"]) == list(ref["reward_cfg"]["reward_scales"])          # the evaluation order of the terms
    assert _plain(obs_cfg) == ref["obs_cfg"] and _plain(reward_cfg) == ref["reward_cfg"] and _plain(command_cfg) == ref["command_cfg"]
    f, i, _ = flatten_walk_cfg(64, env_cfg, obs_cfg, reward_cfg, command_cfg)
    assert i[C["GO2SIM_IC_TILE_MODE"]] == 1 and i[C["GO2SIM_IC_USE_TERRAIN"]] == 0 and i[C["GO2SIM_IC_SCAN_N"]] == 0
    want = {"heightmap": (1, 1, 15.0, 15.0, 6.0, 6.0, 6.5), "grid": (2, 2, 8.0, 8.0, 2.5, 2.5, 3.0)}[mode]
    got = (i[C["GO2SIM_IC_TILE_N_ROWS"]], i[C["GO2SIM_IC_TILE_N_COLS"]], f[C["GO2SIM_FC_TILE_SIZE_X"]], f[C["GO2SIM_FC_TILE_SIZE_Y"]],
           f[C["GO2SIM_FC_TILE_JITTER_X"]], f[C["GO2SIM_FC_TILE_JITTER_Y"]], f[C["GO2SIM_FC_TILE_MAX_WANDER"]])
    assert got == want and f[C["GO2SIM_FC_TILE_SPAWN_OFFSET"]] == 0.05
