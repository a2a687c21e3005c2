"""CPU checks of the stairwell env's host side and of the law's restatement (tests/wells_ref.py), against the reference's own code
(tests/golden/ref_wells.npz, tests/golden/ref_cfgs_stairwell.json; tools/make_ref_stairwell_fixtures.py).

1. terrain_wells.build_stairwell_terrain equals the reference's builder exactly on the three configurations of tests/wells_cases.py.
2. wells_ref.scan_f32 equals the reference's _compute_height_scan bit for bit on every point that is not within rounding of a cell edge, and lies in
   the admissible set of wells_ref.scan_sets on all points.  wells_ref.assign_levels and wells_ref.spawn, fed the fixture's constant schedule, equal
   _assign_wells and _get_spawn_pos exactly.
3. get_stairwell_cfgs equals the train script's dictionaries; the mirror table; the routing predicate and the refusals, none of which touches a device."""
import copy
import json
import os

import numpy as np
import pytest

import wells_cases as WC
import wells_ref as R
from go2_sim2real_locomotion_rl_amd import Go2SimError
from go2_sim2real_locomotion_rl_amd.configs import (flatten_walk_cfg, get_rough_cfgs, get_stair_cfgs, get_stair_info_cfgs, get_stair_lidar_cfgs,
                                                    get_stairwell_cfgs)
from go2_sim2real_locomotion_rl_amd.capi import C
from go2_sim2real_locomotion_rl_amd.go2_env import Go2Env, mirror_tables
from go2_sim2real_locomotion_rl_amd.terrain_wells import build_stairwell_terrain, is_well_terrain_cfg, well_centers, well_scan_axes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "ref_wells.npz"))


# ---- 1. the builder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.TERRAINS))
def test_builder_equals_the_reference(fx, name):
    hf, info = build_stairwell_terrain(WC.TERRAINS[name])
    assert hf.dtype == np.int16 and hf.shape == fx[name + "_hf"].shape
    assert np.array_equal(hf, fx[name + "_hf"])
    assert np.array_equal(np.asarray(well_centers(info), np.float64), fx[name + "_centers"])
    assert np.array_equal(np.asarray(info["terrain_origin"], np.float64), fx[name + "_origin"])
    assert info["ground_height_m"] == float(fx[name + "_ground_height_m"])
    assert np.array_equal(np.asarray(info["step_heights_m"]), fx[name + "_step_heights_m"])
    assert (info["total_x_m"], info["total_y_m"]) == tuple(fx[name + "_total_m"])
    assert set(info) == {"heightfield", "horizontal_scale", "vertical_scale", "terrain_origin", "total_x_m", "total_y_m", "num_difficulty_levels",
                         "well_spawns", "step_heights_m", "ground_height_m", "steps_per_flight", "num_flights_per_side", "step_depth_m"}


def test_terrain_a_has_every_feature():
    hf, info = build_stairwell_terrain(WC.TERRAIN_A)
    assert hf.shape == (113, 78)                                             # three wells to a row, the fourth alone on the second row
    ground = hf.max()
    levels = [np.unique(hf[max(0, int(round((c[0] - info["terrain_origin"][0]) / 0.05)) - 12):int(round((c[0] - info["terrain_origin"][0]) / 0.05)) + 13,
                           max(0, int(round((c[1] - info["terrain_origin"][1]) / 0.05)) - 12):int(round((c[1] - info["terrain_origin"][1]) / 0.05)) + 13])
              for c in well_centers(info)]
    assert all(len(l) == 5 for l in levels)                                 # bottom, two steps, landing = the second step's height, two more steps: 5 heights
    assert hf[-30:, -30:].min() == ground                                   # the empty part of the second well row is ground


def test_training_field_size_is_derived():
    hf, info = build_stairwell_terrain(get_stairwell_cfgs()[0]["terrain"])
    # radius = 20 + 2 x 10 x 8 + 30 = 210 cells, block = 421 + 80, three blocks and a surround: 3 x 501 + 80
    assert hf.shape == (1583, 1583) and info["num_difficulty_levels"] == 9


# ---- 2. the restatement --------------------------------------------------------------------------------------------------------------------
def test_scan_restatement_equals_the_reference(fx):
    hf, info = build_stairwell_terrain(WC.TERRAIN_A)
    P = R.field(hf, info)
    xs, ys = well_scan_axes(WC.with_scan(WC.TERRAIN_A))
    assert np.array_equal(xs, fx["scan_xs"]) and np.array_equal(ys, fx["scan_ys"])
    pts = R.grid_points(xs, ys)
    got = R.scan_f32(P, fx["scan_pos"], fx["scan_quat"], pts)
    vals, tol, amb = R.scan_sets(P, fx["scan_pos"], fx["scan_quat"], pts)
    sure = ~amb
    print(f"{amb.sum()} of {amb.size} points lie within rounding of a cell edge")
    assert sure[:24].mean() > 0.95 and amb[24:].any()                      # the generic poses are decided, the named ones sit on cell edges
    assert np.array_equal(got[sure].view(np.uint32), fx["scan"][sure].view(np.uint32))
    for side in (got, fx["scan"]):
        ok, worst = R.match(side, vals, tol)
        assert ok.all(), worst
    assert len(np.unique(fx["scan"])) > 50                                  # the poses see stairs, not one plane


@pytest.mark.parametrize("k", range(3))
def test_assignment_and_spawn_equal_the_reference(fx, k):
    _, info = build_stairwell_terrain(WC.TERRAIN_A)
    u = list(fx[f"spawn{k}_u"])
    n = len(fx[f"spawn{k}_levels"])
    take = lambda: u.pop(0)
    draw = lambda lo, hi, count: np.array([lo + int(take() * (hi + 1 - lo)) for _ in range(count)], np.int64)
    levels = R.assign_levels(n, float(fx[f"spawn{k}_level"]), info["num_difficulty_levels"], draw, draw, fx[f"spawn{k}_perm"])
    assert len(fx[f"spawn{k}_u"]) - len(u) == int(fx[f"spawn{k}_n_assign_draws"])
    assert np.array_equal(levels, fx[f"spawn{k}_levels"])
    ux, uy = np.array(u[0::2]), np.array(u[1::2])
    x, y, _ = R.spawn(well_centers(info), levels, ux, uy)
    z = np.array([R.spawn_z(well_centers(info)[l][2], float(fx["spawn_base_init_z"])) for l in levels], np.float32)
    ref = fx[f"spawn{k}_pos"]
    assert np.array_equal(np.stack([x, y, z], 1).view(np.uint32), ref.view(np.uint32))
    if float(fx[f"spawn{k}_level"]) == 1.0:
        assert len(np.unique(levels)) >= 3                                  # frontier, near and easy wells all occur


def test_yaw_restatement_is_gs_rand_float():
    import torch

    lo, hi = np.radians(-5.0), np.radians(5.0)
    for u in WC.U_CYCLE:
        want = ((hi - lo) * torch.tensor([u], dtype=torch.float32) + lo).numpy()[0]
        assert R.rand_float(lo, hi, u).view(np.uint32) == want.view(np.uint32)


def test_alive_restatement():
    rew = np.zeros((5, 3), np.float32)
    resets = np.zeros((5, 3), bool)
    resets[2, 1] = resets[4, 0] = True
    out, s, k, ep = R.alive_steps(rew, resets, 0.2)
    inc = np.float32(0.2 * 0.02)
    assert np.all(out == inc) and list(k) == [0, 2, 5] and s[0] == 0.0
    three = np.float32(np.float32(inc + inc) + inc)
    assert ep[2, 1] == three / (np.float32(3.0) * np.float32(0.02)) and np.isnan(ep[2, 0])


# ---- 3. configuration, mirror, routing ---------------------------------------------------------------------------------------------------------
def test_cfgs_equal_the_reference_script():
    ref = json.load(open(os.path.join(GOLDEN, "ref_cfgs_stairwell.json")))
    env_cfg, obs_cfg, reward_cfg, command_cfg = get_stairwell_cfgs()
    assert env_cfg == ref["env_cfg"] and obs_cfg == ref["obs_cfg"] and command_cfg == ref["command_cfg"]
    assert reward_cfg == ref["reward_cfg"]                                  # (dict equality: the same items)
    names, ref_names = list(reward_cfg["reward_scales"]), list(ref["reward_cfg"]["reward_scales"])
    assert names[-1] == "alive" and ref_names[2] == "alive"                 # alive last here, third there (include/go2sim_wells.h says why)
    assert [n for n in names if n != "alive"] == [n for n in ref_names if n != "alive"]
    assert "forward_progress" not in names and obs_cfg["num_privileged_obs"] == 226
    assert get_stairwell_cfgs(False)[1] == dict(obs_cfg, num_obs=45, num_privileged_obs=222)


def test_mirror_table_swaps_the_scan_columns():
    env_cfg, obs_cfg, _, _ = get_stairwell_cfgs()
    t = mirror_tables(env_cfg, obs_cfg)
    src, sign = t["critic"][0].numpy(), t["critic"][1].numpy()
    assert len(src) == 226 and sorted(src) == list(range(226))
    assert np.array_equal(src[src], np.arange(226)) and np.all(sign[src] * sign == 1.0)     # an involution
    base = 49 + 56
    for i in range(11):
        for j in range(11):
            assert src[base + i * 11 + j] == base + i * 11 + (10 - j) and sign[base + i * 11 + j] == 1.0
    assert src[base - 1] == base - 1                                        # the well level is a fixed point
    assert len(t["policy"][0]) == 49
    bad = copy.deepcopy(env_cfg)
    bad["terrain"]["height_scan"]["y_range"] = [-0.5, 0.4]
    with pytest.raises(Go2SimError, match="not symmetric"):
        mirror_tables(bad, obs_cfg)


def test_routing_predicate():
    assert is_well_terrain_cfg(get_stairwell_cfgs()[0]["terrain"])
    for key in ("num_difficulty_levels", "wells_per_row", "steps_per_flight", "num_flights_per_side"):
        assert is_well_terrain_cfg({"enabled": True, key: 2})
        assert not is_well_terrain_cfg({"enabled": False, key: 2})
    assert not is_well_terrain_cfg(None) and not is_well_terrain_cfg({"enabled": True})
    for cfgs in (get_stair_cfgs(), get_stair_lidar_cfgs(), get_stair_info_cfgs(), get_rough_cfgs("grid"), get_rough_cfgs("heightmap")):
        assert not is_well_terrain_cfg(cfgs[0]["terrain"])


def test_flatten_routes_a_well_dictionary():
    cfgs = get_stairwell_cfgs()
    env_cfg = dict(cfgs[0], terrain=WC.with_scan(WC.TERRAIN_A))
    inner = dict(cfgs[1], num_privileged_obs=49 + 56)
    f, i, names = flatten_walk_cfg(8, env_cfg, inner, cfgs[2], cfgs[3])
    I, F = (lambda n: C["GO2SIM_IC_" + n]), (lambda n: C["GO2SIM_FC_" + n])
    assert i[I("WELL_SPAWN")] == 1 and i[I("USE_TERRAIN")] == 1 and i[I("TILE_MODE")] == 0 and i[I("SCAN_N")] == 0 and i[I("N_TERRAIN_ROWS")] == 4
    assert "alive" not in names and len(names) == 19 and i[I("N_REWARDS")] == 19
    _, info = build_stairwell_terrain(WC.TERRAIN_A)
    assert np.array_equal(f[F("ROW_CENTER0"):F("ROW_CENTER0") + 12], np.asarray(well_centers(info)).reshape(-1))     # doubles, unrounded
    assert f[F("TERRAIN_ORIGIN_X")] == info["terrain_origin"][0]
    # the corridor route keeps its flag off and its own limits
    f2, i2, _ = flatten_walk_cfg(8, *get_stair_cfgs())
    assert i2[I("WELL_SPAWN")] == 0 and i2[I("SCAN_N")] == 77
    wide = get_stair_cfgs()
    wide[0]["terrain"]["height_scan"] = dict(WC.SCAN_11)
    with pytest.raises(NotImplementedError, match="at most 80 points"):
        flatten_walk_cfg(8, *wide)


def test_refusals_before_any_device_work():
    cfgs = get_stairwell_cfgs()
    many = dict(cfgs[0], terrain=dict(WC.with_scan(WC.TERRAIN_A), num_difficulty_levels=17))
    with pytest.raises(Go2SimError, match="at most 16 difficulty levels"):
        flatten_walk_cfg(8, many, dict(cfgs[1], num_privileged_obs=105), cfgs[2], cfgs[3])
    wide = dict(cfgs[0], terrain=dict(WC.TERRAIN_A, height_scan=dict(WC.SCAN_11, num_x=17)))
    with pytest.raises(Go2SimError, match="at most 16 points per axis"):
        flatten_walk_cfg(8, wide, dict(cfgs[1], num_privileged_obs=105), cfgs[2], cfgs[3])
    for key, block in (("lidar", get_stair_lidar_cfgs()[0]["lidar"]), ("stair_info", get_stair_info_cfgs()[0]["stair_info"])):
        with pytest.raises(Go2SimError, match="does not combine"):
            Go2Env(8, dict(cfgs[0], **{key: block}), *cfgs[1:], device="cpu")
    with pytest.raises(Go2SimError, match="226"):                           # the widths the grid gives are named
        Go2Env(8, cfgs[0], dict(cfgs[1], num_privileged_obs=182), *cfgs[2:], device="cpu")
