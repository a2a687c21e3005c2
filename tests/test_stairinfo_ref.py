"""The stair info without a GPU: tests/stairinfo_ref.py reproduces the fixture recorded from the reference's own code (tests/golden/ref_stair_info.npz,
tools/make_ref_stairinfo_fixtures.py) -- masks exactly, values within the float32-against-float64 bound stairinfo_ref derives -- the terrain builder
equals the reference's heightfield bit for bit and today's output without the new keys, the fixture regenerates from a reference checkout, the GPU
case table keeps its ambiguous env-steps under 1 %, and the Python layer around the handle: cfgs, widths, refusals, mirror tables, exports."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import stairinfo_cases as SC
import stairinfo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_stair_info.npz")

EXPECTED = {"go2sim_stairinfo_create", "go2sim_stairinfo_destroy", "go2sim_stairinfo_step", "go2sim_stairinfo_clear", "go2sim_stairinfo_get_step",
            "go2sim_stairinfo_set_step", "go2sim_stairinfo_get_state", "go2sim_stairinfo_set_state", "go2sim_stairinfo_env_rows"}
# sha256 of build_stair_terrain(get_stair_terrain_cfg()) as the commit before the per-row depths returned it: dtype, shape and bytes of the heightfield,
# then the json of the info dict without the heightfield, keys sorted (`terrain_digest` below)
PARENT_TERRAIN_DIGEST = "99a17fca550ced358047a2f686266f12d28407b3b6a2b5729b927022e7656252"


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def fixture_constants(fx, block):
    N = dict(zip([str(k) for k in fx["scalar_names"]], [float(v) for v in fx["scalar_values"]]))
    N.update(zip([str(k) for k in fx["noise_names"]], [float(v) for v in fx["noise_values"]]))
    N["edge_dist_scale"], N["threshold"] = float(fx[block + "_edge_dist_scale"]), float(fx[block + "_threshold"])
    cfg = SC.stair_info_cfg(int(fx["num_samples"]), edge_dist_scale=N["edge_dist_scale"], threshold=N["threshold"])
    N["sample_x"] = SC.layout_of(cfg)["sample_x"]
    N["row_heights"], N["row_depths"] = fx["step_heights_m"].astype(np.float32), fx["step_depths_m"].astype(np.float32)
    P = {"hf": fx["hf"], "origin": tuple(fx["origin"]), "h_scale": float(fx["h_scale"]), "v_scale": float(fx["v_scale"])}
    return P, N


# ---- 1. stairinfo_ref against the reference's methods -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["s37", "s1", "t105"])
def test_stairinfo_ref_reproduces_the_reference_fixture(fx, block):
    """Per step: the restated Philox draws are the recorded ones bit for bit (as float32, what torch was handed), so the masks are the reference's
    exactly; both buffers match one admissible candidate within stairinfo_ref's bound, the direction and every masked entry exactly."""
    P, N = fixture_constants(fx, block)
    L, seed = float(fx["level"]), int(fx["seed"])
    g = lambda k: fx[f"{block}_{k}"]
    n = g("pos").shape[1]
    prev = np.zeros((n, 4), np.float32)
    fired = {"flip": 0, "latency": 0, "blackout": 0, "reset": 0, "seen": 0, "not_seen": 0, "ambiguous": 0}
    worst_all = 0.0
    for t in range(g("pos").shape[0]):
        d = R.draws(n, seed, t)
        for k in d:
            assert np.array_equal(d[k].astype(np.float32), g(k)[t]), f"draw {k} of step {t} is not the recorded one"
        d32 = {k: g(k)[t].astype(np.float64) for k in d}
        cands, m = R.stair_info(P, N, g("pos")[t], g("quat")[t], g("rows")[t], L, d32, prev, g("reset")[t])
        ok, worst, _ = R.match(g("actor")[t], g("clean")[t], cands)
        amb = sum(len(c) > 1 for c in cands)
        print(f"{block} step {t}: worst ratio {worst:.3f}, ambiguous {amb}")
        assert ok.all(), np.flatnonzero(~ok)
        rows0 = m["reset"]
        assert not g("actor")[t][rows0].any() and not g("clean")[t][rows0].any()
        top = np.float32(np.float32(N["max_range"]) * np.float32(N["edge_dist_scale"]))
        assert (g("actor")[t][m["blackout"], 0] == top).all() and not g("actor")[t][m["blackout"], 3].any()
        for k in ("flip", "latency", "blackout", "reset"):
            fired[k] += int(m[k].sum())
        fired["ambiguous"] += amb
        worst_all = max(worst_all, worst)
        prev = g("actor")[t]
    names = SC.poses(n, SC.STEPS, seed, N["sample_x"], fx["step_depths_m"].tolist(), thr_row=3 if N["threshold"] > 0.1 else 0)[2]
    for t in range(SC.STEPS):
        for b in range(n):
            if names[t][b].startswith("threshold_") and not g("reset")[t][b]:
                fired["seen" if g("clean")[t][b, 3] > 0 else "not_seen"] += 1
    print(f"{block}: fired {fired}, worst ratio {worst_all:.3f}")
    assert all(fired[k] > 0 for k in ("flip", "latency", "blackout", "reset", "not_seen")) and fired["ambiguous"] == 0
    assert (fired["seen"] > 0) == (block == "t105")       # the default threshold never sees row 0's riser; 0.105 sees row 3's third by float32 rounding
    assert worst_all <= 1.0


def test_scale_blocks_show_the_divide_and_multiply_of_stale_rows(fx):
    """A stale edge is stored / s_e * s_e in float32: the identity with s_e = 1, the float32 divide-then-multiply with 3.7 (bit for bit numpy's)."""
    seen = {"s1": 0, "s37": 0}
    for block in seen:
        P, N = fixture_constants(fx, block)
        s = np.float32(N["edge_dist_scale"])
        for t in range(1, SC.STEPS):
            d = {k: fx[f"{block}_{k}"][t].astype(np.float64) for k in ("u_flip", "u_lat", "u_black")}
            m = R.masks_of(N, float(fx["level"]), d, fx[f"{block}_reset"][t])
            for b in np.flatnonzero(m["latency"] & ~m["blackout"]):
                prev = fx[f"{block}_actor"][t - 1][b, 0]
                if prev != 0:
                    assert fx[f"{block}_actor"][t][b, 0] == np.float32(np.float32(prev / s) * s)
                    seen[block] += 1
    assert min(seen.values()) > 0, seen


def test_fixture_regenerates_from_the_reference_checkout(fx):
    ref = os.environ.get("GO2SIM_REFERENCE_DIR")
    if not ref or not os.path.exists(os.path.join(ref, "examples", "locomotion", "go2_env_stair_lidar_2.py")):
        pytest.skip("GO2SIM_REFERENCE_DIR does not point at a checkout of the reference project")
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_ref_stairinfo_fixtures", os.path.join(ROOT, "tools", "make_ref_stairinfo_fixtures.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    new = tool.make()
    assert set(new) == set(fx)
    for k, v in new.items():
        v = np.asarray(v)
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape and v.tobytes() == fx[k].tobytes(), k


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) < 100 * 1024


# ---- 2. the terrain ---------------------------------------------------------------------------------------------------------------------------
def terrain_digest(hf, info):
    h = hashlib.sha256()
    h.update(str(hf.dtype).encode()); h.update(str(hf.shape).encode()); h.update(np.ascontiguousarray(hf).tobytes())
    h.update(json.dumps({k: v for k, v in info.items() if k != "heightfield"}, sort_keys=True).encode())
    return h.hexdigest()


def test_terrain_with_the_recorded_depths_is_the_references_bit_for_bit(fx):
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain

    hf, info = build_stair_terrain(dict(SC.TERRAIN_CFG, step_depths_m=fx["step_depths_m"].tolist()))
    assert hf.dtype == fx["hf"].dtype and hf.shape == fx["hf"].shape and hf.tobytes() == fx["hf"].tobytes()
    assert np.asarray(info["row_centers"], np.float64).tobytes() == fx["row_centers"].tobytes()
    assert np.asarray(info["terrain_origin"], np.float64).tobytes() == fx["origin"].tobytes()
    assert info["step_depths_m"] == fx["step_depths_m"].tolist() and info["step_heights_m"] == fx["step_heights_m"].tolist()
    assert info["heightfield"] is hf and (info["horizontal_scale"], info["vertical_scale"]) == (float(fx["h_scale"]), float(fx["v_scale"]))
    # the reference pads: three of the four rows are shallower than the deepest, their ascent ends at the top height, their descent at 0
    assert sorted(np.round(fx["step_depths_m"] / 0.05).astype(int).tolist()) == [2, 3, 3, 4]


def test_terrain_without_the_new_keys_is_todays():
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain, get_stair_terrain_cfg

    hf, info = build_stair_terrain(get_stair_terrain_cfg())
    assert "step_depths_m" not in info and info["heightfield"] is hf
    assert terrain_digest(hf, info) == PARENT_TERRAIN_DIGEST


def test_terrain_permutation_is_seeded_and_two_calls_agree():
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain, get_stair_info_terrain_cfg, stair_step_depths

    for cfg in (SC.TERRAIN_CFG, get_stair_info_terrain_cfg()):
        (hf1, i1), (hf2, i2) = build_stair_terrain(cfg), build_stair_terrain(dict(cfg))
        assert hf1.tobytes() == hf2.tobytes() and terrain_digest(hf1, i1) == terrain_digest(hf2, i2)
        rows = cfg["num_difficulty_rows"]
        lo, hi = cfg["step_depth_range"]
        assert sorted(i1["step_depths_m"]) == np.linspace(lo, hi, rows).tolist() and i1["step_depths_m"] != np.linspace(lo, hi, rows).tolist()
        other = build_stair_terrain(dict(cfg, step_depth_seed=1))[1]["step_depths_m"]
        assert sorted(other) == sorted(i1["step_depths_m"]) and other != i1["step_depths_m"]
        assert stair_step_depths(cfg).tolist() == i1["step_depths_m"]
    hf, info = build_stair_terrain(get_stair_info_terrain_cfg())
    cells = int(np.round(0.30 / 0.05))
    assert hf.shape == (40 + 4 * (2 * 6 * cells + 30 + 30) + 40, 13 * 120) and hf.max() == 6 * 40          # 6 steps of 0.20 m in the hardest row
    with pytest.raises(ValueError, match="one value per difficulty row"):
        build_stair_terrain(dict(SC.TERRAIN_CFG, step_depths_m=[0.1, 0.2]))
    # a scalar range, as the reference accepts it: every row the same depth
    assert build_stair_terrain(dict(SC.TERRAIN_CFG, step_depth_range=0.15))[1]["step_depths_m"] == [0.15] * 4


# ---- 3. the GPU case table's own condition ----------------------------------------------------------------------------------------------------
def test_case_table_keeps_ambiguous_env_steps_under_one_percent():
    """The admissible-set answer of stairinfo_ref alone, over every distinct pose table of tests/test_stairinfo_gpu.py."""
    seen, amb_all, tot_all = set(), 0, 0
    for case in SC.cases():
        key = (case[1], case[2], case[7], case[8])
        if key in seen:
            continue
        seen.add(key)
        amb, tot = SC.ambiguous_env_steps(case)
        print(f"{case[0]}: ambiguous {amb}/{tot}")
        assert amb <= 0.01 * tot, case[0]
        amb_all, tot_all = amb_all + amb, tot_all + tot
    print(f"all tables: ambiguous {amb_all}/{tot_all} = {100.0 * amb_all / tot_all:.3f} %")


def test_case_table_holds_the_named_poses():
    """On the clean detector of stairinfo_ref: up and down the stairs, across a row boundary both ways, the last and the first pair, none in range, the
    threshold riser on both sides."""
    case = [c for c in SC.cases() if c[0] == "s14-n67-L1"][0]
    inp = SC.case_inputs(case)
    N = inp["N"]
    xs = N["sample_x"]
    sets = R.edge_sets(inp["P"], inp["pos"][0], inp["quat"][0], xs, N["max_range"], N["threshold"])
    by = {inp["names"][0][b]: sets[b] for b in range(67)}
    mid = lambda k: float((xs[k] + xs[k + 1]) / np.float32(2.0))
    none = [(float(np.float32(0.27)), 0.0)]
    assert by["up"][0][1] == 1.0 and by["down"][0][1] == -1.0 and by["row_boundary"][0][1] == 1.0 and by["row_boundary_down"][0][1] == -1.0
    assert by["last_pair"] == [(mid(12), 1.0)] and by["first_pair"] == [(mid(0), 1.0)] and by["none"] == none
    assert by["threshold_first"] == none and by["threshold_second"] == none and by["threshold_third"] == none
    assert by["yaw_pi_plus"][0][1] == -1.0 and by["yaw_pi_minus"][0][1] == -1.0
    for name in ("beyond_x_lo", "beyond_x_hi"):                # the clamped column is flat ground (beyond the y edges the clamped row's stairs stay in view)
        assert by[name] == none
    case = [c for c in SC.cases() if c[0] == "s14-n67-L1-thr105"][0]
    inp = SC.case_inputs(case)
    sets = R.edge_sets(inp["P"], inp["pos"][0], inp["quat"][0], xs, 0.27, 0.105)
    by = {inp["names"][0][b]: sets[b] for b in range(67)}
    assert by["threshold_first"] == none and by["threshold_third"][0][1] == 1.0 and len(by["threshold_third"]) == 1


def test_a_sample_on_a_riser_gives_a_set_of_two_and_either_member_matches():
    """A sample that falls on the cell boundary of a riser (within delta) may be looked up on either side: the edge lies in the pair before it or in
    the pair after it.  Both are admissible, nothing else is."""
    case = [c for c in SC.cases() if c[0] == "s14-n5-L0"][0]
    inp = SC.case_inputs(case)
    N, xs = inp["N"], inp["N"]["sample_x"]
    pos = np.array([[SC.X_FIRST_RISER - float(xs[5]), SC.row_y(2), 0.4]], np.float32)
    quat = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    sets = R.edge_sets(inp["P"], pos, quat, xs, N["max_range"], N["threshold"])
    mid = lambda k: float((xs[k] + xs[k + 1]) / np.float32(2.0))
    assert sets == [[(mid(4), 1.0), (mid(5), 1.0)]]
    cands, _ = R.stair_info(inp["P"], N, pos, quat, [2], 0.0, R.draws(1, 1, 0), np.zeros((1, 4), np.float32))
    assert len(cands[0]) == 2
    for k in (4, 5):
        row = np.array([[np.float32(mid(k)) * np.float32(3.7), N["row_heights"][2] * np.float32(5.0), N["row_depths"][2] * np.float32(3.3), 1.0]], np.float32)
        assert R.match(row, row, cands)[0].all()
    wrong = np.array([[np.float32(mid(6)) * np.float32(3.7), N["row_heights"][2] * np.float32(5.0), N["row_depths"][2] * np.float32(3.3), 1.0]], np.float32)
    assert not R.match(wrong, wrong, cands)[0].any()


def test_dr_level_mapping_and_draw_layout():
    s = {"phase1_level": 0.15, "terrain_gate": 0.5}
    assert R.dr_level(0.3, None) == 0.3 and R.dr_level(0.49, s) == 0.15 and abs(R.dr_level(0.8, s) - 0.66) < 1e-15
    d0, d1 = R.draws(5, 9, 0), R.draws(5, 9, 1)
    assert set(d0) == {"z_e", "z_h", "z_d", "u_flip", "u_lat", "u_black"} and all(v.shape == (5,) for v in d0.values())
    assert not any(np.array_equal(d0[k], d1[k]) for k in d0)
    import lidar_ref

    assert R.PURPOSE == 13 and lidar_ref.PURPOSE == 12


# ---- 4. the Python layer ------------------------------------------------------------------------------------------------------------------------
def _is_involution(src, sign):
    src, sign = src.tolist(), sign.tolist()
    return sorted(src) == list(range(len(src))) and all(src[src[j]] == j and sign[j] * sign[src[j]] == 1.0 for j in range(len(src)))


@pytest.mark.parametrize("pls,widths", [(True, (53, 113, 16)), (False, (49, 109, 12))])
def test_mirror_tables_of_the_stair_info_layout(pls, widths):
    from go2_sim2real_locomotion_rl_amd import get_stair_cfgs, get_stair_info_cfgs
    from go2_sim2real_locomotion_rl_amd.go2_env import mirror_tables

    env_cfg, obs_cfg, _, _ = get_stair_info_cfgs(pls_enable=pls)
    t = mirror_tables(env_cfg, obs_cfg)
    for key, w in zip(("policy", "critic", "actions"), widths):
        src, sign = t[key]
        assert len(src) == len(sign) == w and _is_involution(src, sign), key
    n_in = widths[0] - 4
    for key, o in (("policy", n_in), ("critic", n_in), ("critic", widths[1] - 4)):         # the four columns: fixed points, sign +1
        src, sign = t[key]
        assert src[o:o + 4].tolist() == [o, o + 1, o + 2, o + 3] and sign[o:o + 4].tolist() == [1.0] * 4
    src, sign = t["critic"]
    assert src[widths[1] - 5] == widths[1] - 5 and sign[widths[1] - 5] == 1.0                 # the terrain row
    s_env, s_obs, _, _ = get_stair_cfgs(pls_enable=pls)
    ssrc, ssign = mirror_tables(s_env, s_obs)["critic"]
    assert (src[n_in + 4:n_in + 60] - 4).tolist() == ssrc[n_in:n_in + 56].tolist() and sign[n_in + 4:n_in + 60].tolist() == ssign[n_in:n_in + 56].tolist()
    assert src[:n_in].tolist() == ssrc[:n_in].tolist() and sign[:n_in].tolist() == ssign[:n_in].tolist()


def test_cfgs_widths_and_the_refusals_by_name():
    from go2_sim2real_locomotion_rl_amd import Go2SimError, get_stair_cfgs, get_stair_info_cfg, get_stair_info_cfgs, get_stair_lidar_cfgs
    from go2_sim2real_locomotion_rl_amd.configs import get_lidar_cfg, get_stair_info_terrain_cfg
    from go2_sim2real_locomotion_rl_amd.lidar import lidar_enabled
    from go2_sim2real_locomotion_rl_amd.stairinfo import check_stair_info_widths, stair_info_enabled, stair_info_layout, stair_info_widths

    for pls, (no, npriv, n_in) in ((True, (53, 113, 49)), (False, (49, 109, 45))):
        env_cfg, obs_cfg, reward_cfg, command_cfg = get_stair_info_cfgs(pls_enable=pls)
        assert (obs_cfg["num_obs"], obs_cfg["num_privileged_obs"]) == (no, npriv) and stair_info_enabled(env_cfg) and not lidar_enabled(env_cfg)
        assert check_stair_info_widths(env_cfg, obs_cfg) == n_in and stair_info_widths(env_cfg) == (n_in, no, npriv)
        # get_stair_cfgs() plus the block, the script's terrain block and the widths; nothing else
        s_env, s_obs, s_rew, s_cmd = get_stair_cfgs(pls_enable=pls)
        assert not stair_info_enabled(s_env) and reward_cfg == s_rew and command_cfg == s_cmd
        assert {k: v for k, v in env_cfg.items() if k not in ("stair_info", "terrain")} == {k: v for k, v in s_env.items() if k != "terrain"}
        assert {k: v for k, v in obs_cfg.items() if k not in ("num_obs", "num_privileged_obs")} == {k: v for k, v in s_obs.items() if k not in ("num_obs", "num_privileged_obs")}
        assert env_cfg["stair_info"] == get_stair_info_cfg() and env_cfg["terrain"] == get_stair_info_terrain_cfg()
    t = get_stair_info_terrain_cfg()
    assert t["step_depth_range"] == [0.22, 0.30] and t["step_height_max"] == 0.20 and "step_depth_m" not in t and "height_scan" not in t
    b = get_stair_info_cfg()
    assert b["edge_detection"] == {"max_range": 0.27, "threshold": 0.02, "num_samples": 14}
    assert (b["edge_dist_scale"], b["height_scale"], b["depth_scale"], b["direction_scale"]) == (3.7, 5.0, 3.3, 1.0)
    assert b["noise"] == {"edge_noise_std": 0.04, "height_noise_std": 0.01, "depth_noise_std": 0.01, "direction_flip_prob": 0.03, "full_blackout_prob": 0.05,
                          "latency_prob": 0.10}
    custom = get_stair_info_cfgs(stair_info=dict(b, edge_dist_scale=1.0))[0]["stair_info"]
    assert custom["edge_dist_scale"] == 1.0 and b["edge_dist_scale"] == 3.7
    # the layout reads the block as StairInfoConfig does: defaults for missing keys, float32 linspace samples
    lay = stair_info_layout({})
    assert lay["sample_x"].dtype == np.float32 and lay["sample_x"].shape == (14,) and lay["sample_x"][0] == 0 and lay["sample_x"][-1] == np.float32(0.27)
    assert lay["edge_dist_scale"] == 1.0 / 0.27 and lay["latency_prob"] == 0.10 and lay["threshold"] == 0.02
    # refusals, by name
    env_cfg, obs_cfg, _, _ = get_stair_info_cfgs()
    obs_cfg["num_obs"] = 49
    with pytest.raises(Go2SimError, match=r"49 / 113.*53 / 113"):
        check_stair_info_widths(env_cfg, obs_cfg)
    env_cfg["stair_info"]["enabled"] = False
    assert not stair_info_enabled(env_cfg)
    for bad, word in (({"num_samples": 1}, "num_samples"), ({"num_samples": 65}, "num_samples"), ({"max_range": -0.1}, "max_range"),
                      ({"max_range": float("inf")}, "max_range"), ({"threshold": float("nan")}, "threshold"), ({"threshold": -1.0}, "threshold")):
        with pytest.raises(Go2SimError, match=word):
            stair_info_layout({"edge_detection": bad})
    assert lidar_enabled(get_stair_lidar_cfgs()[0]) and get_lidar_cfg()["enabled"]


def test_both_exteroceptive_blocks_together_are_refused_by_name():
    """`lidar` + `stair_info` in one env_cfg: the check Go2Env's constructor runs before any GPU work"""
    from go2_sim2real_locomotion_rl_amd import Go2Env, Go2SimError, get_stair_info_cfgs, get_stair_lidar_cfgs
    from go2_sim2real_locomotion_rl_amd.configs import get_lidar_cfg
    from go2_sim2real_locomotion_rl_amd.stairinfo import check_one_exteroceptive_layout

    cfgs = get_stair_info_cfgs()
    check_one_exteroceptive_layout(cfgs[0])
    check_one_exteroceptive_layout(get_stair_lidar_cfgs()[0])
    cfgs[0]["lidar"] = get_lidar_cfg()
    with pytest.raises(Go2SimError, match="both `lidar` and `stair_info`"):
        check_one_exteroceptive_layout(cfgs[0])
    with pytest.raises(Go2SimError, match="both `lidar` and `stair_info`"):
        Go2Env(4, *cfgs, device="cpu")


def test_header_parses_into_a_list_of_its_own_and_the_library_exports_it(libs_built):
    from go2_sim2real_locomotion_rl_amd import capi

    assert set(capi.DECLARED_STAIRINFO_FUNCS) == EXPECTED and len(capi.DECLARED_STAIRINFO_FUNCS) == len(EXPECTED)
    for other in (capi.DECLARED_FUNCS, capi.DECLARED_TRAIN_FUNCS, capi.DECLARED_RNN_FUNCS, capi.DECLARED_NORM_FUNCS, capi.DECLARED_LIDAR_FUNCS):
        assert not set(other) & EXPECTED
    assert len(capi.DECLARED_FUNCS) == 53
    assert capi.C["GO2SIM_STAIRINFO_RNG_PURPOSE"] == R.PURPOSE == 13 and capi.C["GO2SIM_STAIRINFO_PRIV_EXTRA"] == 56 and capi.C["GO2SIM_STAIRINFO_N"] == 4
    assert capi.C["GO2SIM_STAIRINFO_MAX_SAMPLES"] == 64 and capi.C["GO2SIM_STAIRINFO_MAX_ROWS"] == 16
    for name in ("go2sim.h", "go2sim_lidar.h"):                                          # declared in the new header only
        assert "stairinfo" not in open(os.path.join(ROOT, "include", name)).read()
    if not os.path.exists(capi.HIP_LIB):
        pytest.fail("csrc/libgo2sim.so has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert EXPECTED <= exported, sorted(EXPECTED - exported)


def test_cfg_struct_matches_the_header():
    """StairInfoCfg's fields, in order, are the header's: doubles first, then ints"""
    import re

    from go2_sim2real_locomotion_rl_amd.stairinfo import StairInfoCfg

    txt = open(os.path.join(ROOT, "include", "go2sim_stairinfo.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} go2sim_stairinfo_cfg_t;", txt, flags=re.S).group(1), flags=re.S)
    fields = []
    for kind, names in re.findall(r"(double|int)\s+([^;]+);", body):
        fields += [(n.strip(), kind) for n in names.split(",")]
    assert fields == [(n, "double") for n in StairInfoCfg.DOUBLES] + [(n, "int") for n in StairInfoCfg.INTS]


def test_package_exports_the_class_and_the_cfgs():
    import go2_sim2real_locomotion_rl_amd as pkg
    from go2_sim2real_locomotion_rl_amd.stairinfo import StairInfo

    assert pkg.StairInfo is StairInfo and {"StairInfo", "get_stair_info_cfg", "get_stair_info_cfgs"} <= set(pkg.__all__)
    assert callable(pkg.get_stair_info_cfg) and callable(pkg.get_stair_info_cfgs)
