"""The LIDAR scan without a GPU: tests/lidar_ref.py reproduces the fixture recorded from the reference's own methods (tests/golden/ref_lidar_scan.npz,
tools/make_ref_lidar_fixtures.py) -- masks exactly, values within the float32-against-float64 bound lidar_ref derives -- the fixture regenerates from a
reference checkout, the GPU case table keeps its ambiguous points rare, and the Python layer around the handle: mirror tables, cfg widths, exports."""
import os
import subprocess

import numpy as np
import pytest

import lidar_cases as LC
import lidar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_lidar_scan.npz")

EXPECTED = {"go2sim_lidar_create", "go2sim_lidar_destroy", "go2sim_lidar_get_step", "go2sim_lidar_set_step", "go2sim_lidar_clear", "go2sim_lidar_get_scan",
            "go2sim_lidar_set_scan", "go2sim_lidar_step", "go2sim_lidar_env_pose"}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


# ---- 1. lidar_ref against the reference's methods ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["s1", "s05"])
def test_lidar_ref_reproduces_the_reference_fixture(fx, block):
    """Per step: the restated Philox draws are the recorded ones bit for bit (as float32, what torch was handed), so the three masks are the
    reference's exactly; both buffers lie in the admissible set within lidar_ref's bound (torch's float32 atan2 / sin / cos are within the error
    the cell tolerance delta allows the yaw, and the recorded z are the float64 normals rounded once, so EZ is not even used up)."""
    lay = LC.layout_of(LC.lidar_cfg("5x3_9x5"))
    P = {"hf": fx["hf"], "origin": tuple(fx["origin"]), "h_scale": float(fx["h_scale"]), "v_scale": float(fx["v_scale"])}
    N = dict(zip([str(k) for k in fx["noise_names"]], [float(v) for v in fx["noise_values"]]), height_clip=float(fx["height_clip"]),
             height_scale=float(fx[block + "_height_scale"]))
    L, seed = float(fx["level"]), int(fx["seed"])
    g = lambda k: fx[f"{block}_{k}"]
    n, na = g("pos").shape[1], lay["actor_xy"].shape[1]
    prev = np.zeros((n, na), np.float32)
    fired = {"dropout": 0, "latency": 0, "blackout": 0, "reset": 0}
    worst_all = 0.0
    for t in range(g("pos").shape[0]):
        d = R.draws(n, na, seed, t)
        for k in ("z", "u", "z_b", "u_lat", "u_black"):
            assert np.array_equal(d[k].astype(np.float32), g(k)[t]), f"draw {k} of step {t} is not the recorded one"
        d32 = {k: g(k)[t].astype(np.float64) for k in d}
        v, tol, amb, masks = R.actor_scan(P, N, g("pos")[t], g("quat")[t], lay["actor_xy"], L, d32, prev, g("reset")[t])
        ok, worst = R.match(g("actor")[t], v, tol)
        vc, tolc, ambc = R.critic_scan(P, N, g("pos")[t], g("quat")[t], lay["critic_xy"], g("reset")[t])
        okc, worstc = R.match(g("critic")[t], vc, tolc)
        print(f"{block} step {t}: actor worst ratio {worst:.3f} (ambiguous {int(amb.sum())}), critic {worstc:.3f} (ambiguous {int(ambc.sum())})")
        assert ok.all() and okc.all()
        # the masks show in the recorded buffer: a blacked-out or reset row is 0, a stale row is the previous buffer clipped and scaled again
        rows0 = masks["blackout"] | masks["reset"]
        assert not g("actor")[t][rows0].any()
        stale = masks["latency"] & ~masks["blackout"]
        assert np.array_equal(g("actor")[t][stale], np.float32(R.clip_scale(prev[stale].astype(np.float64), N["height_clip"], N["height_scale"])))
        for k in fired:
            fired[k] += int(masks[k].sum())
        worst_all = max(worst_all, worst, worstc)
        prev = g("actor")[t]
    assert all(c > 0 for c in fired.values()), fired
    assert worst_all <= 1.0


def test_half_scale_block_shows_the_double_scaling(fx):
    """height_scale 0.5: a stale row holds a quarter of the raw height, not half -- the stored scan was scaled once when it was stored"""
    N = dict(zip([str(k) for k in fx["noise_names"]], [float(v) for v in fx["noise_values"]]))
    seen = 0
    for t in range(1, fx["s05_pos"].shape[0]):
        lat = (fx["s05_u_lat"][t] < R.threshold(N["latency_prob"], float(fx["level"]))) & (fx["s05_reset"][t] == 0)
        black = fx["s05_u_black"][t] < R.threshold(N["full_blackout_prob"], float(fx["level"]))
        for b in np.flatnonzero(lat & ~black):
            prev = fx["s05_actor"][t - 1][b]
            if prev.any():
                assert np.array_equal(fx["s05_actor"][t][b], prev * np.float32(0.5))
                seen += 1
    assert seen > 0


def test_fixture_regenerates_from_the_reference_checkout(fx):
    ref = os.environ.get("GO2SIM_REFERENCE_DIR")
    if not ref or not os.path.exists(os.path.join(ref, "examples", "locomotion", "go2_env_stair_lidar.py")):
        pytest.skip("GO2SIM_REFERENCE_DIR does not point at a checkout of the reference project")
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_ref_lidar_fixtures", os.path.join(ROOT, "tools", "make_ref_lidar_fixtures.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    new = tool.make()
    assert set(new) == set(fx)
    for k, v in new.items():
        v = np.asarray(v)
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape and v.tobytes() == fx[k].tobytes(), k


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) < 128 * 1024


# ---- 2. the GPU case table's own condition ----------------------------------------------------------------------------------------------------
def test_case_table_keeps_ambiguous_points_rare():
    seen = set()
    for case in LC.cases():
        key = (case[1], case[2], case[7])
        if key in seen:
            continue
        seen.add(key)
        frac = LC.ambiguous_fraction(case)
        print(f"{case[0]}: ambiguous {100 * frac:.3f} %")
        assert frac <= 0.02, case[0]


def test_dr_level_mapping():
    s = {"phase1_level": 0.15, "terrain_gate": 0.5}
    assert R.dr_level(0.3, None) == 0.3 and R.dr_level(0.3, None, curriculum_enabled=False) == 1.0
    assert R.dr_level(0.49, s) == 0.15 and R.dr_level(0.5, s) == 0.15 and R.dr_level(1.0, s) == 1.0
    assert abs(R.dr_level(0.8, s) - 0.66) < 1e-15


# ---- 3. the Python layer ------------------------------------------------------------------------------------------------------------------------
def _is_involution(src, sign):
    src, sign = src.tolist(), sign.tolist()
    return sorted(src) == list(range(len(src))) and all(src[src[j]] == j and sign[j] * sign[src[j]] == 1.0 for j in range(len(src)))


@pytest.mark.parametrize("pls,widths", [(True, (64, 165, 16)), (False, (60, 161, 12))])
def test_mirror_tables_of_the_lidar_layout(pls, widths):
    from go2_sim2real_locomotion_rl_amd import get_stair_lidar_cfgs
    from go2_sim2real_locomotion_rl_amd.go2_env import mirror_tables

    env_cfg, obs_cfg, _, _ = get_stair_lidar_cfgs(pls_enable=pls)
    t = mirror_tables(env_cfg, obs_cfg)
    for key, w in zip(("policy", "critic", "actions"), widths):
        src, sign = t[key]
        assert len(src) == len(sign) == w and _is_involution(src, sign), key
    n_in = widths[0] - 15
    # the 5 x 3 block, entry by entry: point ix * 3 + iy <-> ix * 3 + (2 - iy), sign +1
    block = [2, 1, 0, 5, 4, 3, 8, 7, 6, 11, 10, 9, 14, 13, 12]
    for key in ("policy", "critic"):
        src, sign = t[key]
        assert src[n_in:n_in + 15].tolist() == [n_in + k for k in block] and sign[n_in:n_in + 15].tolist() == [1.0] * 15
    # the 9 x 5 block closes the critic row: ix * 5 + iy <-> ix * 5 + (4 - iy)
    block = [4, 3, 2, 1, 0, 9, 8, 7, 6, 5, 14, 13, 12, 11, 10, 19, 18, 17, 16, 15, 24, 23, 22, 21, 20, 29, 28, 27, 26, 25, 34, 33, 32, 31, 30,
             39, 38, 37, 36, 35, 44, 43, 42, 41, 40]
    src, sign = t["critic"]
    o = widths[1] - 45
    assert src[o:].tolist() == [o + k for k in block] and sign[o:].tolist() == [1.0] * 45
    assert src[o - 1] == o - 1 and sign[o - 1] == 1.0                                   # the terrain row is a fixed point
    # between the two scans the critic row is the stair layout's privileged block, moved by the 15 scan columns
    from go2_sim2real_locomotion_rl_amd import get_stair_cfgs

    s_env, s_obs, _, _ = get_stair_cfgs(pls_enable=pls)
    ssrc, ssign = mirror_tables(s_env, s_obs)["critic"]
    assert (src[n_in + 15:o] - 15).tolist() == ssrc[n_in:n_in + 56].tolist() and sign[n_in + 15:o].tolist() == ssign[n_in:n_in + 56].tolist()
    assert src[:n_in].tolist() == ssrc[:n_in].tolist()


def test_asymmetric_scans_have_no_mirror():
    from go2_sim2real_locomotion_rl_amd import Go2SimError, get_stair_lidar_cfgs
    from go2_sim2real_locomotion_rl_amd.go2_env import mirror_tables

    env_cfg, obs_cfg, _, _ = get_stair_lidar_cfgs()
    env_cfg["lidar"]["actor_scan"]["y_points"] = [-0.15, 0.0, 0.2]
    with pytest.raises(Go2SimError, match="actor scan"):
        mirror_tables(env_cfg, obs_cfg)
    env_cfg, obs_cfg, _, _ = get_stair_lidar_cfgs()
    env_cfg["lidar"]["critic_scan"]["y_range"] = [-0.3, 0.2]
    with pytest.raises(Go2SimError, match="critic scan"):
        mirror_tables(env_cfg, obs_cfg)


def test_cfg_widths_and_the_refusal_by_name():
    from go2_sim2real_locomotion_rl_amd import Go2SimError, get_stair_cfgs, get_stair_lidar_cfgs
    from go2_sim2real_locomotion_rl_amd.lidar import check_lidar_widths, lidar_enabled

    for pls, (no, npriv, n_in) in ((True, (64, 165, 49)), (False, (60, 161, 45))):
        env_cfg, obs_cfg, reward_cfg, command_cfg = get_stair_lidar_cfgs(pls_enable=pls)
        assert (obs_cfg["num_obs"], obs_cfg["num_privileged_obs"]) == (no, npriv) and lidar_enabled(env_cfg)
        assert check_lidar_widths(env_cfg, obs_cfg) == n_in
        assert env_cfg["terrain"]["height_scan"] == {"num_x": 9, "num_y": 5, "x_range": [-0.4, 0.8], "y_range": [-0.3, 0.3]}
        s_env, _, s_rew, s_cmd = get_stair_cfgs(pls_enable=pls)
        assert not lidar_enabled(s_env) and reward_cfg == s_rew and command_cfg == s_cmd
        assert {k: v for k, v in env_cfg.items() if k not in ("lidar", "terrain")} == {k: v for k, v in s_env.items() if k != "terrain"}
    env_cfg, obs_cfg, _, _ = get_stair_lidar_cfgs()
    obs_cfg["num_obs"] = 49
    with pytest.raises(Go2SimError, match=r"49 / 165.*64 / 165"):
        check_lidar_widths(env_cfg, obs_cfg)
    env_cfg["lidar"]["enabled"] = False
    assert not lidar_enabled(env_cfg)


def test_header_parses_into_a_list_of_its_own_and_the_library_exports_it(libs_built):
    from go2_sim2real_locomotion_rl_amd import capi

    assert set(capi.DECLARED_LIDAR_FUNCS) == EXPECTED and len(capi.DECLARED_LIDAR_FUNCS) == len(EXPECTED)
    for other in (capi.DECLARED_FUNCS, capi.DECLARED_TRAIN_FUNCS, capi.DECLARED_RNN_FUNCS, capi.DECLARED_NORM_FUNCS):
        assert not set(other) & EXPECTED
    assert capi.C["GO2SIM_LIDAR_RNG_PURPOSE"] == R.PURPOSE == 12 and capi.C["GO2SIM_LIDAR_PRIV_EXTRA"] == 56
    if not os.path.exists(capi.HIP_LIB):
        pytest.fail("csrc/libgo2sim.so has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert EXPECTED <= exported, sorted(EXPECTED - exported)


def test_package_exports_the_class_and_the_cfgs():
    import go2_sim2real_locomotion_rl_amd as pkg
    from go2_sim2real_locomotion_rl_amd.lidar import LidarScan

    assert pkg.LidarScan is LidarScan and "LidarScan" in pkg.__all__ and "get_stair_lidar_cfgs" in pkg.__all__
