"""The HIP library's stair info (include/go2sim_stairinfo.h) against tests/stairinfo_ref.py over the cases of tests/stairinfo_cases.py: six consecutive
steps with resets from the library's own stored rows, the curriculum level handed over through a device pointer, 2 / 14 / 64 samples, 1 / 5 / 67 envs;
then what the header promises: the stored rows and the step counter round-trip, replay, equal calls on two streams give equal bits, poses are read
through strides, the wider rows are assembled around the fours, a stale edge is divided and multiplied, terrain rows are read at step time, a NaN
pose stays inside the field, and refused calls touch nothing.  Every comparison with a bound prints the worst ratio first.

Measured on the MI355X: worst ratio 0.90 over all tables (entries that round once are held to one rounding), 0 ambiguous env-steps of 6060 (the CPU test
holds the tables under 1 %), all 160 stale edges equal to numpy's float32 (stored / s) * s bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import stairinfo_cases as SC
import stairinfo_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make_info(inp, n, **kw):
    from go2_sim2real_locomotion_rl_amd import StairInfo

    P, info = inp["P"], inp["info"]
    args = dict(seed=inp["seed"], dr_schedule=inp["dr_schedule"], curriculum_enabled=True, device=DEV)
    args.update(kw)
    return StairInfo(inp["cfg"], n, P["hf"], P["h_scale"], P["v_scale"], P["origin"], info["step_heights_m"], info["step_depths_m"], **args)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def run_case(case, stats):
    """All steps of a case on the device, checked step by step against stairinfo_ref fed with the device's own stored rows: -> per-step (actor, both)"""
    inp = SC.case_inputs(case)
    n = inp["pos"].shape[1]
    si = make_info(inp, n)
    level = torch.tensor([inp["level"]], dtype=torch.float64, device=DEV)
    L = R.dr_level(inp["level"], inp["dr_schedule"])
    outs = []
    assert si.step_count == 0 and not si.stored_rows().numpy().any()
    for t in range(SC.STEPS):
        prev = si.stored_rows().numpy()
        actor, both = si.info(dev(inp["pos"][t]), dev(inp["quat"][t]), dev(inp["rows"][t]), dev(inp["reset"][t]), level)
        actor, both = actor.cpu().numpy(), both.cpu().numpy()
        print(case[0], end=" ")
        SC.check_step(inp, t, L, prev, actor, both, stats)
        assert np.array_equal(si.stored_rows().numpy().view(np.uint32), actor.view(np.uint32)), "the stored row is not the actor row"
        assert si.step_count == t + 1
        outs.append((actor, both))
    return inp, outs


# ---- 1. the case table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.ENVS)
@pytest.mark.parametrize("ns", SC.SAMPLES)
def test_six_steps_against_the_reference(ns, n):
    for case in SC.cases():
        if case[1] == ns and case[2] == n and case[6] == 3.7 and case[8] == 0.02:
            stats = {}
            run_case(case, stats)
            print(f"{case[0]}: {stats}")
            assert stats["reset"] == 3 and stats["ambiguous"] <= 0.01 * stats["env_steps"] + (1 if n < 67 else 0)
            if case[3] == "L0":                                       # L = 0: every degradation is off, the actor four are the clean four
                assert stats["flip"] == stats["latency"] == stats["blackout"] == 0
            elif n == 67:                                             # enough draws for every branch
                assert min(stats["flip"], stats["latency"], stats["blackout"], stats["stale_nonzero"], stats["up"], stats["down"], stats["none"]) > 0
                assert stats["clamped_hi"] > 0 and (ns == 2 or stats["clamped_lo"] > 0)
            if n == 67:
                sp = stats["special"]
                mr = np.float32(np.float32(0.27) * np.float32(3.7))
                assert sp["up"][1] == 1 and sp["down"][1] == -1 and sp["row_boundary"][1] == 1 and sp["row_boundary_down"][1] == -1
                assert sp["none"] == (mr, 0) and sp["last_pair"][1] == 1 and sp["last_pair"][0] < mr
                assert sp["yaw_pi_plus"][1] == -1 and sp["yaw_pi_minus"][1] == -1
                if ns > 2:                                            # two samples 0.27 m apart straddle several risers of row 0
                    assert sp["threshold_first"] == (mr, 0) and sp["threshold_second"] == (mr, 0) and sp["threshold_third"] == (mr, 0)
                # beyond the x edges the clamped column is flat ground; beyond the y edges the clamped row's own stairs stay in view
                assert sp["beyond_x_lo"] == (mr, 0) and sp["beyond_x_hi"] == (mr, 0)


def test_threshold_riser_on_the_other_side():
    """threshold 0.105 = row 3's riser: its first two steps are no edges, the third is one by the float32 rounding of 63 and 42 units"""
    case = [c for c in SC.cases() if c[0] == "s14-n67-L1-thr105"][0]
    stats = {}
    run_case(case, stats)
    print(stats)
    sp = stats["special"]
    mr = np.float32(np.float32(0.27) * np.float32(3.7))
    assert sp["threshold_first"] == (mr, 0) and sp["threshold_third"][1] == 1 and sp["threshold_third"][0] < mr


def test_scale_one_and_scale_37_on_a_stale_row():
    """A stale edge is stored / s_e * s_e: with s_e = 1 the stored bits repeat, with 3.7 the float32 divide-then-multiply (stairinfo_ref holds it to
    2 ulp; whether the bits are numpy's is printed)."""
    seen = {}
    for name in ("s14-n67-L1-scale1", "s14-n67-L1"):
        case = [c for c in SC.cases() if c[0] == name][0]
        inp, outs = run_case(case, {})
        s = np.float32(case[6])
        N = inp["N"]
        cnt = same = 0
        for t in range(1, SC.STEPS):
            m = R.masks_of(N, 1.0, R.draws(67, inp["seed"], t), inp["reset"][t])
            for b in np.flatnonzero(m["latency"] & ~m["blackout"]):
                prev, now = outs[t - 1][0][b], outs[t][0][b]
                if prev[0] != 0:
                    if case[6] == 1.0:
                        assert now[0].view(np.uint32) == prev[0].view(np.uint32) and now[3].view(np.uint32) == prev[3].view(np.uint32)
                    assert abs(float(now[0]) - float(prev[0])) <= 2.0 * R.U * abs(float(prev[0]))
                    same += int(now[0] == np.float32(np.float32(prev[0] / s) * s))
                    cnt += 1
        print(f"{name}: {cnt} stale rows with a non-zero edge, {same} equal numpy's float32 (stored / s) * s bit for bit")
        seen[name] = cnt
    assert min(seen.values()) > 0, seen


# ---- 2. state, determinism, layouts ------------------------------------------------------------------------------------------------------------
def test_stored_rows_and_step_counter_round_trip_and_replay():
    case = [c for c in SC.cases() if c[0] == "s14-n5-L1"][0]
    inp = SC.case_inputs(case)
    si = make_info(inp, 5)
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    x = np.random.default_rng(0).standard_normal((5, 4)).astype(np.float32)
    x[0, 0], x[1, 1] = -0.0, np.float32(1e-42)                       # a signed zero and a denormal keep their bits
    si.set_stored_rows(x)
    assert np.array_equal(si.stored_rows().numpy().view(np.uint32), x.view(np.uint32))
    si.step_count = 0xFFFFFFFF
    assert si.step_count == 0xFFFFFFFF
    args = (dev(inp["pos"][0]), dev(inp["quat"][0]), dev(inp["rows"][0]), None, level)
    a1 = si.info(*args)[1].cpu().numpy()
    assert si.step_count == 0                                         # the counter wraps as a uint32
    si.step_count = 0xFFFFFFFF
    si.set_stored_rows(x)
    a2 = si.info(*args)[1].cpu().numpy()
    assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)), "the same (state, inputs, step) did not give the same bits"
    si.step_count = 7
    si.set_stored_rows(x)
    a3 = si.info(*args)[1].cpu().numpy()
    assert not np.array_equal(a1[:, :4], a3[:, :4]) and np.array_equal(a1[:, 4:], a3[:, 4:])     # another step: other draws, the same clean four
    # clear: an index list (entries outside the batch are passed over), then all
    si.set_stored_rows(x)
    si.clear(torch.tensor([3, 1, 99, -1], dtype=torch.int32, device=DEV))
    s = si.stored_rows().numpy()
    assert not s[[1, 3]].any() and np.array_equal(s[[0, 2, 4]].view(np.uint32), x[[0, 2, 4]].view(np.uint32))
    si.clear()
    assert not si.stored_rows().numpy().any()


def test_equal_calls_on_two_streams_give_equal_bits():
    case = [c for c in SC.cases() if c[0] == "s64-n67-L1"][0]
    inp = SC.case_inputs(case)
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    res = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            si = make_info(inp, 67)
            outs = [si.info(dev(inp["pos"][t]), dev(inp["quat"][t]), dev(inp["rows"][t]), dev(inp["reset"][t]), level)[1] for t in range(SC.STEPS)]
        s.synchronize()
        res.append([o.cpu().numpy().view(np.uint32) for o in outs])
    assert all(np.array_equal(a, b) for a, b in zip(*res))


def test_strided_poses_and_the_wider_rows():
    """The env's own layout -- components [3][n] / [4][n] apart, envs adjacent -- gives the bits of [n][3] / [n][4] rows; with inner rows the outputs are
    obs | actor four and priv[0 .. n_in) | actor four | priv[n_in .. n_in + 56) | clean four, the fours being those of the call without inner rows."""
    case = [c for c in SC.cases() if c[0] == "s14-n67-L1"][0]
    inp = SC.case_inputs(case)
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    pos, quat, rows, reset = dev(inp["pos"][0]), dev(inp["quat"][0]), dev(inp["rows"][0]), dev(inp["reset"][1])
    eq = lambda x, y: np.array_equal(x.contiguous().cpu().numpy().view(np.uint32), y.contiguous().cpu().numpy().view(np.uint32))
    rng = np.random.default_rng(3)
    n = 67
    a = make_info(inp, n)
    actor, both = a.info(pos, quat, rows, reset, level)
    for n_in in (49, 45, 70):                                          # 70: more inner columns than a wavefront has lanes
        b = make_info(inp, n)
        pos_t, quat_t = pos.t().contiguous(), quat.t().contiguous()
        obs, priv = dev(rng.standard_normal((n, n_in)).astype(np.float32)), dev(rng.standard_normal((n, n_in + 56)).astype(np.float32))
        obs_out, priv_out = torch.full((n, n_in + 4), 7.0, device=DEV), torch.full((n, n_in + 64), 7.0, device=DEV)
        b.step(pos_t, (n, 1), quat_t, (n, 1), rows, reset, level, obs, priv, n_in, obs_out, priv_out)
        assert eq(obs_out[:, :n_in], obs) and eq(obs_out[:, n_in:], actor)
        assert eq(priv_out[:, :n_in], priv[:, :n_in]) and eq(priv_out[:, n_in:n_in + 4], actor)
        assert eq(priv_out[:, n_in + 4:n_in + 60], priv[:, n_in:]) and eq(priv_out[:, n_in + 60:], both[:, 4:])
    assert not actor[reset.bool()].any() and not both[reset.bool()].any()


def test_terrain_rows_are_read_at_step_time():
    """Rows changed between steps (what set_terrain_rows does to the env's buffer) change height and depth of the next step, and only them; rows
    outside the table are clamped."""
    case = [c for c in SC.cases() if c[0] == "s14-n5-L0"][0]
    inp = SC.case_inputs(case)
    si = make_info(inp, 5)
    level = torch.tensor([0.0], dtype=torch.float64, device=DEV)
    rows = torch.tensor([0, 1, 2, 3, 0], dtype=torch.int32, device=DEV)
    pos, quat = dev(inp["pos"][0]), dev(inp["quat"][0])
    h32, d32 = inp["N"]["row_heights"], inp["N"]["row_depths"]
    a = si.info(pos, quat, rows, None, level)[1].cpu().numpy()
    rows.copy_(torch.tensor([3, 2, 1, -4, 99], dtype=torch.int32))      # in place: the same device buffer
    b = si.info(pos, quat, rows, None, level)[1].cpu().numpy()
    for out, r in ((a, [0, 1, 2, 3, 0]), (b, [3, 2, 1, 0, 3])):
        assert np.array_equal(out[:, 5], h32[r] * np.float32(5.0)) and np.array_equal(out[:, 6], d32[r] * np.float32(3.3))
        assert np.array_equal(out[:, :4].view(np.uint32), out[:, 4:].view(np.uint32))                # L = 0: the actor four are the clean four
    assert np.array_equal(a[:, [4, 7]], b[:, [4, 7]])


def test_nan_and_infinite_poses_stay_inside_the_field():
    """The header's promise: a NaN or infinite x / y / quaternion selects clamped indices and all eight outputs stay finite; z is not read."""
    case = [c for c in SC.cases() if c[0] == "s14-n5-L1"][0]
    inp = SC.case_inputs(case)
    si = make_info(inp, 5)
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    pos, quat = inp["pos"][0].copy(), inp["quat"][0].copy()
    pos[0, 0], pos[1, 1], pos[2, 0], quat[3, 0], pos[4, 2] = np.nan, np.inf, -np.inf, np.nan, np.nan
    quat[2, 3] = np.inf
    actor, both = (x.cpu().numpy() for x in si.info(dev(pos), dev(quat), dev(inp["rows"][0]), None, level))
    assert np.isfinite(both).all() and np.isfinite(actor).all()
    top = np.float32(np.float32(0.27) * np.float32(3.7))
    assert (np.abs(both[:, 7]) <= 1).all() and (both[:, 4] >= 0).all() and (both[:, 4] <= top).all()
    assert both[3, 7] == 0 and both[3, 4] == top                    # a NaN yaw puts every sample on cell (0, 0): no edge


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_badarg_and_touch_nothing(hip_lib):
    from go2_sim2real_locomotion_rl_amd.capi import C
    from go2_sim2real_locomotion_rl_amd.stairinfo import StairInfoCfg

    BAD = C["GO2SIM_E_BADARG"]
    case = [c for c in SC.cases() if c[0] == "s14-n5-L1"][0]
    inp = SC.case_inputs(case)
    n, n_in = 5, 49
    si = make_info(inp, n)
    x = np.random.default_rng(1).standard_normal((n, 4)).astype(np.float32)
    si.set_stored_rows(x)
    si.step_count = 3
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    pos, quat, rows = dev(inp["pos"][0]), dev(inp["quat"][0]), dev(inp["rows"][0])
    obs, priv = torch.full((n, n_in), 5.0, device=DEV), torch.full((n, n_in + 56), 5.0, device=DEV)
    obs_out, priv_out = torch.full((n, n_in + 4), 7.0, device=DEV), torch.full((n, n_in + 64), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    LL = ctypes.c_longlong
    step = hip_lib.fn("stairinfo_step")

    def call(h=si.h, n_=n, pos_=pos, quat_=quat, rows_=rows, level_=level, obs_=obs, priv_=priv, n_in_=n_in, oo=obs_out, po=priv_out, ps=1):
        return step(h, ctypes.c_int(n_), p(pos_), LL(ps), LL(3), p(quat_), LL(1), LL(4), p(rows_), None, p(level_), p(obs_), p(priv_), ctypes.c_int(n_in_),
                    p(oo), p(po), None)

    refused = {"NULL handle": call(h=None), "n mismatch": call(n_=n - 1), "n too large": call(n_=n + 1), "outer == inner (obs)": call(oo=obs),
               "outer == inner (priv)": call(po=priv), "outer crossed": call(oo=priv), "both outputs the same": call(po=obs_out), "NULL pos": call(pos_=None),
               "NULL quat": call(quat_=None), "NULL output": call(oo=None), "NULL level with the curriculum on": call(level_=None),
               "NULL rows with four rows": call(rows_=None), "a negative stride": call(ps=-1),
               "one inner row": call(priv_=None), "inner rows without a width": call(n_in_=0), "a width without inner rows": call(obs_=None, priv_=None)}
    print(refused)
    assert all(rc == BAD for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((obs_out == 7.0).all()) and bool((priv_out == 7.0).all()) and bool((obs == 5.0).all()) and bool((priv == 5.0).all())
    assert si.step_count == 3 and np.array_equal(si.stored_rows().numpy().view(np.uint32), x.view(np.uint32))
    assert call() == 0 and si.step_count == 4                          # the same arguments, unrefused

    # the refusals of create
    P, info, lay = inp["P"], inp["info"], si.layout
    hf = np.ascontiguousarray(P["hf"], np.int16)
    xs64 = np.linspace(0, 0.27, 65).astype(np.float32)

    def create(**kw):
        c = StairInfoCfg()
        vals = dict(max_range=0.27, threshold=0.02, edge_dist_scale=3.7, height_scale=5.0, depth_scale=3.3, direction_scale=1.0, horizontal_scale=P["h_scale"],
                    vertical_scale=P["v_scale"], n_envs=n, n_samples=14, n_rows=4, hf_rows=hf.shape[0], hf_cols=hf.shape[1])
        vals.update(kw)
        for k, v in vals.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        rc = hip_lib.fn("stairinfo_create")(ctypes.c_int(0), ctypes.byref(c), hf.ctypes.data_as(ctypes.c_void_p), xs64.ctypes.data_as(ctypes.c_void_p),
                                            si.row_heights.ctypes.data_as(ctypes.c_void_p), si.row_depths.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(1),
                                            ctypes.byref(h))
        if rc == 0:
            hip_lib.fn("stairinfo_destroy")(h)
        return rc, h.value

    assert create()[0] == 0 and create(n_samples=2)[0] == 0 and create(n_samples=64)[0] == 0 and create(threshold=0.0, max_range=0.0)[0] == 0
    for kw in (dict(n_samples=1), dict(n_samples=65), dict(n_samples=0), dict(max_range=-0.1), dict(max_range=float("inf")), dict(max_range=float("nan")),
               dict(threshold=-0.01), dict(threshold=float("inf")), dict(threshold=float("nan")), dict(n_envs=0), dict(n_rows=0), dict(n_rows=17),
               dict(hf_rows=0), dict(horizontal_scale=0.0), dict(edge_dist_scale=float("nan")), dict(latency_prob=float("nan"))):
        rc, h = create(**kw)
        assert rc == BAD and not h, kw
    assert hip_lib.fn("stairinfo_destroy")(None) == BAD
    assert hip_lib.fn("stairinfo_clear")(None, None, ctypes.c_int(0), None) == BAD
    assert hip_lib.fn("stairinfo_get_step")(si.h, None) == BAD and hip_lib.fn("stairinfo_get_state")(si.h, None, None) == BAD
    assert hip_lib.fn("stairinfo_set_state")(si.h, None, None) == BAD and hip_lib.fn("stairinfo_env_rows")(None, None) == BAD
    # and the Python layer's own: a layout the library would refuse, mismatched tables
    from go2_sim2real_locomotion_rl_amd import Go2SimError, StairInfo

    with pytest.raises(Go2SimError, match="num_samples"):
        StairInfo(SC.stair_info_cfg(65), n, hf, P["h_scale"], P["v_scale"], P["origin"], info["step_heights_m"], info["step_depths_m"], device=DEV)
    with pytest.raises(Go2SimError, match="two lists of one length"):
        StairInfo(SC.stair_info_cfg(14), n, hf, P["h_scale"], P["v_scale"], P["origin"], info["step_heights_m"], info["step_depths_m"][:3], device=DEV)
