"""The HIP library's LIDAR scan (include/go2sim_lidar.h) against tests/lidar_ref.py over the cases of tests/lidar_cases.py: six consecutive steps with
resets, the curriculum level handed over through a device pointer; then what the header promises: the stored scan and the step counter round-trip,
equal calls on two streams give equal bits, poses are read through strides, the wider rows are assembled around the scans, a stale row is scaled
twice, a NaN pose stays inside the field, and refused calls touch nothing.  Every comparison with a bound prints the worst ratio first."""
import ctypes

import numpy as np
import pytest
import torch

import lidar_cases as LC
import lidar_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make_scanner(inp, n, **kw):
    from go2_sim2real_locomotion_rl_amd import LidarScan

    return LidarScan(inp["cfg"], n, LC.heightfield(), LC.H_SCALE, LC.V_SCALE, LC.ORIGIN, seed=inp["seed"], dr_schedule=inp["dr_schedule"],
                     curriculum_enabled=True, device=DEV, **kw)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def run_case(case, stats):
    """All steps of a case on the device, checked step by step against lidar_ref fed with the device's own stored scan: -> per-step (actor, both) bits"""
    inp = LC.case_inputs(case)
    n = inp["pos"].shape[1]
    scan = make_scanner(inp, n)
    lay = scan.layout
    level = torch.tensor([inp["level"]], dtype=torch.float64, device=DEV)
    L = R.dr_level(inp["level"], inp["dr_schedule"])
    outs = []
    assert scan.step_count == 0 and not scan.stored_scan().numpy().any()
    for t in range(LC.STEPS):
        prev = scan.stored_scan().numpy()
        actor, both = scan.scan(dev(inp["pos"][t]), dev(inp["quat"][t]), dev(inp["reset"][t]), level)
        actor, both = actor.cpu().numpy(), both.cpu().numpy()
        print(case[0], end=" ")
        LC.check_step(inp, lay, t, L, prev, actor, both, stats)
        assert np.array_equal(scan.stored_scan().numpy().view(np.uint32), actor.view(np.uint32)), "the stored scan is not the row's"
        assert scan.step_count == t + 1
        outs.append((actor, both))
    return outs


# ---- 1. the case table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LC.ENVS)
@pytest.mark.parametrize("grid", list(LC.GRIDS))
def test_six_steps_against_the_reference(grid, n):
    for case in LC.cases():
        if case[1] == grid and case[2] == n and case[6] == 1.0:
            stats = {}
            run_case(case, stats)
            print(f"{case[0]}: {stats}")
            assert stats["reset"] == 3
            if case[3] == "L0":                                       # L = 0: every randomisation is off, the actor scan is the clean one
                assert stats["dropout"] == stats["latency"] == stats["blackout"] == 0
            elif n == 67:                                             # enough draws for every branch
                assert min(stats["dropout"], stats["latency"], stats["blackout"], stats["clipped"]) > 0
                if grid != "1x1_none":
                    assert stats["stale_nonzero"] > 0


def test_half_scale_shows_the_double_scaling_of_stale_rows():
    case = [c for c in LC.cases() if c[6] == 0.5][0]
    inp = LC.case_inputs(case)
    stats = {}
    outs = run_case(case, stats)
    N = inp["cfg"]["noise"]
    seen = 0
    for t in range(1, LC.STEPS):
        d = R.draws(67, 15, inp["seed"], t)
        stale = (d["u_lat"].astype(np.float32) < R.threshold(N["latency_prob"], 1.0)) & ~(d["u_black"].astype(np.float32) < R.threshold(N["full_blackout_prob"], 1.0))
        for b in np.flatnonzero(stale & (inp["reset"][t] == 0)):
            prev = outs[t - 1][0][b]
            if prev.any():
                assert np.array_equal(outs[t][0][b], prev * np.float32(0.5))          # already clipped and scaled once: a quarter of the raw height
                seen += 1
    print(f"stale rows seen: {seen}")
    assert seen > 0


# ---- 2. state, determinism, layouts ------------------------------------------------------------------------------------------------------------
def test_stored_scan_and_step_counter_round_trip_and_replay():
    case = [c for c in LC.cases() if c[0] == "5x3_9x5-n5-L1"][0]
    inp = LC.case_inputs(case)
    scan = make_scanner(inp, 5)
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    x = np.random.default_rng(0).standard_normal((5, 15)).astype(np.float32)
    x[0, 0], x[1, 1] = -0.0, np.float32(1e-42)                       # a signed zero and a denormal keep their bits
    scan.set_stored_scan(x)
    assert np.array_equal(scan.stored_scan().numpy().view(np.uint32), x.view(np.uint32))
    scan.step_count = 0xFFFFFFFF
    assert scan.step_count == 0xFFFFFFFF
    args = (dev(inp["pos"][0]), dev(inp["quat"][0]), None, level)
    a1 = scan.scan(*args)[1].cpu().numpy()
    assert scan.step_count == 0                                       # the counter wraps as a uint32
    scan.step_count = 0xFFFFFFFF
    scan.set_stored_scan(x)
    a2 = scan.scan(*args)[1].cpu().numpy()
    assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)), "the same (state, inputs, step) did not give the same bits"
    scan.step_count = 7
    scan.set_stored_scan(x)
    a3 = scan.scan(*args)[1].cpu().numpy()
    assert not np.array_equal(a1[:, :15], a3[:, :15]) and np.array_equal(a1[:, 15:], a3[:, 15:])     # another step: other draws, the same clean scan
    # clear: an index list (entries outside the batch are passed over), then all
    scan.set_stored_scan(x)
    scan.clear(torch.tensor([3, 1, 99, -1], dtype=torch.int32, device=DEV))
    s = scan.stored_scan().numpy()
    assert not s[[1, 3]].any() and np.array_equal(s[[0, 2, 4]].view(np.uint32), x[[0, 2, 4]].view(np.uint32))
    scan.clear()
    assert not scan.stored_scan().numpy().any()


def test_equal_calls_on_two_streams_give_equal_bits():
    case = [c for c in LC.cases() if c[0] == "3x3_11x7-n67-L1"][0]
    inp = LC.case_inputs(case)
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    res = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            scan = make_scanner(inp, 67)
            outs = [scan.scan(dev(inp["pos"][t]), dev(inp["quat"][t]), dev(inp["reset"][t]), level)[1] for t in range(LC.STEPS)]
        s.synchronize()
        res.append([o.cpu().numpy().view(np.uint32) for o in outs])
    assert all(np.array_equal(a, b) for a, b in zip(*res))


def test_strided_poses_and_the_wider_rows():
    """The env's own layout -- components [3][n] / [4][n] apart, envs adjacent -- gives the bits of [n][3] / [n][4] rows; with inner rows the outputs are
    obs | actor scan and priv[0 .. n_in) | actor scan | priv[n_in .. n_in + 56) | critic scan, the scans being those of the call without inner rows."""
    case = [c for c in LC.cases() if c[0] == "5x3_9x5-n67-L1"][0]
    inp = LC.case_inputs(case)
    n, n_in, na, nc = 67, 49, 15, 45
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    pos, quat, reset = dev(inp["pos"][0]), dev(inp["quat"][0]), dev(inp["reset"][1])
    a = make_scanner(inp, n)
    actor, both = a.scan(pos, quat, reset, level)
    b = make_scanner(inp, n)
    pos_t, quat_t = pos.t().contiguous(), quat.t().contiguous()
    rng = np.random.default_rng(3)
    obs, priv = dev(rng.standard_normal((n, n_in)).astype(np.float32)), dev(rng.standard_normal((n, n_in + 56)).astype(np.float32))
    obs_out, priv_out = torch.full((n, n_in + na), 7.0, device=DEV), torch.full((n, n_in + na + 56 + nc), 7.0, device=DEV)
    b.step(pos_t, (n, 1), quat_t, (n, 1), reset, level, obs, priv, n_in, obs_out, priv_out)
    eq = lambda x, y: np.array_equal(x.contiguous().cpu().numpy().view(np.uint32), y.contiguous().cpu().numpy().view(np.uint32))
    assert eq(obs_out[:, :n_in], obs) and eq(obs_out[:, n_in:], actor)
    assert eq(priv_out[:, :n_in], priv[:, :n_in]) and eq(priv_out[:, n_in:n_in + na], actor)
    assert eq(priv_out[:, n_in + na:n_in + na + 56], priv[:, n_in:]) and eq(priv_out[:, n_in + na + 56:], both[:, na:])
    assert not actor[reset.bool()].any() and not both[reset.bool()].any()


def test_nan_and_infinite_poses_stay_inside_the_field():
    """The header's promise: a NaN or infinite x / y / quaternion selects a clamped index and the scan stays finite; a NaN z gives NaN scans."""
    case = [c for c in LC.cases() if c[0] == "5x3_9x5-n5-L0"][0]
    inp = LC.case_inputs(case)
    scan = make_scanner(inp, 5)
    level = torch.tensor([0.0], dtype=torch.float64, device=DEV)
    pos, quat = inp["pos"][0].copy(), inp["quat"][0].copy()
    pos[0, 0], pos[1, 1], pos[2, 0], quat[3, 0], pos[4, 2] = np.nan, np.inf, -np.inf, np.nan, np.nan
    actor, both = (x.cpu().numpy() for x in scan.scan(dev(pos), dev(quat), None, level))
    assert np.isfinite(both[:4]).all() and np.isnan(both[4]).all()
    hf = LC.heightfield().astype(np.float64) * LC.V_SCALE
    raw0 = np.clip(hf[0] - float(pos[0, 2]), -1.0, 1.0)                 # env 0: NaN x -> column index 0, whatever the row
    assert all(np.isclose(raw0, v, atol=1e-6).any() for v in both[0])


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_badarg_and_touch_nothing(hip_lib):
    from go2_sim2real_locomotion_rl_amd.capi import C
    from go2_sim2real_locomotion_rl_amd.lidar import LidarCfg

    BAD = C["GO2SIM_E_BADARG"]
    case = [c for c in LC.cases() if c[0] == "5x3_9x5-n5-L1"][0]
    inp = LC.case_inputs(case)
    n, n_in, na, nc = 5, 49, 15, 45
    scan = make_scanner(inp, n)
    x = np.random.default_rng(1).standard_normal((n, na)).astype(np.float32)
    scan.set_stored_scan(x)
    scan.step_count = 3
    level = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    pos, quat = dev(inp["pos"][0]), dev(inp["quat"][0])
    obs, priv = torch.full((n, n_in), 5.0, device=DEV), torch.full((n, n_in + 56), 5.0, device=DEV)
    obs_out, priv_out = torch.full((n, n_in + na), 7.0, device=DEV), torch.full((n, n_in + na + 56 + nc), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    LL = ctypes.c_longlong
    step = hip_lib.fn("lidar_step")

    def call(h=scan.h, n_=n, pos_=pos, quat_=quat, level_=level, obs_=obs, priv_=priv, n_in_=n_in, oo=obs_out, po=priv_out):
        return step(h, ctypes.c_int(n_), p(pos_), LL(1), LL(3), p(quat_), LL(1), LL(4), None, p(level_), p(obs_), p(priv_), ctypes.c_int(n_in_), p(oo), p(po), None)

    refused = {"NULL handle": call(h=None), "n mismatch": call(n_=n - 1), "n too large": call(n_=n + 1), "outer == inner (obs)": call(oo=obs),
               "outer == inner (priv)": call(po=priv), "outer crossed": call(oo=priv), "both outputs the same": call(po=obs_out), "NULL pos": call(pos_=None),
               "NULL quat": call(quat_=None), "NULL output": call(oo=None), "NULL level with the curriculum on": call(level_=None),
               "one inner row": call(priv_=None), "inner rows without a width": call(n_in_=0), "a width without inner rows": call(obs_=None, priv_=None)}
    print(refused)
    assert all(rc == BAD for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((obs_out == 7.0).all()) and bool((priv_out == 7.0).all()) and bool((obs == 5.0).all()) and bool((priv == 5.0).all())
    assert scan.step_count == 3 and np.array_equal(scan.stored_scan().numpy().view(np.uint32), x.view(np.uint32))
    assert call() == 0 and scan.step_count == 4                        # the same arguments, unrefused

    # no point on either side, and the other refusals of create
    lay = scan.layout
    hf = LC.heightfield()

    def create(**kw):
        c = LidarCfg()
        vals = dict(height_clip=1.0, height_scale=1.0, horizontal_scale=LC.H_SCALE, vertical_scale=LC.V_SCALE, n_envs=n, n_actor=na, n_critic=nc, hf_rows=LC.ROWS,
                    hf_cols=LC.COLS)
        vals.update(kw)
        for k, v in vals.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        rc = hip_lib.fn("lidar_create")(ctypes.c_int(0), ctypes.byref(c), hf.ctypes.data_as(ctypes.c_void_p), lay["actor_xy"].ctypes.data_as(ctypes.c_void_p),
                                        lay["critic_xy"].ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(1), ctypes.byref(h))
        if rc == 0:
            hip_lib.fn("lidar_destroy")(h)
        return rc, h.value

    assert create()[0] == 0
    for kw in (dict(n_actor=0, n_critic=0), dict(n_envs=0), dict(n_actor=-1), dict(hf_rows=0), dict(horizontal_scale=0.0), dict(height_clip=-1.0),
               dict(height_scale=float("nan"))):
        rc, h = create(**kw)
        assert rc == BAD and not h, kw
    for name in ("lidar_destroy",):
        assert hip_lib.fn(name)(None) == BAD
    assert hip_lib.fn("lidar_clear")(None, None, ctypes.c_int(0), None) == BAD
    assert hip_lib.fn("lidar_get_step")(scan.h, None) == BAD and hip_lib.fn("lidar_get_scan")(scan.h, None, None) == BAD
