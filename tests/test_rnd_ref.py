"""The random-network-distillation reference (tests/rnd_ref.py) against itself, on the CPU: the MSE gradient against its closed form, the three weight
schedules at their corners, the reward normaliser's one-column fold against a direct float64 variance of everything it has seen, and the std == 0 branch.
The product's pure schedule function (rnd.rnd_weight) is held to the reference's at the same corners."""
import numpy as np
import pytest
import torch

import norm_ref as NR
import rnd_cases as RC
import rnd_ref as R


@pytest.mark.parametrize("case", [c for c in RC.GRAD_CASES if c[1] <= 37], ids=RC.case_id)
def test_mse_gradient_is_the_closed_form(case):
    c = RC.get_grad_case(*case)
    ref = c.ref["f64"]
    n, E = c.n, c.pdims[-1]
    closed = 2.0 * (ref["p"] - ref["t"]) / (n * E)
    err = float((ref["dp"] - closed).abs().max())
    print(f"closed form {RC.case_id(case)} max|dL/dp - 2(p-t)/(nE)| = {err:.3e}")
    assert err <= 1e-15 * max(1.0, float(closed.abs().max()))
    assert ref["loss"] == pytest.approx(float(((ref["p"] - ref["t"]) ** 2).mean()), rel=1e-14)
    # the last layer's bias gradient is the column sum of dL/dp
    last = f"predictor.{2 * (len(c.pdims) - 2)}.bias"
    assert torch.allclose(ref["grads"][last], closed.sum(0), rtol=1e-12, atol=1e-18)


LINEAR = {"mode": "linear", "initial_step": 10, "final_step": 30, "final_value": 0.5}
STEP = {"mode": "step", "final_step": 20, "final_value": 0.25}
W0 = 2.0
CORNERS = [(None, 7, W0), ({"mode": "constant"}, 10 ** 6, W0),
           (LINEAR, 9, W0), (LINEAR, 10, W0), (LINEAR, 20, W0 + (0.5 - W0) * 0.5), (LINEAR, 30, 0.5), (LINEAR, 31, 0.5),
           (STEP, 19, W0), (STEP, 20, 0.25), (STEP, 21, 0.25)]


@pytest.mark.parametrize("schedule,counter,want", CORNERS)
def test_weight_schedules_at_their_corners(schedule, counter, want):
    from go2_sim2real_locomotion_rl_amd.rnd import rnd_weight

    got = R.weight(W0, schedule, counter)
    print(f"schedule {schedule} counter {counter}: {got}")
    assert got == want
    assert rnd_weight(W0, schedule, counter) == got


def test_linear_schedule_is_monotone_between_its_ends():
    w = [R.weight(W0, LINEAR, k) for k in range(5, 40)]
    assert all(a >= b for a, b in zip(w, w[1:])) and w[0] == W0 and w[-1] == 0.5


@pytest.mark.parametrize("n", [17, 257, 1000])
def test_reward_fold_is_the_variance_of_everything_seen(n):
    """K steps of the one-column fold against np.var of all K n values of avg; the only differences are the float32 roundings of the stored state"""
    rng = np.random.default_rng(n)
    norm, seen = R.RewardNormalizer(n), []
    for k in range(8):
        r = np.abs(rng.standard_normal(n)).astype(np.float32) + np.float32(0.1)
        avg_before = norm.avg.copy()
        out = norm(r)
        assert np.array_equal(norm.avg.view(np.int32), ((np.float32(0.99) * avg_before).astype(np.float32) + r).view(np.int32))
        seen.append(norm.avg.astype(np.float64))
        allv = np.concatenate(seen)
        # the initial state (mean 0, var 1, count 0) has weight zero after the first fold
        mean, var = float(norm.state["mean"][0]), float(norm.state["var"][0])
        print(f"fold n={n} step {k}: mean {mean:.9g} vs {allv.mean():.9g}, var {var:.9g} vs {allv.var():.9g}")
        assert norm.state["count"] == (k + 1) * n
        assert mean == pytest.approx(allv.mean(), rel=(k + 2) * 2 * NR.U32) and var == pytest.approx(allv.var(), rel=(k + 2) * 8 * NR.U32)
        assert float(norm.state["std"][0]) == pytest.approx(np.sqrt(allv.var()), rel=(k + 2) * 8 * NR.U32)
        assert np.array_equal(out.view(np.int32), (r / norm.state["std"][0]).astype(np.float32).view(np.int32))


def test_std_zero_leaves_the_reward_unchanged():
    """N = 1: the first fold has var_b = 0 and rate = 1, so var' = 1 + (0 - 1 + dm (mean_b - mean')) with mean' = mean_b: exactly 0, std = 0"""
    norm = R.RewardNormalizer(1)
    r = np.array([0.37], np.float32)
    out = norm(r)
    assert norm.state["var"][0] == 0.0 and norm.state["std"][0] == 0.0 and norm.state["count"] == 1
    assert np.array_equal(out.view(np.int32), r.view(np.int32))
    intrinsic, total = R.finish(r, norm.state["std"][0], 0.5, np.array([1.0], np.float32))
    assert intrinsic[0] == np.float32(0.5) * r[0] and total[0] == np.float32(1.0) + intrinsic[0]
    out2 = norm(r)                                              # the second value of avg differs from the first: var' > 0 from here on
    assert norm.state["std"][0] > 0 and out2[0] == r[0] / norm.state["std"][0]


def test_distance_is_rounded_once():
    rng = np.random.default_rng(3)
    t, p = rng.standard_normal((37, 12)).astype(np.float32), rng.standard_normal((37, 12)).astype(np.float32)
    r64 = R.distance64(t, p)
    assert np.allclose(r64, np.linalg.norm(t.astype(np.float64) - p.astype(np.float64), axis=1), rtol=1e-15)
    assert (np.abs(r64.astype(np.float32).astype(np.float64) - r64) <= NR.U32 * r64).all()
