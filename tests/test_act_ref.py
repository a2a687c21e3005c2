"""tests/act_ref.py against torch in float64: every activation equals the torch module rsl_rl's resolve_nn_activation maps its name to, the
derivative written on the post-activation equals autograd's, and the `elu` column is the network of tests/policy_ref.py.  No GPU."""
import numpy as np
import pytest
import torch

import act_ref as AR
import policy_ref as PR

TORCH_ACT = {"elu": torch.nn.ELU, "selu": torch.nn.SELU, "relu": torch.nn.ReLU, "lrelu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh,
             "sigmoid": torch.nn.Sigmoid, "identity": torch.nn.Identity}
TINY = float(np.finfo(np.float64).tiny)
EDGES = [0.0, -0.0, TINY, -TINY, 1e-300, -1e-300, 1e-10, -1e-10, 20.0, -20.0, 100.0, -100.0, float("inf"), float("-inf"), float("nan")]
SWEEP = np.concatenate([np.asarray(EDGES), np.linspace(-30.0, 30.0, 2401), np.random.default_rng(3).standard_normal(500) * 3.0])


def test_the_seven_names():
    assert set(AR.NAMES) == set(TORCH_ACT) and len(AR.NAMES) == 7
    assert set(AR.BOUND_ABS) == set(AR.BOUND_REL) == set(AR.NAMES)


@pytest.mark.parametrize("name", AR.NAMES)
def test_act64_is_the_torch_module(name):
    want = TORCH_ACT[name]()(torch.from_numpy(SWEEP.copy())).numpy()
    got = AR.act64(name, SWEEP)
    assert got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    rel = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-320)
    rel[got[fin] == want[fin]] = 0.0
    print(f"RATIO act64 {name} worst relative difference {rel.max():.3e}")
    assert rel.max() <= 1e-15


def test_the_non_finite_table():
    inf, nan = float("inf"), float("nan")
    LA = AR.SELU_L * AR.SELU_A
    for name in AR.NAMES:
        assert np.isnan(AR.act64(name, np.float64([nan]))[0]), name            # relu(NaN) is NaN, not 0
    a = lambda name, v: float(AR.act64(name, np.float64([v]))[0])
    assert a("relu", -inf) == 0.0 and a("lrelu", -inf) == -inf and a("tanh", inf) == 1.0 and a("tanh", -inf) == -1.0
    assert a("sigmoid", -inf) == 0.0 and a("sigmoid", inf) == 1.0 and a("selu", -inf) == -LA and a("elu", -inf) == -1.0
    for name in ("elu", "selu", "relu", "lrelu", "identity"):
        assert a(name, inf) == inf
    assert a("sigmoid", 0.0) == 0.5                                            # why the padded columns are stored as 0, not as f(0)


@pytest.mark.parametrize("name", AR.NAMES)
def test_derivative_from_the_post_activation_is_autograds(name):
    v = SWEEP[np.isfinite(SWEEP)]
    x = torch.from_numpy(v.copy()).requires_grad_(True)
    TORCH_ACT[name]()(x).sum().backward()
    want = x.grad.numpy()
    got = AR.dact64_from_a(name, AR.act64(name, v))
    # a + L A (and a + 1, 1 - a a, a (1 - a)) carry the rounding of a: an absolute error of a few 2^-53 of the function's scale, whatever the size of
    # the derivative itself
    scale = AR.SELU_L * AR.SELU_A if name == "selu" else 1.0
    err = np.abs(got - want).max() / scale
    print(f"RATIO dact64 {name} worst absolute difference / scale {err:.3e}")
    assert err <= 1e-15
    at0 = float(AR.dact64_from_a(name, AR.act64(name, np.float64([0.0])))[0])
    assert at0 == {"elu": 1.0, "selu": AR.SELU_L * AR.SELU_A, "relu": 0.0, "lrelu": 0.01, "tanh": 1.0, "sigmoid": 0.25, "identity": 1.0}[name]
    assert at0 == float(want[np.flatnonzero(v == 0.0)[0]])


def test_elu_column_is_the_policy_reference():
    rng = np.random.default_rng(5)
    dims = [19, 24, 40, 8]
    params = (rng.standard_normal(sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))) / 4).astype(np.float32)
    x = rng.standard_normal((37, dims[0])).astype(np.float32)
    pre_a, pre_p = [], []
    assert np.array_equal(AR.mlp64("elu", dims, params, x, pre_a), PR.mlp64(dims, params, x, pre_p))
    assert all(np.array_equal(p, q) for p, q in zip(pre_a, pre_p)) and len(pre_a) == 3
    assert np.array_equal(AR.mlp32_plain("elu", dims, params, x), PR.mlp32_plain(dims, params, x))
    assert AR.mlp_yardstick("elu", dims, params, x)[1] == PR.mlp_yardstick(dims, params, x)[1]
    assert AR.BOUND_ABS["elu"] == PR.ELU_ABS and AR.U24 == PR.U24


def test_zero_margin_sees_a_pre_activation_at_zero():
    dims = [2, 2, 1]
    params = np.float32([1, -1, 1, 1, 0, 0, 1, 1, 0])                         # hidden 0 = x0 - x1, hidden 1 = x0 + x1
    assert AR.zero_margin("relu", dims, params, np.float32([[1.0, 1.0]])) == 0.0
    assert AR.zero_margin("relu", dims, params, np.float32([[1.0, 0.5]])) > 1.0
    assert AR.zero_margin("relu", [3, 2], np.zeros(8, np.float32), np.zeros((1, 3), np.float32)) == np.inf
