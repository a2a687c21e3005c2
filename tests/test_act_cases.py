"""The case builders of tests/act_cases.py on the CPU: every case's condition holds at the seed the builder states, the swap reaches every reference
model and is undone afterwards, and a case with the condition violated is seen.  No GPU."""
import numpy as np
import pytest
import torch
from torch import nn

import act_cases as AC
import act_ref as AR
import distill_ref as DR
import ppo_ref as R


def test_swap_replaces_every_elu_and_is_undone():
    for name in AC.NEW_NAMES:
        with AC.swapped(name):
            for net in (R.mlp([3, 4, 5, 2]), DR.mlp([3, 4, 5, 2])):
                assert [type(m) for m in net] == [nn.Linear, AC.TORCH_ACT[name], nn.Linear, AC.TORCH_ACT[name], nn.Linear]
    assert [type(m) for m in R.mlp([3, 4, 2])] == [nn.Linear, nn.ELU, nn.Linear] and [type(m) for m in DR.mlp([3, 4, 2])] == [nn.Linear, nn.ELU, nn.Linear]


def test_zero_watch_agrees_with_the_numpy_margin_and_sees_a_zero():
    dims = [5, 7, 6, 2]
    g = torch.Generator().manual_seed(1)
    with AC.swapped("relu"):
        net = R.mlp(dims).double()
    x = torch.randn(9, 5, generator=g).double()
    watch = AC.ZeroWatch(net)
    net(x)
    watch.close()
    params = np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])
    assert watch.margin == pytest.approx(AR.zero_margin("relu", dims, params, x.numpy()), rel=1e-9) and watch.margin > 0
    with torch.no_grad():
        net[0].bias[0] = -float(net[0].weight[0] @ x[0])                      # one pre-activation at (the rounding of) zero
    watch = AC.ZeroWatch(net)
    net(x)
    assert watch.margin < 1.0


@pytest.mark.parametrize("shape", list(AC.FWD_DIMS_ALL))
@pytest.mark.parametrize("name", AC.NEW_NAMES)
def test_forward_cases_are_conditioned(name, shape):
    for rows in AC.FWD_ROWS:
        c = AC.fwd_case(name, shape, rows)
        pre = []
        AR.mlp64(name, c.dims, c.params, c.x, pre)
        assert AC.conditioned(name, pre) and np.isfinite(c.y64).all() and c.e32 > 0
        print(f"SEED fwd {name} {shape} {rows}: {c.seed} (start {AC.fwd_start(shape, rows)})")
        assert AC.yardstick_is_no_outlier(name, c.dims, c.params, c.x, pre, c.y64)
        assert AC.fwd_start(shape, rows) <= c.seed < AC.fwd_start(shape, rows) + (3 if c.y64.size >= 8 else 10)   # the few-sample condition passes 6 seeds in 10


@pytest.mark.parametrize("case", AC.PPO_GRAD_CASES, ids=AC.case_id)
def test_ppo_grad_cases_build(case):
    c = AC.ppo_grad_case(*case)
    start = 20000 + 101 * AC.PPO_GRAD_CASES.index(case)
    print(f"SEED ppo grad {AC.case_id(case)}: {c.seed} (start {start})")
    assert start <= c.seed < start + 3                                    # most first seeds pass; a walk of more than two would say the condition is too tight
    g64, g32 = c.ref["f64"][0], c.ref["f32"][0]
    assert all(float(g64[k].abs().max()) > 0 for k in g64) and set(g64) == set(g32)


@pytest.mark.parametrize("case", AC.PPO_UPDATE_CASES, ids=AC.case_id)
def test_ppo_update_cases_build(case):
    c = AC.ppo_update_case(*case)
    start = 40000 + 101 * AC.PPO_UPDATE_CASES.index(case)
    print(f"SEED ppo update {AC.case_id(case)}: {c.seed} (start {start})")
    assert start <= c.seed < start + 3
    assert all(float((c.f32["params"][k].double() - p).abs().max()) > 0 for k, p in c.f64["params"].items())


def test_recurrent_and_distillation_cases_build():
    r, ru, d, du = AC.rnn_grad_case(), AC.rnn_update_case(), AC.distill_grad_case(), AC.distill_update_case()
    print(f"SEED rnn {r.seed} {ru.seed} distill {d.seed} {du.seed}")
    assert (r.seed, ru.seed) == (61000, 62000) and 63000 <= d.seed < 63003 and 64000 <= du.seed < 64003
    assert len(r.adims) == 4 and len(du.f64["norms"]) == 2
