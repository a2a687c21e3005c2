"""The float64 reference of the PPO update (tests/ppo_ref.py: torch autograd, clip_grad_norm_, Adam) against things it shares no code with:
central finite differences of its loss, the closed forms of the loss head written out by hand, and the learning-rate rule's five outcomes."""
import math

import pytest
import torch

import ppo_cases as PC
import ppo_ref as R

ADIMS, CDIMS, ROWS = [5, 7, 3], [6, 7, 1], 24


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    state = PC.init_state(ADIMS, CDIMS, g)
    ro = PC.make_rollout(ADIMS, CDIMS, state, ROWS, "keep", 6)
    return state, {k: x.double() for k, x in ro.items()}


def test_gradients_equal_central_differences(case):
    """every parameter of the [5, 7, 3] / [6, 7, 1] pair, relative 1e-6 of the tensor's largest gradient"""
    state, mb = case
    m = R.make_model(ADIMS, CDIMS, state, torch.float64)
    grads, _ = R.minibatch_grad(m, mb)
    h = 1e-6
    with torch.no_grad():
        for k, p in R.ordered_params(m):
            fd = torch.zeros_like(p)
            pv, fv = p.view(-1), fd.view(-1)
            for i in range(pv.numel()):
                x = float(pv[i])
                pv[i] = x + h; lp = float(R.loss_terms(m, mb)[0])
                pv[i] = x - h; lm = float(R.loss_terms(m, mb)[0])
                pv[i] = x
                fv[i] = (lp - lm) / (2 * h)
            err, scale = float((fd - grads[k]).abs().max()), float(grads[k].abs().max())
            assert err <= 1e-6 * scale, (k, err, scale)


def closed_form_head(mu, sigma, v, mb, hp=R.HP):
    """d loss / d mu [n][A], d loss / d sigma [A], d loss / d v [n] in the issue's terms, no autograd"""
    n = mu.shape[0]
    a, adv, clip = mb["actions"], mb["advantages"], hp["clip_param"]
    logp = (-(a - mu) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - math.log(math.sqrt(2 * math.pi))).sum(-1)
    ratio = torch.exp(logp - mb["old_log_prob"])
    inside = (ratio >= 1 - clip) & (ratio <= 1 + clip)
    s1, s2 = -adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)
    g_ratio = torch.where(inside | (s1 > s2), -adv, torch.zeros_like(adv))       # outside the range the clipped arm carries no gradient
    dlogp = g_ratio * ratio / n
    dmu = dlogp[:, None] * (a - mu) / sigma ** 2
    dsigma = (dlogp[:, None] * ((a - mu) ** 2 / sigma ** 3 - 1 / sigma)).sum(0) - hp["entropy_coef"] / sigma
    tv, ret = mb["target_values"], mb["returns"]
    vin = (v - tv).abs() <= clip
    vc = tv + (v - tv).clamp(-clip, clip)
    e1, e2 = (v - ret) ** 2, (vc - ret) ** 2
    dv = torch.where(vin | (e1 > e2), 2 * (v - ret), torch.zeros_like(v)) * hp["value_loss_coef"] / n
    branches = dict(below=ratio < 1 - clip, inside=inside, above=ratio > 1 + clip, v_inside=vin, v_out_unclipped_arm=~vin & (e1 > e2), v_out_clipped_arm=~vin & (e1 < e2))
    return dmu, dsigma, dv, branches


def test_head_gradients_equal_closed_forms(case):
    state, mb = case
    m = R.make_model(ADIMS, CDIMS, state, torch.float64)
    with torch.no_grad():
        mu0, v0 = m.actor(mb["obs"]), m.critic(mb["critic_obs"]).squeeze(-1)
    mu, v, std = mu0.clone().requires_grad_(), v0.clone().requires_grad_(), m.std.detach().clone().requires_grad_()
    loss, _ = R.head_terms(mu, std, v, mb)
    gmu, gstd, gv = torch.autograd.grad(loss, (mu, std, v))
    dmu, dsigma, dv, br = closed_form_head(mu0, m.std.detach(), v0, mb)
    pos = mb["advantages"] > 0
    for name in ("below", "inside", "above"):                                  # rows in every branch, both signs of advantage
        assert bool((br[name] & pos).any()) and bool((br[name] & ~pos).any()), name
    for name in ("v_inside", "v_out_unclipped_arm", "v_out_clipped_arm"):
        assert bool(br[name].any()), name
    assert bool((dmu[br["above"] & pos] == 0).all()) and bool((dmu[br["below"] & ~pos] == 0).all())     # the clipped arm is the larger one there
    for got, want in ((gmu, dmu), (gstd, dsigma), (gv, dv)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("lr,kl,want", [(1e-3, 0.05, 1e-3 / 1.5), (1e-3, 0.002, 1.5e-3), (1e-3, 0.01, 1e-3), (1.2e-5, 0.05, 1e-5), (8e-3, 0.002, 1e-2),
                                         (1e-3, 0.0, 1e-3), (1e-3, -1.0, 1e-3)])
def test_learning_rate_rule(lr, kl, want):
    """down, up, unchanged, floor 1e-5, ceiling 1e-2; kl_mean <= 0 changes nothing"""
    assert R.lr_rule(lr, kl, 0.01) == pytest.approx(want, rel=1e-15)


def test_update_reuses_one_permutation_and_reports_means(case):
    """2 epochs x 2 mini-batches: the means are over all four mini-batches and the first one's terms are those of a single evaluation"""
    state, mb = case
    m = R.make_model(ADIMS, CDIMS, state, torch.float64)
    perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(1))
    _, first = R.minibatch_grad(R.make_model(ADIMS, CDIMS, state, torch.float64), R.rows_of(mb, perm[:ROWS // 2], torch.float64))
    hp = dict(R.HP, schedule="fixed")
    means1, lr, kls = R.update(m, mb, perm, 1, 1, hp)
    assert lr == hp["learning_rate"] and len(kls) == 1
    m2 = R.make_model(ADIMS, CDIMS, state, torch.float64)
    means, _, kls = R.update(m2, mb, perm, 2, 2, hp)
    assert len(kls) == 4 and kls[0] == pytest.approx(first["kl_mean"], rel=1e-12)
    assert all(math.isfinite(x) for x in means)
