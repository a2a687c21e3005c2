"""Self-checks of the mirror-symmetry reference (tests/ppo_sym_ref.py) that need no GPU: with identity tables the augmented law is the plain law on
the rows duplicated, the float64 gradient of the mirror loss agrees with a central finite difference, and the case table keeps its promises."""
import torch

import ppo_cases as PC
import ppo_ref as R
import ppo_sym_cases as SC
import ppo_sym_ref as SR


def identity_tables(adims, cdims):
    ident = lambda n: (torch.arange(n, dtype=torch.int32), torch.ones(n))
    return {"policy": ident(adims[0]), "critic": ident(cdims[0]), "actions": ident(adims[-1])}


def test_identity_tables_with_augmentation_equal_the_plain_reference_on_duplicated_rows():
    c = SC.get_case("small", 17)
    mb = c.rows(torch.float64)
    dup = {k: torch.cat([v, v]) for k, v in mb.items()}
    ident = identity_tables(c.adims, c.cdims)
    g_sym, s_sym = SR.minibatch_grad(R.make_model(c.adims, c.cdims, c.state, torch.float64), mb, ident, True, False, 0.0)
    g_dup, s_dup = R.minibatch_grad(R.make_model(c.adims, c.cdims, c.state, torch.float64), dup)
    for k in g_dup:
        assert torch.allclose(g_sym[k], g_dup[k], rtol=1e-12, atol=1e-15), k
    for k in ("surrogate", "value_loss", "entropy", "kl_mean"):
        assert abs(s_sym[k] - s_dup[k]) <= 1e-12 * abs(s_dup[k]), k
    assert s_sym["symmetry"] == 0.0                              # the mirror of a row under the identity is the row


def test_flags_off_is_the_plain_reference():
    c = SC.get_case("small", 17)
    mb = c.rows(torch.float64)
    g_off, s_off = SR.minibatch_grad(R.make_model(c.adims, c.cdims, c.state, torch.float64), mb, c.tables, False, False, 0.5)
    g, s = R.minibatch_grad(R.make_model(c.adims, c.cdims, c.state, torch.float64), mb)
    assert all(torch.equal(g_off[k], g[k]) for k in g) and all(s_off[k] == s[k] for k in s) and s_off["symmetry"] > 0


def test_mirror_loss_gradient_agrees_with_a_finite_difference():
    """3-layer actor at 5 rows, float64: d L_sym / d theta from autograd (target detached) against a central difference of L_sym with the target held"""
    adims, cdims = [7, 6, 5, 3], [9, 4, 1]
    g = torch.Generator().manual_seed(5)
    state = PC.init_state(adims, cdims, g)
    model = R.make_model(adims, cdims, state, torch.float64)
    obs = torch.randn(5, 7, generator=g).double()
    tables = SC.SMALL_TABLES

    def l_sym(target=None):
        mu, mu_m = model.actor(obs), model.actor(SR.apply_table(obs, tables["policy"]))
        t = SR.apply_table(mu.detach(), tables["actions"]) if target is None else target
        return (mu_m - t).pow(2).mean(), t

    loss, target = l_sym()
    grads = torch.autograd.grad(loss, list(model.actor.parameters()))
    h, worst = 1e-6, 0.0
    for p, gp in zip(model.actor.parameters(), grads):
        flat, gflat = p.data.view(-1), gp.reshape(-1)
        for j in range(0, flat.numel(), max(1, flat.numel() // 7)):
            old = float(flat[j])
            with torch.no_grad():
                flat[j] = old + h; up = float(l_sym(target)[0])
                flat[j] = old - h; dn = float(l_sym(target)[0])
                flat[j] = old
            fd = (up - dn) / (2 * h)
            worst = max(worst, abs(fd - float(gflat[j])))
            assert abs(fd - float(gflat[j])) <= 1e-8 + 1e-6 * abs(fd), (j, fd, float(gflat[j]))   # central difference: O(h^2) truncation, 1e-16 / h rounding
    assert float(loss.detach()) > 0 and max(float(g_.abs().max()) for g_ in grads) > 1e-3


def test_the_case_table_keeps_its_promises():
    for shape in SC.SHAPES:
        c = SC.get_case(*shape)                                    # the constructor asserts margins, mirrored-only clipping and ties
        for key, width in (("policy", c.adims[0]), ("critic", c.cdims[0]), ("actions", c.adims[-1])):
            src, sign = c.tables[key]
            assert sorted(src.tolist()) == list(range(width)) and set(sign.tolist()) <= {1.0, -1.0}
            assert torch.equal(src[src.long()].long(), torch.arange(width)) and torch.equal(sign[src.long()] * sign, torch.ones(width))   # an involution
    small = SC.SMALL_TABLES
    assert any(int(s) == j for j, s in enumerate(small["policy"][0])) and any(int(s) != j for j, s in enumerate(small["policy"][0]))
    assert {1.0, -1.0} == set(small["policy"][1].tolist()) == set(small["critic"][1].tolist()) == set(small["actions"][1].tolist())
