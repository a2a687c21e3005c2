"""The recurrent reference and its case table on the CPU (tests/ppo_rnn_ref.py, tests/ppo_rnn_cases.py): the masked fixed-grid unroll equals nn.LSTM run over
the split trajectories (rsl_rl's split-and-pad), the cases meet their own conditions, and the state-dict keys, shapes and flat order are those of
include/go2sim_rnn.h as ppo.state_dict_keys lists them."""
import pytest
import torch
from torch import nn

import ppo_rnn_cases as RC
import ppo_rnn_collect_ref as CR
import ppo_rnn_ref as RR


def test_unroll_equals_nn_lstm_over_split_trajectories():
    """Every env's steps are cut after each done; each piece runs through nn.LSTM as one sequence, the first from the saved state, the others from zero."""
    T, n, n_in, H = 9, 6, 5, 7
    g = torch.Generator().manual_seed(3)
    lstm = nn.LSTM(n_in, H).double()
    x = torch.randn(T, n, n_in, generator=g).double()
    h0, c0 = torch.randn(n, H, generator=g).double(), torch.randn(n, H, generator=g).double()
    dones = (torch.rand(T, n, generator=g) < 0.3).to(torch.uint8)
    dones[:, 0] = 0; dones[:, 1] = 1; dones[T - 1, 2] = 1
    with torch.no_grad():
        hs, (h_end, c_end), _ = RR.unroll(lstm, x, h0, c0, dones)
        worst = 0.0
        for e in range(n):
            start, state = 0, (h0[e].reshape(1, 1, H), c0[e].reshape(1, 1, H))
            for t in range(T):
                if dones[t, e] or t == T - 1:
                    out, state_end = lstm(x[start:t + 1, e:e + 1], state)
                    worst = max(worst, float((out[:, 0] - hs[start:t + 1, e]).abs().max()))
                    if t == T - 1:
                        worst = max(worst, float((state_end[0][0, 0] - h_end[e]).abs().max()), float((state_end[1][0, 0] - c_end[e]).abs().max()))
                    start, state = t + 1, (torch.zeros(1, 1, H).double(), torch.zeros(1, 1, H).double())
    print(f"unroll against split trajectories: {worst:.3e}")
    assert worst <= 1e-15


def test_reference_cell_is_the_stated_law():
    """One step written out (gate order i, f, g, o, two biases) against nn.LSTM"""
    g = torch.Generator().manual_seed(5)
    lstm = nn.LSTM(4, 3).double()
    x, h, c = (torch.randn(2, k, generator=g).double() for k in (4, 3, 3))
    with torch.no_grad():
        z = x @ lstm.weight_ih_l0.T + lstm.bias_ih_l0 + h @ lstm.weight_hh_l0.T + lstm.bias_hh_l0
        i, f, gg, o = torch.sigmoid(z[:, 0:3]), torch.sigmoid(z[:, 3:6]), torch.tanh(z[:, 6:9]), torch.sigmoid(z[:, 9:12])
        c1 = f * c + i * gg
        h1 = o * torch.tanh(c1)
        out, (hn, cn) = lstm(x.unsqueeze(0), (h.unsqueeze(0), c.unsqueeze(0)))
    assert float((hn[0] - h1).abs().max()) <= 1e-15 and float((cn[0] - c1).abs().max()) <= 1e-15 and torch.equal(out[0], hn[0])


def test_case_table_covers_the_axes():
    cs = list(RC.GRAD_CASES.values())
    assert {c[0] for c in cs} == {16, 20, 48, 68, 80, 256, 512} and {c[1] for c in cs} | {c[2] for c in cs} == {5, 49, 64, 104}
    assert {c[3] for c in cs} == {1, 2, 3, 8} and {c[4] for c in cs} == {1, 5, 17, 33, 37, 70}
    assert {c[5] for c in cs} == set(RC.PATTERNS) and {c[6] for c in cs} == {"zero", "nonzero"} and {c[7] for c in cs} == {1, 3}
    assert any(c[3] * c[4] > 512 for c in cs), "one case crosses a 512-row chunk"
    # the column groups of k_lstm_cell / k_lstm_bptt: a workgroup owns NWAVE tiles of 16 hidden units, blockIdx.y walks the further groups
    tiles = lambda H: (H + 15) // 16
    assert any(tiles(c[0]) > RC.NWAVE for c in cs), "a second column group"
    assert any(tiles(c[0]) > RC.NWAVE and tiles(c[0]) % RC.NWAVE for c in cs), "a last group whose trailing wavefronts leave"
    assert any(c[0] % 16 and (tiles(c[0]) - 1) // RC.NWAVE > 0 for c in cs), "a padded tile in a later group"
    assert any(c[1] % 16 == 0 or c[2] % 16 == 0 for c in cs), "an input width without padding"
    assert any(c[0] == 256 and {c[1], c[2]} == {49, 104} for c in cs), "the product's widths"
    assert any(c[0] == 512 for c in cs), "GO2SIM_MLP_MAX_WIDTH"
    assert any(c[4] > 32 and c[4] % 32 == 1 and tiles(c[0]) > RC.NWAVE for c in cs), "a second row tile of one row under a second column group"


def test_case_seeds_do_not_depend_on_the_table():
    """The seeds of the first nine cases are the ones their recorded ratios (include/go2sim_rnn.h) were measured with; new names get seeds of their own."""
    assert RC.SEED_NAMES_0 == tuple(sorted(RC.SEED_NAMES_0)) and len(RC.SEED_NAMES_0) == 9
    assert set(RC.SEED_NAMES_0) | set(RC.SEED_NAMES_1) == set(RC.GRAD_CASES) and not set(RC.SEED_NAMES_0) & set(RC.SEED_NAMES_1)
    assert RC.SEED_NAMES_0 == tuple(sorted(list(RC.GRAD_CASES)[:9])), "the earlier rule: the sorted position among the first nine names"
    import unittest.mock as mock

    seen = {}
    with mock.patch.object(RC, "Case", lambda name, seed: seen.setdefault(name, seed)):
        for name in RC.GRAD_CASES:
            RC.get_case.__wrapped__(name)
    assert seen["h16-t1-n1"] == 5000 and seen["h48-t8-n37-random"] == 5000 + 31 * 8 and seen["h20-t3-n17-last"] == seen["h20-t3-n17-none"] == 5000 + 31 * 5
    new = [seen[k] for k in RC.SEED_NAMES_1]
    assert new == [9000 + 31 * i for i in range(len(new))] and len(set(seen.values())) == len(seen) - 1
    assert not {s + d for s in new for d in (0, 1)} & {seen[k] + d for k in RC.SEED_NAMES_0 for d in (0, 1)}, "a case uses seed and seed + 1"


@pytest.mark.parametrize("name", sorted(RC.GRAD_CASES))
def test_cases_meet_their_conditions(name):
    c = RC.get_case(name)                                   # the constructor asserts the gate regimes and the margins
    sl = slice(c.e0, c.e0 + c.nb)
    d = c.rollout["dones"][:, sl]
    if c.pattern == "none":
        assert not d.any()
    elif c.pattern == "last":
        assert d[-1].any() and not d[:-1].any()
    elif c.pattern == "step0":
        assert d[0].any() and not d[1:].any()
    elif c.pattern == "every":
        assert d[:, 0].all() and not d[:, 1:].any()
    else:
        assert d.any() or c.T * c.nb < 10
    zero = all(not c.init[k][sl].any() for k in c.init)
    assert zero == (c.init_kind == "zero")
    assert all(torch.isnan(x[:, :c.e0]).all() for k, x in c.rollout.items() if k != "dones"), "the envs outside the block hold NaN"
    g64, s64, _ = c.ref["f64"]
    assert all(bool(torch.isfinite(v).all()) for v in g64.values())
    for k, v in g64.items():                                # one step from a zero state: h_prev = 0, W_hh has no gradient; every other tensor has one
        assert (float(v.abs().max()) > 0) != (k.endswith("weight_hh_l0") and c.T == 1 and c.init_kind == "zero"), k
    for q in ("a", "c"):
        assert torch.equal(g64[f"memory_{q}.rnn.bias_ih_l0"], g64[f"memory_{q}.rnn.bias_hh_l0"]), "the two biases have equal gradients"


def test_dones_at_the_last_step_change_nothing_within_the_rollout():
    a, b = RC.get_case("h20-t3-n17-last"), RC.get_case("h20-t3-n17-none")
    assert a.rollout["dones"].ne(b.rollout["dones"]).any()
    for k, g in a.ref["f64"][0].items():
        assert torch.equal(g, b.ref["f64"][0][k]), k
    assert a.ref["f64"][1] == b.ref["f64"][1]


@pytest.mark.parametrize("name", sorted(RC.UPDATE_CASES))
def test_update_case_moves_every_tensor(name):
    u = RC.get_update_case(name)
    assert (u["H"] + 15) // 16 > RC.NWAVE or name == "h20-t3-n17"
    assert u["B"] == u["nb"] * u["n_mb"] and len(u["f64"]["kls"]) == u["epochs"] * u["n_mb"]
    for k, p in u["f64"]["params"].items():
        assert float((p - u["state"][k].double()).abs().max()) > 0, k
        assert float((u["f32"]["params"][k].double() - p).abs().max()) > 0, k


def test_state_dict_keys_shapes_and_flat_order():
    from go2_sim2real_locomotion_rl_amd.ppo import flatten, state_dict_keys, unflatten

    c = RC.get_case("h20-t3-n17-none")
    m = c.ref["f64"][2]
    want = [(k, tuple(p.shape)) for k, p in RR.ordered_params(m)]
    assert state_dict_keys(c.adims, c.cdims, c.mdims) == want
    assert {k for k, _ in want} == set(m.state_dict()), "the keys of the torch module (rsl_rl's ActorCriticRecurrent: actor, critic, std, memory_a, memory_c)"
    H = c.H
    assert dict(want)["memory_a.rnn.weight_ih_l0"] == (4 * H, c.Ia) and dict(want)["memory_c.rnn.weight_hh_l0"] == (4 * H, H)
    assert dict(want)["memory_c.rnn.bias_ih_l0"] == (4 * H,) and want[-1] == ("std", (RC.A,))
    i_mem = [i for i, (k, _) in enumerate(want) if k.startswith("memory_")]
    assert i_mem == list(range(len(want) - 9, len(want) - 1)), "the memories sit between the critic and std"
    flat = flatten(c.state, c.adims, c.cdims, c.mdims)
    back = unflatten(flat, c.adims, c.cdims, c.mdims)
    assert all(torch.equal(back[k], c.state[k]) for k in c.state) and list(back) == [k for k, _ in want]
    # without memories the plain order is unchanged
    assert state_dict_keys(c.adims, c.cdims) == [kv for kv in want if not kv[0].startswith("memory_")]


# ---- the collection replay (tests/ppo_rnn_collect_ref.py) ----------------------------------------------------------------------------------------
def _collect_by_hand(model, obs, cobs, dones, last, save_after=False, no_reset=False, dones_shift=0, skip_last_step=False):
    """The classes' order of calls, one env step at a time and written out without unroll: save, act (both memories), reset(dones), ..., evaluate"""
    _, T, B = dones.shape
    H = model.H
    st = {k: torch.zeros(B, H, dtype=torch.float64) for k in CR.STATE_KEYS}
    step = lambda lstm, x, h, c: [s[0] for s in lstm(x.unsqueeze(0), (h.unsqueeze(0), c.unsqueeze(0)))[1]]
    out = []
    with torch.no_grad():
        for r in range(2):
            saved, mus, vs = None, [], []
            for t in range(T):
                if t == 0 and not save_after:
                    saved = {k: v.clone() for k, v in st.items()}
                st["h_a"], st["c_a"] = step(model.memory_a.rnn, obs[r, t], st["h_a"], st["c_a"])
                st["h_c"], st["c_c"] = step(model.memory_c.rnn, cobs[r, t], st["h_c"], st["c_c"])
                if t == 0 and save_after:
                    saved = {k: v.clone() for k, v in st.items()}
                mus.append(model.actor(st["h_a"])); vs.append(model.critic(st["h_c"]).squeeze(-1))
                if not no_reset:
                    d = dones[r, t - dones_shift] if 0 <= t - dones_shift < T else torch.zeros(B, dtype=torch.uint8)
                    for k in st:
                        st[k] = st[k] * (d == 0).double().unsqueeze(-1)
            if not skip_last_step:
                st["h_c"], st["c_c"] = step(model.memory_c.rnn, last[r], st["h_c"], st["c_c"])
            out.append(dict(saved=saved, mu=torch.stack(mus), v=torch.stack(vs), live={k: v.clone() for k, v in st.items()}))
    return out


def _collect_inputs():
    T, B, H, Ia, Ic = 4, 6, 20, 5, 7
    g = torch.Generator().manual_seed(11)
    sd = RC.init_state(H, Ia, Ic, [H, 8, RC.A], [H, 8, 1], g)
    model = RR.make_model(Ia, Ic, [H, 8, RC.A], [H, 8, 1], sd, torch.float64)
    obs = RC.obs_scale(Ia, H) * torch.randn(2, T, B, Ia, generator=g).double()
    cobs = RC.obs_scale(Ic, H) * torch.randn(2, T, B, Ic, generator=g).double()
    last = RC.obs_scale(Ic, H) * torch.randn(2, B, Ic, generator=g).double()
    return model, obs, cobs, CR.scripted_dones(T, B), last


def _replay_two(model, obs, cobs, dones, last):
    live, out = CR.zero_state(dones.shape[2], model.H, torch.float64), []
    for r in range(2):
        out.append(CR.replay_rollout(model, live, obs[r], cobs[r], dones[r], last[r]))
        live = out[-1]["live"]
    return out


def _worst(a, b):
    return max(float((x[k] - y[k]).abs().max()) for x, y in zip(a, b) for k in ("mu", "v")), \
        max(float((x[w][k] - y[w][k]).abs().max()) for x, y in zip(a, b) for w in ("saved", "live") for k in CR.STATE_KEYS)


def test_collect_replay_is_the_order_of_calls():
    model, obs, cobs, dones, last = _collect_inputs()
    CR.check_dones_script(dones)
    want, got = _collect_by_hand(model, obs, cobs, dones, last), _replay_two(model, obs, cobs, dones, last)
    assert max(_worst(want, got)) <= 1e-15
    s = got[1]["saved"]                                     # rollout 1's saved state: env 2 was done at rollout 0's last step, env 3 never
    assert not s["h_a"][2].any() and not s["c_a"][2].any(), "memory_a of an env done at the last step starts the next rollout at zero"
    assert s["h_c"][2].any() and s["c_c"][2].any(), "memory_c of that env has taken compute_returns' step from zero"
    assert all(s[k][3].any() for k in s) and not any(got[0]["saved"][k].any() for k in s)
    assert float((got[0]["live"]["h_c"] - s["h_c"]).abs().max()) == 0.0


@pytest.mark.parametrize("mutation", ["save_after", "no_reset", "dones_shift", "skip_last_step"])
def test_collect_replay_tells_the_mistakes_apart(mutation):
    """Each mistake the collection test is written for moves the recorded numbers far above any rounding"""
    model, obs, cobs, dones, last = _collect_inputs()
    kw = {mutation: 1 if mutation == "dones_shift" else True}
    got, want = _collect_by_hand(model, obs, cobs, dones, last, **kw), _replay_two(model, obs, cobs, dones, last)
    assert max(_worst(want, got)) > 1e-3
