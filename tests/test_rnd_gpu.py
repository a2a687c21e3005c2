"""The HIP library's random network distillation (include/go2sim_rnd.h) against the float64 reference of tests/rnd_ref.py over the cases of
tests/rnd_cases.py, with the float32 torch evaluation of the same expressions as the yardstick:
  (a) the step's embeddings: bit-equal to go2sim_mlp_forward; |r - r64| <= 2^-24 r64 against float64 on the library's own embeddings
  (b) the reward normaliser over a sequence of steps: avg bit-equal to the float32 recurrence on the library's own r, the state within the bounds of
      tests/norm_ref.py for a one-column fold, the std == 0 branch (N = 1), intrinsic and rewards_total exactly items 5 to 7 from the library's own r and state
  (c) the state normaliser in front: s bit-equal to go2sim_norm_step, and s is what the step embeds
  (d) mini-batch gradients, per predictor tensor:  max|g - g64| <= C_GRAD max(max|g32 - g64|, 2^-24 max|g64|)
  (e) whole updates, per tensor:  max|p - p64| <= C_UPD max|p32 - p64|;  rnd_loss equal to a float64 evaluation on the library's own embeddings to 1e-12 relative
  (f) the target never moves, equal calls give equal bits, export / import / set_step round-trip, the status codes.
C_GRAD = 16 and C_UPD = 8 are the project's constants (include/go2sim_train.h).  Every test prints its ratios before it asserts.
Worst ratios measured on the MI355X: 1.73 (C_GRAD: wide_e20, 17 rows, the last bias), 2.22 (C_UPD: wide_e20, 5 x 4, the last bias), 1.000 (the distance's
2^-24 r64), 0.83 (the reward state's bounds), 3.3e-16 (rnd_loss); include/go2sim_rnd.h names the cases."""
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as NR
import rnd_cases as RC
import rnd_ref as R

pytestmark = pytest.mark.gpu

C_GRAD = 16
C_UPD = 8
EPS = 2.0 ** -24
DEV = "cuda:0"


def r16(v):
    return (v + 15) // 16 * 16


def real_entry_mask(dims):
    parts = []
    for l in range(len(dims) - 1):
        w = np.zeros((r16(dims[l + 1]), r16(dims[l])), bool); w[:dims[l + 1], :dims[l]] = True
        b = np.zeros(r16(dims[l + 1]), bool); b[:dims[l + 1]] = True
        parts += [w.reshape(-1), b]
    return np.concatenate(parts)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


class Side:
    """Predictor, target and one go2sim_rnd handle on the GPU"""

    def __init__(self, lib, net, state, max_rows, **hyper):
        from go2_sim2real_locomotion_rl_amd.policy import Mlp, flatten_sequential
        from go2_sim2real_locomotion_rl_amd.rnd import RndHandle

        self.lib = lib
        self.pdims, self.tdims, self.act = RC.NETS[net]
        self.predictor = Mlp(lib, self.pdims, flatten_sequential(state, "predictor", len(self.pdims) - 1)[0], 0, self.act)
        self.target = Mlp(lib, self.tdims, flatten_sequential(state, "target", len(self.tdims) - 1)[0], 0, self.act)
        self.h = RndHandle(lib, self.predictor, self.target, max_rows, **hyper)
        self.E = self.pdims[-1]

    def split(self, flat):
        from go2_sim2real_locomotion_rl_amd.module_core import mlp_keys, unflatten_keys

        return {k: v.double() for k, v in unflatten_keys(flat.cpu(), mlp_keys("predictor", self.pdims)).items()}

    def forward(self, rows):
        """(target, predictor) embeddings of `rows` through go2sim_mlp_forward"""
        n = rows.shape[0]
        t, p = (torch.full((n, self.E), float("nan"), device=DEV) for _ in range(2))
        self.target.forward(rows.contiguous(), t, n)
        self.predictor.forward(rows.contiguous(), p, n)
        return t, p

    def step(self, s, rewards, w):
        n = s.shape[0]
        intrinsic, total = (torch.full((n,), float("nan"), device=DEV) for _ in range(2))
        self.h.step(s, rewards, w, intrinsic, total)
        return intrinsic, total

    def stats(self):
        s = self.h.stats().cpu()
        return dict(loss=float(s[0]), lr=float(s[1]), grad_norm=float(s[2]), step=int(s[3]), minibatches=int(s[4]), applies=int(s[5])), s


# ---- (a) embeddings and the distance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.STEP_CASES, ids=RC.case_id)
def test_step_embeddings_and_distance(hip_lib, case):
    net, n = case
    side = Side(hip_lib, net, RC.net_state(net, 100 + n), n)
    s = RC.states(net, n, 200 + n).to(DEV)
    rewards = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    w = 0.75
    intrinsic, total = side.step(s, rewards, w)
    t, p, r = side.h.last_step(n)
    tf, pf = side.forward(s)
    torch.cuda.synchronize()
    assert np.array_equal(bits(t), bits(tf)) and np.array_equal(bits(p), bits(pf)), "the step's embeddings are go2sim_mlp_forward's"
    assert np.isfinite(t.cpu().numpy()).all() and np.isfinite(p.cpu().numpy()).all()
    r64 = R.distance64(t.cpu().numpy(), p.cpu().numpy())
    err = np.abs(r.cpu().numpy().astype(np.float64) - r64)
    ok = r64 >= 2.0 ** -126                                                  # a subnormal distance is rounded absolutely: exempt
    ratio = float((err[ok] / (EPS * r64[ok])).max()) if ok.any() else 0.0
    print(f"RATIO distance {RC.case_id(case)} {ratio:.3f} (of 2^-24 r64)")
    assert ratio <= 1.0 and float(r64.min()) > 0.0
    # without the reward normaliser: items 6 and 7 from the library's own r, exactly
    want_i, want_t = R.finish(r.cpu().numpy(), 0.0, w, rewards.cpu().numpy())
    assert np.array_equal(bits(intrinsic), want_i.view(np.int32)) and np.array_equal(bits(total), want_t.view(np.int32))
    m, v, sd, cnt, _ = side.h.get_reward_state(0)
    assert (m, v, sd, cnt) == (0.0, 1.0, 1.0, 0), "the reward normaliser is off: its state does not move"


# ---- (b) the reward normaliser -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("tiny_e1", 1), ("tiny_e1", 17), ("obs45_e12", 37), ("default_e32", 257), ("obs45_e12", 1000), ("wide_e20", 1000)], ids=RC.case_id)
def test_reward_normaliser_sequence(hip_lib, case):
    net, n = case
    side = Side(hip_lib, net, RC.net_state(net, 300 + n), n, reward_normalization=True)
    g = torch.Generator().manual_seed(400 + n)
    state = NR.initial_state(1)
    avg = np.zeros(n, np.float32)
    worst = {"mean": 0.0, "var": 0.0, "std": 0.0}
    for k in range(6):
        s = (torch.randn(n, side.pdims[0], generator=g) * (1.0 + 0.5 * k)).float().to(DEV)
        rewards = torch.randn(n, generator=g).float().to(DEV)
        w = R.weight(0.8, {"mode": "linear", "initial_step": 2, "final_step": 5, "final_value": 0.1}, k + 1)
        intrinsic, total = side.step(s, rewards, w)
        _, _, r = side.h.last_step(n)
        r = r.cpu().numpy()
        m, v, sd, cnt, avg_dev = side.h.get_reward_state(n)
        avg = R.advance_avg(avg, r)
        assert np.array_equal(avg_dev.view(np.int32), avg.view(np.int32)), f"step {k}: avg is the float32 recurrence on the library's own r"
        new64, bound = R.reward_fold(state, avg)
        assert cnt == new64["count"] == (k + 1) * n
        for name, got in (("mean", m), ("var", v), ("std", sd)):
            err, b = abs(float(got) - float(new64[name][0])), float(bound[name][0])
            worst[name] = max(worst[name], err / b)
            assert err <= b, (k, name, got, new64[name][0], b)
        if n == 1 and k == 0:
            assert v == 0.0 and sd == 0.0, "N = 1: the first fold gives var = 0"
        want_i, want_t = R.finish(r, sd, w, rewards.cpu().numpy())      # from the library's own r and state: exact
        assert np.array_equal(bits(intrinsic), want_i.view(np.int32)), f"step {k}: intrinsic"
        assert np.array_equal(bits(total), want_t.view(np.int32)), f"step {k}: rewards_total"
        if n == 1 and k == 0:
            assert np.array_equal(bits(intrinsic), (np.float32(w) * r).view(np.int32)), "std == 0: r is unchanged"
        state = {"mean": np.array([m], np.float32), "var": np.array([v], np.float32), "std": np.array([sd], np.float32), "count": cnt}   # one step at a time
    print(f"RATIO reward state {RC.case_id(case)} " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()) + " (of the bounds of norm_ref)")


def test_reward_state_round_trip_and_until(hip_lib):
    net, n = "obs45_e12", 37
    a = Side(hip_lib, net, RC.net_state(net, 5), n, reward_normalization=True)
    b = Side(hip_lib, net, RC.net_state(net, 5), 64, reward_normalization=True)      # another max_rows: the state does not depend on it
    s, rewards = RC.states(net, n, 6).to(DEV), torch.zeros(n, device=DEV)
    for _ in range(2):
        a.step(s, rewards, 1.0)
    m, v, sd, cnt, avg = a.h.get_reward_state(n)
    b.h.set_reward_state(m, v, sd, cnt, avg)
    assert [x for x in b.h.get_reward_state(n)[:4]] == [m, v, sd, cnt] and np.array_equal(b.h.get_reward_state(n)[4].view(np.int32), avg.view(np.int32))
    out = [side.step(s, rewards, 1.0) for side in (a, b)]
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    sa, sb = a.h.get_reward_state(n), b.h.get_reward_state(n)
    assert sa[:4] == sb[:4] and np.array_equal(sa[4].view(np.int32), sb[4].view(np.int32))
    # count >= until: avg still advances, the state stands still
    b.h.set_reward_state(m, v, sd, 10 ** 8, avg)
    i1, _ = b.step(s, rewards, 1.0)
    m2, v2, sd2, cnt2, avg2 = b.h.get_reward_state(n)
    _, _, r = b.h.last_step(n)
    assert (m2, v2, sd2, cnt2) == (m, v, sd, 10 ** 8)
    assert np.array_equal(avg2.view(np.int32), R.advance_avg(avg, r.cpu().numpy()).view(np.int32))
    assert np.array_equal(bits(i1), R.finish(r.cpu().numpy(), sd, 1.0, rewards.cpu().numpy())[0].view(np.int32))


# ---- (c) the state normaliser in front ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 257])
def test_state_normaliser_rows_are_what_gets_embedded(hip_lib, n):
    from go2_sim2real_locomotion_rl_amd.normalization import EmpiricalNormalization, norm_step
    from go2_sim2real_locomotion_rl_amd.rnd import RandomNetworkDistillation

    rnd = RandomNetworkDistillation(45, num_outputs=12, predictor_hidden_dims=[32, 24], target_hidden_dims=[-1], activation="tanh", weight=0.5, state_normalization=True,
                                    reward_normalization=True, device=torch.device(DEV), seed=3)
    rnd.attach(n)
    assert rnd.pdims == [45, 32, 24, 12] and rnd.tdims == [45, 45, 12]
    twin = EmpiricalNormalization([45], eps=1e-2, until=1.0e8, device=torch.device(DEV))
    g = torch.Generator().manual_seed(n)
    for k in range(3):
        x = (3.0 + torch.randn(n, 45, generator=g) * 2.0).float().to(DEV)
        rewards = torch.randn(n, generator=g).float().to(DEV)
        x0 = bits(x)
        intrinsic, total = rnd.get_intrinsic_reward(x, rewards)
        want = norm_step(twin, x, update=True)[0]
        assert np.array_equal(bits(rnd.last_state), bits(want)), "s is go2sim_norm_step's output"
        assert np.array_equal(bits(x), x0), "the env's rows are not written"
        t, p, _ = rnd._h.last_step(n)
        tf, pf = (torch.empty(n, 12, device=DEV) for _ in range(2))
        rnd._target.forward(want, tf, n); rnd._predictor.forward(want, pf, n)
        assert np.array_equal(bits(t), bits(tf)) and np.array_equal(bits(p), bits(pf)), "the networks read the normalised rows"
        assert rnd.update_counter == k + 1 and np.isfinite(total.cpu().numpy()).all()
    sd = rnd.state_dict()
    assert {k for k in sd if k.startswith("state_normalizer.")} == {"state_normalizer." + k for k in ("_mean", "_var", "_std", "count")}
    assert int(sd["state_normalizer.count"]) == 3 * n and int(sd["reward_normalizer.emp_norm.count"]) == 3 * n
    assert np.array_equal(bits(sd["state_normalizer._mean"]), bits(twin.state_dict()["_mean"]))


def test_predictor_and_target_differ_and_follow_the_seed(hip_lib):
    from go2_sim2real_locomotion_rl_amd.rnd import RandomNetworkDistillation

    a, b, c = (RandomNetworkDistillation(49, num_outputs=4, device=torch.device(DEV), seed=s) for s in (1, 1, 2))
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert sorted(sa) == sorted(f"{p}.{l}.{w}" for p in ("predictor", "target") for l in (0, 2) for w in ("weight", "bias"))
    assert tuple(sa["predictor.0.weight"].shape) == (49, 49) and tuple(sa["target.2.weight"].shape) == (4, 49)     # -1 is num_states
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and not torch.equal(sa["predictor.0.weight"], sc["predictor.0.weight"])
    assert not torch.equal(sa["predictor.0.weight"], sa["target.0.weight"]), "the target's draws have a seed purpose of their own"


# ---- (d) mini-batch gradients ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.GRAD_CASES, ids=RC.case_id)
def test_minibatch_gradients(hip_lib, case):
    c = RC.get_grad_case(*case)
    g64, g32 = c.ref["f64"]["grads"], c.ref["f32"]["grads"]
    side = Side(hip_lib, c.net, c.state, c.n)
    s, idx = c.s.to(DEV), c.idx.to(DEV)
    t0 = bits(side.forward(s)[0])
    side.h.minibatch_grad(s, idx)
    got = side.split(side.h.export("GRADS"))
    padded = side.h.export_padded("GRADS").cpu().numpy()
    worst = 0.0
    for k in g64:
        err, yard = float((got[k] - g64[k]).abs().max()), max(float((g32[k].double() - g64[k]).abs().max()), EPS * float(g64[k].abs().max()))
        print(f"RATIO grad {RC.case_id(case)} {k} {err / yard:.3f}")
        worst = max(worst, err / yard)
    print(f"RATIO worst grad {RC.case_id(case)} {worst:.3f}")
    assert worst <= C_GRAD
    assert np.isfinite(padded).all() and not padded[~real_entry_mask(c.pdims)].any(), "padded gradient entries must be exactly zero"
    # the loss statistic against float64 on the library's own embeddings of the mini-batch's rows
    t, p = side.forward(s[idx.long()])
    want = float(((p.cpu().double() - t.cpu().double()) ** 2).mean())
    st, _ = side.stats()
    print(f"RATIO loss {RC.case_id(case)} {abs(st['loss'] - want) / want:.3e}")
    assert abs(st["loss"] - want) <= 1e-12 * want and st["minibatches"] == 1 and st["step"] == 0 and st["applies"] == 0
    assert st["loss"] == pytest.approx(c.ref["f64"]["loss"], rel=1e-4)       # against the float64 law: fp32 forward passes, a sanity bound
    assert np.array_equal(bits(side.forward(s)[0]), t0)


# ---- (e) whole updates ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.UPDATE_CASES, ids=RC.case_id)
def test_whole_update(hip_lib, case):
    u = RC.get_update_case(*case)
    E, nmb, n = u["E"], u["nmb"], u["n"]
    mbs = n // nmb
    side, twin = (Side(hip_lib, u["net"], u["state"], mbs) for _ in range(2))
    s, idx = u["s"].to(DEV), u["idx"].to(DEV)
    t_before = bits(side.forward(s)[0])
    side.h.update(s, idx, n, E, nmb)
    got = side.split(side.h.export("PARAMS"))
    st, _ = side.stats()
    assert st["step"] == E * nmb and st["applies"] == E * nmb and st["minibatches"] == E * nmb and st["lr"] == R.LR
    worst = 0.0
    for k, p64 in u["f64"]["params"].items():
        err, yard = float((got[k] - p64).abs().max()), float((u["f32"]["params"][k].double() - p64).abs().max())
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
        print(f"RATIO update {RC.case_id(case)} {k} {ratio:.3f}")
        worst = max(worst, ratio)
    print(f"RATIO worst update {RC.case_id(case)} {worst:.3f}")
    assert worst <= C_UPD
    # rnd_loss: the same sequence by hand on a twin handle, the loss of every mini-batch in float64 from the library's own embeddings
    twin.h.reset_stats()
    losses = []
    for _ in range(E):
        for i in range(nmb):
            rows = idx[i * mbs:(i + 1) * mbs]
            t, p = twin.forward(s[rows.long()])
            losses.append(float(((p.cpu().double() - t.cpu().double()) ** 2).mean()))
            twin.h.minibatch_grad(s, rows)
            twin.h.apply()
    want = sum(losses) / len(losses)
    print(f"RATIO rnd_loss {RC.case_id(case)} {abs(st['loss'] - want) / want:.3e}")
    assert abs(st["loss"] - want) <= 1e-12 * want
    assert st["loss"] == pytest.approx(u["f64"]["loss"], rel=1e-4)
    for which in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V"):
        assert np.array_equal(bits(side.h.export(which)), bits(twin.h.export(which))), f"update() is the loop of minibatch_grad and apply: {which}"
    assert np.array_equal(twin.stats()[1].numpy().view(np.int64), side.stats()[1].numpy().view(np.int64))
    mask = real_entry_mask(u["pdims"])
    for which in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V"):
        assert not side.h.export_padded(which).cpu().numpy()[~mask].any(), which
    # (f) the target never moves
    assert np.array_equal(bits(side.forward(s)[0]), t_before)


# ---- (f) independence, reproducibility, round trips ------------------------------------------------------------------------------------------------------------
def test_optimizer_state_round_trip(hip_lib):
    u = RC.get_update_case("obs45_e12", (2, 2))
    n, E, nmb = u["n"], u["E"], u["nmb"]
    s, idx = u["s"].to(DEV), u["idx"].to(DEV)
    a, b = (Side(hip_lib, u["net"], u["state"], n // nmb) for _ in range(2))
    a.h.update(s, idx, n, E, nmb)
    for which in ("PARAMS", "ADAM_M", "ADAM_V"):
        b.h.import_(which, a.h.export(which))
    sa, _ = a.stats()
    assert sa["step"] == 4
    b.h.set_step(sa["step"], sa["lr"])
    for side in (a, b):
        side.h.update(s, idx, n, E, nmb)
    for which in ("PARAMS", "ADAM_M", "ADAM_V", "GRADS"):
        assert np.array_equal(bits(a.h.export(which)), bits(b.h.export(which))), which
    assert np.array_equal(a.stats()[1].numpy().view(np.int64), b.stats()[1].numpy().view(np.int64)) and a.stats()[0]["step"] == 8
    a.h.reset_stats()
    st, _ = a.stats()
    assert st["loss"] == 0.0 and st["minibatches"] == 0 and st["applies"] == 0 and st["step"] == 8


def test_step_and_update_do_not_disturb_each_other(hip_lib):
    """a step between two updates (the embeddings share the update's buffers) changes no bit of the second update, and the other way round"""
    u = RC.get_update_case("wide_e20", (2, 2))
    n, E, nmb = u["n"], u["E"], u["nmb"]
    s, idx = u["s"].to(DEV), u["idx"].to(DEV)
    rewards = torch.ones(n, device=DEV)
    a, b = (Side(hip_lib, u["net"], u["state"], n, reward_normalization=True) for _ in range(2))
    ia = a.step(s, rewards, 0.5)
    a.h.update(s, idx, n, E, nmb)
    b.h.update(s, idx, n, E, nmb)
    ib0 = b.step(s, rewards, 0.5)                                            # b's first step sees the updated predictor: another bonus
    assert not np.array_equal(bits(ia[0]), bits(ib0[0]))
    for which in ("PARAMS", "ADAM_M", "ADAM_V"):
        assert np.array_equal(bits(a.h.export(which)), bits(b.h.export(which))), which
    e, r = torch.zeros(1, a.E, device=DEV), torch.zeros(1, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    assert a.h.L.fn("rnd_last_step")(a.h.h, ptr(e), ptr(e), ptr(r), 1, ctypes.c_void_p(0)) == -1, "after an update the step's embeddings are gone: refused"
    assert b.h.L.fn("rnd_last_step")(b.h.h, ptr(e), ptr(e), ptr(r), 1, ctypes.c_void_p(0)) == 0


def test_bad_arguments_return_a_status_and_launch_nothing(hip_lib):
    from go2_sim2real_locomotion_rl_amd.capi import C, RndCfg

    BAD, null, st = C["GO2SIM_E_BADARG"], ctypes.c_void_p(0), ctypes.c_void_p(0)
    net = "obs45_e12"
    side = Side(hip_lib, net, RC.net_state(net, 1), 16)
    other = Side(hip_lib, "tiny_e1", RC.net_state("tiny_e1", 1), 16)
    L, h, p = hip_lib, side.h.h, lambda t: ctypes.c_void_p(t.data_ptr())
    cfg = RndCfg(1e-3, 0.9, 0.999, 1e-8, 0)
    out = ctypes.c_void_p()
    create = L.fn("rnd_create")
    assert create(null, side.target.h, ctypes.byref(cfg), 16, ctypes.byref(out)) == BAD and create(side.predictor.h, null, ctypes.byref(cfg), 16, ctypes.byref(out)) == BAD
    assert create(side.predictor.h, side.target.h, null, 16, ctypes.byref(out)) == BAD and create(side.predictor.h, side.target.h, ctypes.byref(cfg), 16, null) == BAD
    assert create(side.predictor.h, side.target.h, ctypes.byref(cfg), 0, ctypes.byref(out)) == BAD
    assert create(side.predictor.h, other.target.h, ctypes.byref(cfg), 16, ctypes.byref(out)) == BAD          # last widths 12 and 1
    assert create(side.predictor.h, side.predictor.h, ctypes.byref(cfg), 16, ctypes.byref(out)) == BAD
    assert create(side.predictor.h, side.target.h, ctypes.byref(RndCfg(0.0, 0.9, 0.999, 1e-8, 0)), 16, ctypes.byref(out)) == BAD
    s, rew, a, b = torch.zeros(16, 45, device=DEV), torch.zeros(16, device=DEV), torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    idx = torch.arange(16, dtype=torch.int32, device=DEV)
    side.h.minibatch_grad(s + 1.0, idx)
    before = bits(side.h.export("GRADS"))
    step = L.fn("rnd_step")
    w = ctypes.c_double(1.0)
    assert step(null, p(s), p(rew), 16, w, p(a), p(b), st) == BAD and step(h, null, p(rew), 16, w, p(a), p(b), st) == BAD
    assert step(h, p(s), null, 16, w, p(a), p(b), st) == BAD and step(h, p(s), p(rew), 16, w, null, p(b), st) == BAD and step(h, p(s), p(rew), 16, w, p(a), null, st) == BAD
    assert step(h, p(s), p(rew), -1, w, p(a), p(b), st) == BAD and step(h, p(s), p(rew), 17, w, p(a), p(b), st) == BAD
    assert step(h, p(s), p(rew), 0, w, p(a), p(b), st) == 0
    mb = L.fn("rnd_minibatch_grad")
    assert mb(null, p(s), p(idx), 16, st) == BAD and mb(h, null, p(idx), 16, st) == BAD and mb(h, p(s), null, 16, st) == BAD
    assert mb(h, p(s), p(idx), 0, st) == BAD and mb(h, p(s), p(idx), 17, st) == BAD
    upd = L.fn("rnd_update")
    assert upd(null, p(s), p(idx), 16, 1, 1, st) == BAD and upd(h, null, p(idx), 16, 1, 1, st) == BAD and upd(h, p(s), null, 16, 1, 1, st) == BAD
    assert upd(h, p(s), p(idx), 34, 1, 2, st) == BAD and upd(h, p(s), p(idx), 16, 0, 1, st) == BAD and upd(h, p(s), p(idx), 16, 1, 0, st) == BAD
    assert upd(h, p(s), p(idx), 1, 1, 2, st) == BAD
    assert L.fn("rnd_apply")(null, st) == BAD and L.fn("rnd_stats")(null, p(s), st) == BAD and L.fn("rnd_stats")(h, null, st) == BAD
    assert L.fn("rnd_export")(null, 1, p(s), st) == BAD and L.fn("rnd_export")(h, 7, p(s), st) == BAD and L.fn("rnd_import")(h, 1, null, st) == BAD
    assert L.fn("rnd_set_step")(h, ctypes.c_longlong(-1), ctypes.c_double(1e-3), st) == BAD and L.fn("rnd_destroy")(null) == BAD
    f = ctypes.c_float()
    cnt = ctypes.c_int64()
    assert L.fn("rnd_get_reward_state")(h, null, ctypes.byref(f), ctypes.byref(f), ctypes.byref(cnt), null, 0, st) == BAD
    assert L.fn("rnd_get_reward_state")(h, ctypes.byref(f), ctypes.byref(f), ctypes.byref(f), ctypes.byref(cnt), null, 17, st) == BAD
    assert L.fn("rnd_set_reward_state")(h, ctypes.c_float(0), ctypes.c_float(1), ctypes.c_float(1), ctypes.c_int64(-1), null, 0, st) == BAD
    stt, _ = side.stats()
    assert np.array_equal(bits(side.h.export("GRADS")), before) and stt["minibatches"] == 1 and stt["step"] == 0, "a refused call must not have launched anything"
