"""The HIP library's distillation with a recurrent student (include/go2sim_rdistill.h) against the torch float64 reference of tests/rdistill_ref.py over the
cases of tests/rdistill_cases.py, with the float32 torch evaluation of the same expressions as the yardstick:
  (a) go2sim_rdistill_act:   bit-equal to go2sim_lstm_step followed by go2sim_distill_act on h', with and without a recurrent teacher, over three steps with dones
  (b) window gradients, per tensor (the MLP's and the four LSTM tensors):  max|g - g64| <= C_GRAD max(max|g32 - g64|, 2^-24 max|g64|)
  (c) whole updates, per tensor:  max|p - p64| <= C_UPD max|p32 - p64|; the final state under C_MLP; the loss statistic equal to a float64 evaluation on the
      library's own float32 means to 1e-12 relative; the dropped tail moves the state and the statistic, not the parameters
  (d) a window walked in three env blocks against one block: both under C_GRAD, each bit-reproducible
  (e) the optimizer state's round trip and the status codes.
C_GRAD = 16, C_UPD = 8 (include/go2sim_train.h) and C_MLP = 7 (include/go2sim_policy.h) are the project's own constants.  Every test prints its ratios
before it asserts; include/go2sim_rdistill.h records the worst measured on the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import rdistill_cases as RC

pytestmark = pytest.mark.gpu

C_GRAD = RC.C_GRAD
C_UPD = 8
C_MLP = 7
EPS = RC.EPS
DEV = "cuda:0"
SUB_ENVS = 1024                                             # GO2SIM_RDISTILL_SUB_ENVS, asserted in test_bad_arguments_return_a_status_and_launch_nothing


def r16(v):
    return (v + 15) // 16 * 16


def real_entry_mask(sdims, n_in):
    """the entries of the padded vector student | memory_s that are parameters"""
    parts = []
    for l in range(len(sdims) - 1):
        w = np.zeros((r16(sdims[l + 1]), r16(sdims[l])), bool); w[:sdims[l + 1], :sdims[l]] = True
        b = np.zeros(r16(sdims[l + 1]), bool); b[:sdims[l + 1]] = True
        parts += [w.reshape(-1), b]
    H, Hp = sdims[0], r16(sdims[0])
    for cols, cp in ((n_in, r16(n_in)), (H, Hp)):
        w = np.zeros((4, Hp, cp), bool); w[:, :H, :cols] = True
        parts.append(w.reshape(-1))
    for _ in range(2):
        b = np.zeros((4, Hp), bool); b[:, :H] = True
        parts.append(b.reshape(-1))
    return np.concatenate(parts)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def ratio(got, ref64, ref32):
    err, yard = float((got.double().cpu() - ref64).abs().max()), max(float((ref32.double() - ref64).abs().max()), EPS * float(ref64.abs().max()))
    return 0.0 if err == 0.0 else err / yard if yard > 0.0 else float("inf")      # an all-zero reference (every env done) is met exactly or not at all


class Side:
    """memory_s, the student, the rollout and one go2sim_rdistill handle on the GPU"""

    def __init__(self, lib, n_in, sdims, state, obs, ta, dones, S, max_rows, carried=None, **hyper):
        from go2_sim2real_locomotion_rl_amd.distillation import RDistillHandle
        from go2_sim2real_locomotion_rl_amd.policy import Lstm, Mlp, flatten_lstm, flatten_sequential

        self.lib, self.n_in, self.sdims = lib, n_in, sdims
        self.student = Mlp(lib, sdims, flatten_sequential(state, "student", len(sdims) - 1)[0])
        self.memory = Lstm(lib, n_in, sdims[0], flatten_lstm(state, "memory_s")[0])
        self.obs, self.ta, self.dones = obs.to(DEV).contiguous(), ta.to(DEV).contiguous(), dones.to(DEV).contiguous()
        self.S = tuple(s.to(DEV).contiguous() for s in S)
        self.state = tuple((c if carried is not None else s).to(DEV).clone().contiguous() for c, s in zip(carried or S, S))      # the carried state, in and out
        self.T, self.N = obs.shape[0], obs.shape[1]
        self.h = RDistillHandle(lib, self.memory, self.student, sdims[-1], max_rows, **hyper)
        self.roll = self.h.roll(self.obs, self.ta, self.dones, *self.S, *self.state, self.T, self.N)

    def split(self, flat):
        from go2_sim2real_locomotion_rl_amd.distillation import unflatten_recurrent_student

        return {k: v.double() for k, v in unflatten_recurrent_student(flat.cpu(), self.sdims, (self.n_in, self.sdims[0])).items()}

    def stats(self):
        s = self.h.stats().cpu()
        return dict(loss=float(s[0]), lr=float(s[1]), grad_norm=float(s[2]), step=int(s[3]), pairs=int(s[4]), windows=int(s[5])), s

    def act_loop(self, steps, start, first_reset=None):
        """the library's own means of consecutive `steps` from state `start` through deterministic go2sim_rdistill_act calls whose reset is the previous
        step's dones (`first_reset` for the first): -> (means [len][N][A], (h, c) after the last step, unmasked)"""
        from go2_sim2real_locomotion_rl_amd.distillation import rdistill_act

        A, N = self.sdims[-1], self.N
        std = torch.zeros(A, device=DEV)
        tobs = torch.zeros(N, self.sdims[0], device=DEV)                    # the student stands in as an MLP teacher: it reads [N][H] rows
        h, c = start[0].clone(), start[1].clone()
        spare = torch.empty_like(h)
        means, reset = [], first_reset
        for t in steps:
            out = [torch.empty(N, A, device=DEV) for _ in range(3)]
            rdistill_act(self.lib, self.memory, self.student, None, self.student, self.obs[t], tobs, std, reset, (h, c, spare, c), None, N, 1, 0, True, *out)
            h, spare = spare, h
            means.append(out[1])
            reset = self.dones[t]
        return torch.stack(means), (h, c)


def window_side(lib, c, sub=None, **hyper):
    sub = c.sub if sub is None else sub
    rows = c.P * min(c.N, sub if sub else SUB_ENVS)
    return Side(lib, c.I, c.sdims, c.state, c.obs, c.ta, c.dones, c.S, rows, carried=c.carried, loss_type=c.loss_type, sub_envs=sub, **hyper)


def update_side(lib, u, **hyper):
    rows = u["G"] * min(u["N"], u["sub"] if u["sub"] else SUB_ENVS)
    hp = dict(learning_rate=u["hp"]["learning_rate"], max_grad_norm=u["hp"]["max_grad_norm"], loss_type=u["hp"]["loss_type"], sub_envs=u["sub"])
    hp.update(hyper)
    return Side(lib, u["I"], u["sdims"], u["state"], u["obs"], u["ta"], u["dones"], u["S"], rows, **hp)


def f64_loss(mu, ta, loss_type):
    """sum over the pairs of l_t from means [P][N][A] in float64"""
    d = mu.double().cpu() - ta.double()
    rho = d * d if loss_type == "mse" else torch.where(d.abs() <= 1, d * d / 2, d.abs() - 0.5)
    return float(rho.reshape(rho.shape[0], -1).mean(1).sum())


# ---- (a) the collection step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("shape", [(5, 16, 9, 20, 1), (49, 20, 104, 48, 17), (49, 48, 49, 16, 70)], ids=lambda s: "I%d-H%d-It%d-Ht%d-N%d" % s)
def test_act_equals_lstm_step_then_distill_act(hip_lib, shape, teacher_recurrent, deterministic):
    from go2_sim2real_locomotion_rl_amd.distillation import distill_act, rdistill_act
    from go2_sim2real_locomotion_rl_amd.policy import Lstm, Mlp, flatten_lstm, flatten_sequential, lstm_step

    I, H, It, Ht, N = shape
    g = torch.Generator().manual_seed(100 + N)
    sdims, tdims = [H, 24, RC.A], [Ht if teacher_recurrent else It, 40, 24, RC.A]
    state = RC.init_state(I, sdims, g)
    tstate = {k.replace("student", "teacher").replace("memory_s", "memory_t"): v for k, v in RC.init_state(It, tdims, g).items()}   # memory_t is used by a recurrent teacher only
    student, teacher = Mlp(hip_lib, sdims, flatten_sequential(state, "student", 2)[0]), Mlp(hip_lib, tdims, flatten_sequential(tstate, "teacher", 3)[0])
    mem_s = Lstm(hip_lib, I, H, flatten_lstm(state, "memory_s")[0])
    mem_t = Lstm(hip_lib, It, Ht, flatten_lstm(tstate, "memory_t")[0]) if teacher_recurrent else None
    std = torch.full((RC.A,), 0.3, device=DEV)
    dones = RC.make_dones(3, N, [(0, 0), (1, 5), (2, 3)], g).to(DEV)
    z = lambda w: (0.5 * torch.randn(N, w, generator=g)).to(DEV)
    new = lambda: torch.full((N, RC.A), float("nan"), device=DEV)
    hs, cs, ht, ct = z(H), z(H), z(Ht), z(Ht)                                # the fused side's state
    hs2, cs2, ht2, ct2 = hs.clone(), cs.clone(), ht.clone(), ct.clone()    # the composition's
    reset, seed = None, 0x1234567890
    for t in range(3):
        obs, tobs = torch.randn(N, I, generator=g).to(DEV), torch.randn(N, It, generator=g).to(DEV)
        act, mean, tact, act2, mean2, tact2 = (new() for _ in range(6))
        hs_o, ht_o, hs2_o, ht2_o = torch.empty_like(hs), torch.empty_like(ht), torch.empty_like(hs), torch.empty_like(ht)
        rdistill_act(hip_lib, mem_s, student, mem_t, teacher, obs, tobs, std, reset, (hs, cs, hs_o, cs), (ht, ct, ht_o, ct) if teacher_recurrent else None, N, seed, t,
                     deterministic, act, mean, tact)
        lstm_step(hip_lib, mem_s, obs, hs2, cs2, hs2_o, cs2, mem_t, tobs if teacher_recurrent else None, ht2 if teacher_recurrent else None,
                  ct2 if teacher_recurrent else None, ht2_o if teacher_recurrent else None, ct2 if teacher_recurrent else None, reset=reset, n_rows=N)
        distill_act(hip_lib, student, teacher, hs2_o, ht2_o if teacher_recurrent else tobs, std, N, seed, t, deterministic, act2, mean2, tact2)
        torch.cuda.synchronize()
        for name, x, y in (("actions", act, act2), ("mean", mean, mean2), ("teacher_actions", tact, tact2), ("h_s", hs_o, hs2_o), ("c_s", cs, cs2)):
            assert np.array_equal(bits(x), bits(y)), (t, name)
        if teacher_recurrent:
            assert np.array_equal(bits(ht_o), bits(ht2_o)) and np.array_equal(bits(ct), bits(ct2)), t
            ht, ht2 = ht_o, ht2_o
        assert np.isfinite(act.cpu().numpy()).all() and np.isfinite(tact.cpu().numpy()).all()
        assert np.array_equal(bits(act), bits(mean)) == bool(deterministic)
        hs, hs2, reset = hs_o, hs2_o, dones[t]
    # the reset is part of the launch: a done row's new state is that of a zero state.  Step a zeroed copy without a reset and compare
    obs, width_h = torch.randn(N, I, generator=g).to(DEV), torch.zeros(N, H, device=DEV)
    assert reset.any()
    hz, cz = hs.clone(), cs.clone()
    hz[reset.bool()] = 0; cz[reset.bool()] = 0
    o1, o2 = torch.empty_like(hs), torch.empty_like(hs)
    lstm_step(hip_lib, mem_s, obs, hz, cz, o1, cz, n_rows=N)
    out = [new() for _ in range(3)]
    rdistill_act(hip_lib, mem_s, student, None, student, obs, width_h, std, reset, (hs, cs, o2, cs), None, N, seed, 3, True, *out)   # the student stands in as an MLP teacher on [N][H] rows
    torch.cuda.synchronize()
    assert np.array_equal(bits(o1), bits(o2)) and np.array_equal(bits(cz), bits(cs))


# ---- (b) one window --------------------------------------------------------------------------------------------------------------------------------------
def check_window(side, c, tag):
    g64, l64, mu64, st64 = c.ref["f64"]
    g32, _, mu32, st32 = c.ref["f32"]
    got = side.split(side.h.export("GRADS"))
    worst = 0.0
    for k in g64:
        q = ratio(got[k], g64[k], g32[k])
        print(f"RATIO grad {tag} {k} {q:.3f}")
        worst = max(worst, q)
    print(f"RATIO worst grad {tag} {worst:.3f}")
    return worst, got


@pytest.mark.parametrize("name", sorted(RC.WINDOW_CASES))
def test_window_gradients(hip_lib, name):
    c = RC.get_window_case(name)
    g64, l64, mu64, st64 = c.ref["f64"]
    _, _, mu32, st32 = c.ref["f32"]
    side = window_side(hip_lib, c)
    p0 = bits(side.h.export_padded("PARAMS"))
    side.h.window_grad(side.roll, c.segs)
    worst, got = check_window(side, c, name)
    assert worst <= C_GRAD
    assert np.array_equal(bits(got["memory_s.rnn.bias_ih_l0"].float()), bits(got["memory_s.rnn.bias_hh_l0"].float())), "b_ih and b_hh have equal gradients"
    padded = side.h.export_padded("GRADS").cpu().numpy()
    assert np.isfinite(padded).all() and not padded[~real_entry_mask(c.sdims, c.I)].any(), "padded gradient entries must be exactly zero"
    assert np.array_equal(bits(side.h.export_padded("PARAMS")), p0), "a gradient moves no parameter"
    st, _ = side.stats()
    assert st["pairs"] == c.P and st["windows"] == 0 and st["step"] == 0
    # the state the window leaves: the last step's, its dones applied
    for nm, x, r64, r32 in (("h", side.state[0], st64[0], st32[0]), ("c", side.state[1], st64[1], st32[1])):
        q = ratio(x, r64, r32)
        print(f"RATIO state {name} {nm} {q:.3f}")
        assert q <= C_MLP
    t_last = c.segs[-1][0] + c.segs[-1][1] - 1
    done = c.dones[t_last].bool()
    assert not side.state[0].cpu()[done].any() and not side.state[1].cpu()[done].any()
    # the loss statistic on the library's own means: the same window through the collection step
    means, hc = [], None
    for k, (t0, n) in enumerate(c.segs):
        start = side.S if t0 == 0 else tuple(x.to(DEV) for x in c.carried)
        mu, hc = side.act_loop(range(t0, t0 + n), start, None if t0 == 0 else side.dones[t0 - 1])
        means.append(mu)
    mu = torch.cat(means)
    q = ratio(mu, mu64, mu32)
    print(f"RATIO mean {name} {q:.3f}")
    assert q <= C_MLP
    ta = torch.stack([c.ta[t] for t0, n in c.segs for t in range(t0, t0 + n)])
    want = f64_loss(mu, ta, c.loss_type) / c.P
    print(f"RATIO loss {name} {abs(st['loss'] - want) / want:.3e}")
    assert abs(st["loss"] - want) <= 1e-12 * want
    assert st["loss"] == pytest.approx(sum(l64) / c.P, rel=1e-5)            # against the float64 law: fp32 forward passes, a sanity bound
    keep = ~done
    assert np.array_equal(bits(side.state[0].cpu()[keep]), bits(hc[0].cpu()[keep])), "the carried state is the collection step's, bit for bit"
    # the tail's pass over the same window: the sum and the count double, the gradient stays
    before = bits(side.h.export("GRADS"))
    state0 = tuple(bits(s) for s in side.state)
    for s, x in zip(side.state, c.carried):
        s.copy_(x.to(DEV))
    side.h.loss_only(side.roll, c.segs)
    st2, _ = side.stats()
    assert st2["pairs"] == 2 * c.P and abs(st2["loss"] - want) <= 1e-12 * want and np.array_equal(bits(side.h.export("GRADS")), before)
    if c.segs[0][0] == 0:
        assert all(np.array_equal(bits(s), b) for s, b in zip(side.state, state0))


# ---- (c) whole updates -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.UPDATE_CASES))
def test_whole_update(hip_lib, name):
    u = RC.get_update_case(name)
    T, E, G, N = u["T"], u["E"], u["G"], u["N"]
    side = update_side(hip_lib, u)
    p0 = bits(side.h.export_padded("PARAMS"))
    S0 = tuple(bits(s) for s in side.S)
    side.h.update(side.obs, side.ta, side.dones, *side.S, *side.state, T, N, E, G)
    got = side.split(side.h.export("PARAMS"))
    st, _ = side.stats()
    n_win = (E * T) // G
    assert st["step"] == n_win and st["windows"] == n_win and st["pairs"] == E * T and st["lr"] == u["hp"]["learning_rate"]
    assert st["loss"] == pytest.approx(u["f64"]["loss"], rel=1e-5)         # fp32 forward passes: a sanity bound
    assert all(np.array_equal(bits(s), b) for s, b in zip(side.S, S0)), "S is a constant of the update"
    for nm, x, r64, r32 in (("h", side.state[0], u["f64"]["state"][0], u["f32"]["state"][0]), ("c", side.state[1], u["f64"]["state"][1], u["f32"]["state"][1])):
        q = ratio(x, r64, r32)
        print(f"RATIO state {name} {nm} {q:.3f}")
        assert q <= C_MLP
    done = u["dones"][T - 1].bool()
    assert not side.state[0].cpu()[done].any() and not side.state[1].cpu()[done].any() and (bool(done.all()) or side.state[0].cpu()[~done].any())
    if n_win == 0:
        # (2, 1, 5): everything is a dropped tail.  The parameters stay bit for bit; the state and the statistic move, and both are the collection step's:
        # the float64 loss on the library's own means to 1e-12, the state bit for bit
        assert np.array_equal(bits(side.h.export_padded("PARAMS")), p0) and st["loss"] > 0
        for which in ("ADAM_M", "ADAM_V"):
            assert not side.h.export_padded(which).cpu().numpy().any(), which
        mu, hc = side.act_loop(range(T), side.S)
        want = f64_loss(mu, u["ta"], u["hp"]["loss_type"]) / T
        print(f"RATIO loss {name} {abs(st['loss'] - want) / want:.3e}")
        assert abs(st["loss"] - want) <= 1e-12 * want
        assert np.array_equal(bits(side.state[0].cpu()[~done]), bits(hc[0].cpu()[~done])) and np.array_equal(bits(side.state[1].cpu()[~done]), bits(hc[1].cpu()[~done]))
        assert not np.array_equal(bits(side.state[0]), S0[0])
        return
    worst = 0.0
    for k, p64 in u["f64"]["params"].items():
        err, yard = float((got[k] - p64).abs().max()), float((u["f32"]["params"][k].double() - p64).abs().max())
        print(f"RATIO update {name} {k} {err / yard:.3f}")
        worst = max(worst, err / yard)
    print(f"RATIO worst update {name} {worst:.3f}")
    assert worst <= C_UPD
    assert st["grad_norm"] == pytest.approx(u["f64"]["norms"][-1], rel=1e-4)
    mask = real_entry_mask(u["sdims"], u["I"])
    for which in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V"):
        assert not side.h.export_padded(which).cpu().numpy()[~mask].any(), which


def test_dropped_tail_moves_state_and_statistic_not_parameters(hip_lib):
    """(3, 2, 4): the tail's two pairs change nothing the window's Adam step left, yet the statistic counts them and the state is theirs"""
    u = RC.get_update_case("T3E2G4")
    a, b = update_side(hip_lib, u), update_side(hip_lib, u)
    a.h.update(a.obs, a.ta, a.dones, *a.S, *a.state, u["T"], u["N"], u["E"], u["G"])
    # by hand: the one window, its step, then nothing
    b.h.reset_stats()
    b.h.window_grad(b.roll, [(0, 3), (0, 1)])
    b.h.apply()
    mid = tuple(bits(s) for s in b.state)
    sb, _ = b.stats()
    for which in ("PARAMS", "ADAM_M", "ADAM_V", "GRADS"):
        assert np.array_equal(bits(a.h.export(which)), bits(b.h.export(which))), which
    sa, _ = a.stats()
    assert sa["pairs"] == 6 and sb["pairs"] == 4 and sa["windows"] == sb["windows"] == 1
    assert not np.array_equal(bits(a.state[0]), mid[0])
    b.h.loss_only(b.roll, [(1, 2)])
    assert np.array_equal(a.stats()[1].numpy().view(np.int64), b.stats()[1].numpy().view(np.int64))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a.state, b.state))
    assert abs(sa["loss"] * 6 - sb["loss"] * 4) > 1e-6                      # the tail's two pairs are in the sum


# ---- (d) env blocks ----------------------------------------------------------------------------------------------------------------------------------------
def test_env_blocks_hold_the_bound_and_their_bits(hip_lib):
    c = RC.get_window_case("done_cut")                                      # 37 envs: sub_envs = 16 walks blocks of 16, 16 and 5
    out = {}
    for sub in (16, 0):
        runs = []
        for _ in range(2):
            side = window_side(hip_lib, c, sub=sub)
            side.h.window_grad(side.roll, c.segs)
            worst, _ = check_window(side, c, f"done_cut-sub{sub}")
            assert worst <= C_GRAD
            runs.append([bits(side.h.export_padded("GRADS")), bits(side.state[0]), bits(side.state[1]), side.stats()[1].numpy().view(np.int64).copy()])
        for x, y in zip(*runs):
            assert np.array_equal(x, y), f"sub_envs = {sub}: two runs must give equal bits"
        out[sub] = runs[0]
    assert np.array_equal(out[16][1], out[0][1]) and np.array_equal(out[16][2], out[0][2]), "the forward state does not depend on the blocks"
    assert np.abs(out[16][0].view(np.float32)).max() > 0


def test_update_in_blocks_is_bit_reproducible(hip_lib):
    u = RC.get_update_case("T4E2G4-blocks")
    runs = []
    for _ in range(2):
        side = update_side(hip_lib, u)
        side.h.update(side.obs, side.ta, side.dones, *side.S, *side.state, u["T"], u["N"], u["E"], u["G"])
        runs.append([bits(side.h.export(w)) for w in ("PARAMS", "ADAM_M", "ADAM_V", "GRADS")] + [bits(side.state[0]), bits(side.state[1]), side.stats()[1].numpy().view(np.int64).copy()])
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


# ---- (e) optimizer state and status codes ------------------------------------------------------------------------------------------------------------------
def test_optimizer_state_round_trip(hip_lib):
    """export, import and set_step carry the optimizer from one handle to another: the next update gives equal bits"""
    u = RC.get_update_case("T4E1G3-below")
    args = lambda s: (s.obs, s.ta, s.dones, *s.S, *s.state, u["T"], u["N"], u["E"], u["G"])
    a = update_side(hip_lib, u)
    a.h.update(*args(a))
    b = update_side(hip_lib, u)
    for which in ("PARAMS", "ADAM_M", "ADAM_V"):
        b.h.import_(which, a.h.export(which))
    sa, _ = a.stats()
    assert sa["step"] == 1 and a.h.n_params == sum(v.numel() for k, v in u["state"].items()) and a.h.n_padded == real_entry_mask(u["sdims"], u["I"]).size
    b.h.set_step(sa["step"], sa["lr"])
    for x, y in zip(b.state, a.state):
        x.copy_(y)
    for side in (a, b):
        side.h.update(*args(side))
    for which in ("PARAMS", "ADAM_M", "ADAM_V", "GRADS"):
        assert np.array_equal(bits(a.h.export(which)), bits(b.h.export(which))), which
        assert np.array_equal(bits(a.h.export_padded(which)), bits(b.h.export_padded(which))), which
    assert np.array_equal(a.stats()[1].numpy().view(np.int64), b.stats()[1].numpy().view(np.int64)) and a.stats()[0]["step"] == 2
    assert np.abs(bits(a.h.export("ADAM_M")).view(np.float32)).max() > 0
    a.h.reset_stats()
    s, _ = a.stats()
    assert s["loss"] == 0.0 and s["pairs"] == 0 and s["windows"] == 0 and s["step"] == 2


def test_bad_arguments_return_a_status_and_launch_nothing(hip_lib):
    from go2_sim2real_locomotion_rl_amd.capi import C, RDistillCfg, RDistillRoll, RDistillSeg
    from go2_sim2real_locomotion_rl_amd.policy import Lstm, Mlp, flatten_lstm, flatten_sequential

    BAD, null, st = C["GO2SIM_E_BADARG"], ctypes.c_void_p(0), ctypes.c_void_p(0)
    assert C["GO2SIM_RDISTILL_SUB_ENVS"] == SUB_ENVS
    c = RC.get_window_case("plain")                                         # I = 5, H = 16, 17 envs, T = 3
    side = window_side(hip_lib, c)                                          # workspace: 3 x 17 rows
    L, h = hip_lib, side.h.h
    cfg = RDistillCfg(1e-3, 0.0, 0.9, 0.999, 1e-8, 0, 0)
    out = ctypes.c_void_p()
    create = L.fn("rdistill_create")
    g = torch.Generator().manual_seed(1)
    other = RC.init_state(5, [20, 24, RC.A], g)
    mem20 = Lstm(L, 5, 20, flatten_lstm(other, "memory_s")[0])               # H = 20 against a student whose first width is 16
    wide = Mlp(L, [16, 24, 16], flatten_sequential(RC.init_state(5, [16, 24, 16], g), "student", 2)[0])   # ends in 16 actions, not 12
    A = RC.A
    assert create(null, side.student.h, A, ctypes.byref(cfg), 51, ctypes.byref(out)) == BAD and create(side.memory.h, null, A, ctypes.byref(cfg), 51, ctypes.byref(out)) == BAD
    assert create(side.memory.h, side.student.h, A, null, 51, ctypes.byref(out)) == BAD and create(side.memory.h, side.student.h, A, ctypes.byref(cfg), 51, null) == BAD
    assert create(mem20.h, side.student.h, A, ctypes.byref(cfg), 51, ctypes.byref(out)) == BAD                  # H mismatch between memory and the MLP's first width
    assert create(side.memory.h, side.student.h, A + 1, ctypes.byref(cfg), 51, ctypes.byref(out)) == BAD       # the student's last width is 12
    assert create(side.memory.h, side.student.h, A, ctypes.byref(cfg), 0, ctypes.byref(out)) == BAD
    assert create(side.memory.h, side.student.h, A, ctypes.byref(RDistillCfg(1e-3, 0.0, 0.9, 0.999, 1e-8, 2, 0)), 51, ctypes.byref(out)) == BAD   # no such loss
    assert create(side.memory.h, side.student.h, A, ctypes.byref(RDistillCfg(1e-3, 0.0, 0.9, 0.999, 1e-8, 0, -1)), 51, ctypes.byref(out)) == BAD
    assert create(side.memory.h, side.student.h, A, ctypes.byref(RDistillCfg(0.0, 0.0, 0.9, 0.999, 1e-8, 0, 0)), 51, ctypes.byref(out)) == BAD
    side.h.window_grad(side.roll, c.segs)
    before, state0 = bits(side.h.export("GRADS")), tuple(bits(s) for s in side.state)
    segs = lambda *s: (RDistillSeg * len(s))(*[RDistillSeg(*x) for x in s])
    roll = side.roll
    def changed(**kw):
        r = RDistillRoll(*[getattr(roll, n) for n, _ in RDistillRoll._fields_])
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    for name in ("rdistill_window_grad", "rdistill_loss_only"):
        f = L.fn(name)
        assert f(null, ctypes.byref(roll), segs((0, 3)), 1, st) == BAD and f(h, null, segs((0, 3)), 1, st) == BAD and f(h, ctypes.byref(roll), null, 1, st) == BAD
        for field in ("obs", "teacher_actions", "dones", "h0", "c0", "h", "c"):
            assert f(h, ctypes.byref(changed(**{field: None})), segs((0, 3)), 1, st) == BAD, field
        assert f(h, ctypes.byref(changed(h=roll.h0)), segs((0, 3)), 1, st) == BAD                                # S is never written
        assert f(h, ctypes.byref(roll), segs((0, 3)), 0, st) == BAD and f(h, ctypes.byref(roll), segs((0, 0)), 1, st) == BAD
        assert f(h, ctypes.byref(roll), segs((0, 4)), 1, st) == BAD and f(h, ctypes.byref(roll), segs((1, 3)), 1, st) == BAD   # steps beyond T = 3
        assert f(h, ctypes.byref(roll), segs((0, 2), (1, 1)), 2, st) == BAD                                    # only a window's first segment starts inside an epoch
        assert f(h, ctypes.byref(roll), segs((0, 3), (0, 1)), 2, st) == BAD                                    # 4 pairs x 17 envs over the workspace of 51 rows
        assert f(h, ctypes.byref(changed(n_envs=0)), segs((0, 3)), 1, st) == BAD and f(h, ctypes.byref(changed(n_steps=0)), segs((0, 1)), 1, st) == BAD
    upd = L.fn("rdistill_update")
    assert upd(null, ctypes.byref(roll), 1, 3, st) == BAD and upd(h, null, 1, 3, st) == BAD
    assert upd(h, ctypes.byref(roll), 2, 4, st) == BAD                                                        # G x sub_envs over the workspace
    assert upd(h, ctypes.byref(roll), 0, 3, st) == BAD and upd(h, ctypes.byref(roll), 1, 0, st) == BAD
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    buf = torch.zeros(8, dtype=torch.float64, device=DEV)
    assert L.fn("rdistill_apply")(null, st) == BAD and L.fn("rdistill_stats")(null, p(buf), st) == BAD and L.fn("rdistill_stats")(h, null, st) == BAD
    assert L.fn("rdistill_export")(null, 1, p(buf), st) == BAD and L.fn("rdistill_export")(h, 7, p(buf), st) == BAD and L.fn("rdistill_import")(h, 1, null, st) == BAD
    assert L.fn("rdistill_export_padded")(h, 4, p(buf), st) == BAD and L.fn("rdistill_export_padded")(h, 0, null, st) == BAD
    assert L.fn("rdistill_set_step")(h, ctypes.c_longlong(-1), ctypes.c_double(1e-3), st) == BAD and L.fn("rdistill_destroy")(null) == BAD
    n = ctypes.c_size_t()
    assert L.fn("rdistill_n_params")(h, null) == BAD and L.fn("rdistill_n_padded")(null, ctypes.byref(n)) == BAD
    # the collection step: widths that do not match, NULL arrays, h_out = h_in
    act = L.fn("rdistill_act")
    N = c.N
    a = [torch.zeros(N, A, device=DEV) for _ in range(3)]
    hs = [torch.zeros(N, 16, device=DEV) for _ in range(3)]
    std = torch.ones(A, device=DEV)
    obs = side.obs[0]
    def args(**kw):
        return [kw.get("ms", side.memory.h), kw.get("s", side.student.h), kw.get("mt", null), kw.get("t", side.student.h), kw.get("obs", p(obs)), kw.get("tobs", p(hs[0])),
                kw.get("std", p(std)), null, kw.get("hi", p(hs[0])), kw.get("ci", p(hs[1])), kw.get("ho", p(hs[2])), kw.get("co", p(hs[1])), kw.get("hti", null), null, null, null,
                N, ctypes.c_uint64(1), ctypes.c_uint32(0), 0, kw.get("a0", p(a[0])), kw.get("a1", p(a[1])), kw.get("a2", p(a[2])), st]
    for k in ("ms", "s", "t", "obs", "tobs", "std", "hi", "ci", "ho", "co", "a0", "a1", "a2"):
        assert act(*args(**{k: null})) == BAD, k
    assert act(*args(ms=mem20.h)) == BAD and act(*args(t=wide.h)) == BAD and act(*args(ho=p(hs[0]))) == BAD
    assert act(*args(mt=side.memory.h)) == BAD                                                                 # a recurrent teacher needs its state arrays
    assert act(*args()) == 0
    s, _ = side.stats()
    assert np.array_equal(bits(side.h.export("GRADS")), before) and s["pairs"] == c.P and s["step"] == 0 and s["windows"] == 0, "a refused call must not have launched anything"
    assert all(np.array_equal(bits(x), b) for x, b in zip(side.state, state0))
