"""What the recurrent distillation (include/go2sim_rdistill.h) promises without a GPU: the segment schedule against hand-written lists, both checkpoint
mappings and their refusals, the torch reference (tests/rdistill_ref.py) against a hand evaluation, the C ABI's list, the package's exports and the margins
of the case table the GPU tests run (tests/rdistill_cases.py)."""
import ctypes
import math
import os
import re

import pytest
import torch

import rdistill_cases as RC
import rdistill_ref as R
from go2_sim2real_locomotion_rl_amd import capi
from go2_sim2real_locomotion_rl_amd.capi import Go2SimError
from go2_sim2real_locomotion_rl_amd.distillation import distill_windows, rdistill_schedule, teacher_state_from_checkpoint


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------------------------
def test_segment_schedule_against_hand_written_lists():
    assert rdistill_schedule(3, 2, 4) == ([[(0, 0, 2), (1, 0, 0)]], [(1, 1, 2)])
    assert rdistill_schedule(2, 2, 3) == ([[(0, 0, 1), (1, 0, 0)]], [(1, 1, 1)])
    assert rdistill_schedule(2, 1, 5) == ([], [(0, 0, 1)])
    assert rdistill_schedule(4, 1, 3) == ([[(0, 0, 2)]], [(0, 3, 3)])
    assert rdistill_schedule(3, 1, 1) == ([[(0, 0, 0)], [(0, 1, 1)], [(0, 2, 2)]], [])
    w, tail = rdistill_schedule(24, 5, 15)                                  # the training shape: 120 pairs, 8 windows, no tail
    assert tail == [] and len(w) == 8
    assert w[0] == [(0, 0, 14)] and w[1] == [(0, 15, 23), (1, 0, 5)] and w[2] == [(1, 6, 20)] and w[3] == [(1, 21, 23), (2, 0, 11)]
    assert w[4] == [(2, 12, 23), (3, 0, 2)] and w[5] == [(3, 3, 17)] and w[6] == [(3, 18, 23), (4, 0, 8)] and w[7] == [(4, 9, 23)]
    w, tail = rdistill_schedule(2, 3, 5)                                    # G > 2 T: a window of three segments
    assert w == [[(0, 0, 1), (1, 0, 1), (2, 0, 0)]] and tail == [(2, 1, 1)]


@pytest.mark.parametrize("sched", [(3, 2, 4), (2, 2, 3), (2, 1, 5), (24, 5, 15), (4, 2, 4), (1, 7, 3)])
def test_segments_are_the_windows_pairs(sched):
    """the segments of a window spell its pairs in order; only a window's first segment starts inside an epoch"""
    windows, tail = distill_windows(*sched)
    seg_windows, seg_tail = rdistill_schedule(*sched)
    for pairs, segs in zip(windows + [tail], seg_windows + [seg_tail]):
        assert [(e, t) for e, t0, t1 in segs for t in range(t0, t1 + 1)] == pairs
        assert all(t0 == 0 for _, t0, _ in segs[1:])
    with pytest.raises(Go2SimError):
        rdistill_schedule(0, 1, 1)


# ---- the checkpoint mappings ----------------------------------------------------------------------------------------------------------------------------
def lstm_sd(prefix, n_in, H):
    return {f"{prefix}.rnn.weight_ih_l0": torch.randn(4 * H, n_in), f"{prefix}.rnn.weight_hh_l0": torch.randn(4 * H, H), f"{prefix}.rnn.bias_ih_l0": torch.randn(4 * H),
            f"{prefix}.rnn.bias_hh_l0": torch.randn(4 * H)}


def mlp_sd(prefix, dims):
    sd = {}
    for l in range(len(dims) - 1):
        sd[f"{prefix}.{2 * l}.weight"], sd[f"{prefix}.{2 * l}.bias"] = torch.randn(dims[l + 1], dims[l]), torch.randn(dims[l + 1])
    return sd


SD, TD, SM, TM = [8, 6, 4], [10, 7, 4], (5, 8), (9, 10)


def test_recurrent_ppo_checkpoint_maps_memory_a_to_memory_t():
    ppo = {**mlp_sd("actor", TD), **mlp_sd("critic", [10, 3, 1]), **lstm_sd("memory_a", *TM), **lstm_sd("memory_c", 9, 10), "std": torch.ones(4)}
    mapped, resume = teacher_state_from_checkpoint(ppo, SD, TD, recurrent=True, student_memory=SM, teacher_memory=TM)
    assert resume is False
    assert sorted(mapped) == sorted(list(mlp_sd("teacher", TD)) + list(lstm_sd("memory_t", *TM)))       # critic, memory_c and std are dropped
    assert all(torch.equal(mapped["teacher." + k[6:]], v) for k, v in ppo.items() if k.startswith("actor."))
    assert all(torch.equal(mapped["memory_t." + k[9:]], v) for k, v in ppo.items() if k.startswith("memory_a."))
    with pytest.raises(Go2SimError, match="memory_a.*teacher has no memory"):                          # a recurrent checkpoint onto a teacher without a memory
        teacher_state_from_checkpoint(ppo, SD, [9, 7, 4], recurrent=True, student_memory=SM, teacher_memory=None)
    plain = {k: v for k, v in ppo.items() if not k.startswith("memory_")}
    with pytest.raises(Go2SimError, match="no memory_a"):                                              # and the converse
        teacher_state_from_checkpoint(plain, SD, TD, recurrent=True, student_memory=SM, teacher_memory=TM)
    mapped, resume = teacher_state_from_checkpoint(plain, SD, TD, recurrent=True, student_memory=SM, teacher_memory=None)
    assert resume is False and sorted(mapped) == sorted(mlp_sd("teacher", TD))
    with pytest.raises(Go2SimError, match=r"memory_t\.rnn\.weight_ih_l0 has shape \(40, 9\), this model's is \(40, 11\)"):
        teacher_state_from_checkpoint(ppo, SD, TD, recurrent=True, student_memory=SM, teacher_memory=(11, 10))
    with pytest.raises(Go2SimError, match=r"teacher\.0\.weight has shape \(7, 10\), this model's is \(7, 12\)"):
        teacher_state_from_checkpoint(ppo, SD, [12, 7, 4], recurrent=True, student_memory=SM, teacher_memory=TM)


def test_recurrent_distillation_checkpoint_resumes():
    full = {**mlp_sd("student", SD), **mlp_sd("teacher", TD), **lstm_sd("memory_s", *SM), **lstm_sd("memory_t", *TM), "std": torch.ones(4)}
    mapped, resume = teacher_state_from_checkpoint(full, SD, TD, recurrent=True, student_memory=SM, teacher_memory=TM)
    assert resume is True and sorted(mapped) == sorted(full)
    no_t = {k: v for k, v in full.items() if not k.startswith("memory_t.")}
    with pytest.raises(Go2SimError, match="no memory_t"):
        teacher_state_from_checkpoint(no_t, SD, TD, recurrent=True, student_memory=SM, teacher_memory=TM)
    with pytest.raises(Go2SimError, match="teacher is recurrent"):
        teacher_state_from_checkpoint(full, SD, TD, recurrent=True, student_memory=SM, teacher_memory=None)
    with pytest.raises(Go2SimError, match="memory_s"):
        teacher_state_from_checkpoint({k: v for k, v in full.items() if not k.startswith("memory_s.")}, SD, TD, recurrent=True, student_memory=SM, teacher_memory=TM)
    with pytest.raises(Go2SimError, match=r"memory_s\.rnn\.weight_ih_l0 has shape \(32, 5\), this model's is \(32, 7\)"):
        teacher_state_from_checkpoint(full, SD, TD, recurrent=True, student_memory=(7, 8), teacher_memory=TM)
    with pytest.raises(Go2SimError, match="unexpected keys"):
        teacher_state_from_checkpoint({**full, "critic.0.weight": torch.ones(1)}, SD, TD, recurrent=True, student_memory=SM, teacher_memory=TM)


def test_default_mapping_still_refuses_memories():
    """without the switch the function is the MLP student's: a recurrent checkpoint is refused by name"""
    ppo = {**mlp_sd("actor", TD), **lstm_sd("memory_a", *TM), "std": torch.ones(4)}
    with pytest.raises(Go2SimError, match="memory_a"):
        teacher_state_from_checkpoint(ppo, SD, TD)
    mapped, resume = teacher_state_from_checkpoint({**mlp_sd("actor", TD), "std": torch.ones(4)}, SD, TD)
    assert resume is False and sorted(mapped) == sorted(mlp_sd("teacher", TD))


# ---- the reference against a hand evaluation ------------------------------------------------------------------------------------------------------------
def hand_losses(p, x, ta, h0, c0, done0):
    """H = 1, I = 1, one env, two steps, student = one Linear(1 -> 1): the law in scalars.  p: wi[4], wh[4], bi[4], bh[4] (gates i, f, g, o), w, b"""
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))
    h, c, out = h0, c0, []
    for t in range(2):
        z = [p["wi"][q] * x[t] + p["wh"][q] * h + p["bi"][q] + p["bh"][q] for q in range(4)]
        i, f, g, o = sig(z[0]), sig(z[1]), math.tanh(z[2]), sig(z[3])
        c = f * c + i * g
        h = o * math.tanh(c)
        out.append((p["w"] * h + p["b"] - ta[t]) ** 2)
        if t == 0 and done0:
            h = c = 0.0
    return out


@pytest.mark.parametrize("done0", [False, True])
def test_reference_against_a_hand_evaluation(done0):
    g = torch.Generator().manual_seed(5)
    r = lambda n: [float(v) for v in torch.randn(n, generator=g).double()]
    p = dict(wi=r(4), wh=r(4), bi=r(4), bh=r(4), w=r(1)[0], b=r(1)[0])
    x, ta, (h0, c0) = r(2), r(2), r(2)
    state = {"memory_s.rnn.weight_ih_l0": torch.tensor(p["wi"]).reshape(4, 1), "memory_s.rnn.weight_hh_l0": torch.tensor(p["wh"]).reshape(4, 1),
             "memory_s.rnn.bias_ih_l0": torch.tensor(p["bi"]), "memory_s.rnn.bias_hh_l0": torch.tensor(p["bh"]),
             "student.0.weight": torch.tensor([[p["w"]]]), "student.0.bias": torch.tensor([p["b"]])}
    state = {k: v.double() for k, v in state.items()}
    m = R.make_model(1, [1, 1], state, torch.float64)
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)
    obs, tav = t64(x).reshape(2, 1, 1), t64(ta).reshape(2, 1, 1)
    dones = torch.tensor([[1 if done0 else 0], [0]], dtype=torch.uint8)
    S = (t64([[h0]]), t64([[c0]]))
    grads, losses, means, (h, c) = R.window_grad(m, obs, tav, dones, S, S, [(0, 2)], "mse")
    want = hand_losses(p, x, ta, h0, c0, done0)
    assert losses == pytest.approx(want, rel=1e-12)
    # the gradient of l_0 + l_1 by central differences of the hand evaluation; with the done, nothing of step 1 reaches step 0
    def total(q):
        return sum(hand_losses(q, x, ta, h0, c0, done0))
    for name, key in (("wh", "memory_s.rnn.weight_hh_l0"), ("wi", "memory_s.rnn.weight_ih_l0"), ("bi", "memory_s.rnn.bias_ih_l0"), ("bh", "memory_s.rnn.bias_hh_l0")):
        for q in range(4):
            eps = 1e-6
            hi, lo = dict(p, **{name: [v + (eps if j == q else 0.0) for j, v in enumerate(p[name])]}), dict(p, **{name: [v - (eps if j == q else 0.0) for j, v in enumerate(p[name])]})
            assert float(grads[key].reshape(-1)[q]) == pytest.approx((total(hi) - total(lo)) / (2 * eps), rel=1e-6, abs=1e-9), (name, q)
    assert torch.equal(grads["memory_s.rnn.bias_ih_l0"], grads["memory_s.rnn.bias_hh_l0"])          # two parameters with equal gradients
    # the whole update over the same two steps with G = 2 takes this gradient: one Adam step of size lr against its sign
    m2 = R.make_model(1, [1, 1], state, torch.float64)
    res = R.update(m2, obs, tav, dones, S, 1, 2, dict(R.HP))
    assert res["loss"] == pytest.approx(sum(want) / 2, rel=1e-12) and len(res["norms"]) == 1
    moved = dict(R.ordered_params(m2))["memory_s.rnn.weight_hh_l0"].detach() - state["memory_s.rnn.weight_hh_l0"]
    assert torch.allclose(moved, -1e-3 * torch.sign(grads["memory_s.rnn.weight_hh_l0"]), rtol=1e-4, atol=0)
    assert torch.equal(res["state"][0], h) and torch.equal(res["state"][1], c)                      # the forward state does not feel the step


def test_dropped_tail_and_window_close_in_the_reference():
    """(T, E, G) = (2, 1, 5): no window closes, the parameters stay, the loss is reported and the state advances"""
    u = RC.get_update_case("T2E1G5")
    assert u["f64"]["norms"] == [] and u["f64"]["loss"] > 0
    assert all(torch.equal(p, u["state"][k].double()) for k, p in u["f64"]["params"].items())
    assert not torch.equal(u["f64"]["state"][0], u["S"][0].double())
    assert not u["f64"]["state"][0][u["dones"][-1] != 0].any() and u["f64"]["state"][0][u["dones"][-1] == 0].any()


# ---- the C ABI's list and the package -----------------------------------------------------------------------------------------------------------------------
EXPECTED = {"go2sim_rdistill_" + n for n in ("act", "create", "destroy", "window_grad", "loss_only", "apply", "update", "n_params", "export", "import", "n_padded",
                                             "export_padded", "set_step", "reset_stats", "stats")}


def test_rdistill_list_is_its_own():
    assert set(capi.DECLARED_RDISTILL_FUNCS) == EXPECTED and len(capi.DECLARED_RDISTILL_FUNCS) == len(EXPECTED)
    assert all(n.startswith("go2sim_rdistill_") for n in capi.DECLARED_RDISTILL_FUNCS)
    others = [capi.DECLARED_FUNCS, capi.DECLARED_TRAIN_FUNCS, capi.DECLARED_RNN_FUNCS, capi.DECLARED_NORM_FUNCS, capi.DECLARED_LIDAR_FUNCS, capi.DECLARED_STAIRINFO_FUNCS,
              capi.DECLARED_DISTILL_FUNCS, capi.DECLARED_ACT_FUNCS]
    for lst in others:
        assert not set(lst) & set(capi.DECLARED_RDISTILL_FUNCS)
        assert not any(n.startswith("go2sim_rdistill_") for n in lst)
    assert len(capi.DECLARED_FUNCS) == 53
    for other in ("go2sim.h", "go2sim_policy.h", "go2sim_train.h", "go2sim_rnn.h", "go2sim_distill.h"):
        assert "go2sim_rdistill_" not in open(os.path.join(capi.REPO_ROOT, "include", other)).read()
    C = capi.C
    assert [C["GO2SIM_RDISTILL_" + n] for n in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V")] == [C["GO2SIM_DISTILL_" + n] for n in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V")]
    assert (C["GO2SIM_RDISTILL_MSE"], C["GO2SIM_RDISTILL_HUBER"]) == (0, 1) and C["GO2SIM_RDISTILL_N_STATS"] == C["GO2SIM_RDISTILL_ST_WINDOWS"] + 1 == 6


def test_hip_library_exports_every_rdistill_function(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in capi.DECLARED_RDISTILL_FUNCS:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_struct_layouts_match_the_header():
    txt = open(capi.RDISTILL_HEADER).read()
    for struct, cls, size in (("go2sim_rdistill_cfg", capi.RDistillCfg, 5 * 8 + 2 * 4), ("go2sim_rdistill_roll", capi.RDistillRoll, 7 * 8 + 2 * 4),
                              ("go2sim_rdistill_seg", capi.RDistillSeg, 2 * 4)):
        body = txt[txt.index("typedef struct %s {" % struct):txt.index("} %s_t;" % struct)]
        pos = [re.search(r"\b" + n + r"\s*[,;]", body).start() for n, _ in cls._fields_]
        assert pos == sorted(pos), struct
        assert ctypes.sizeof(cls) == size, struct


def test_kernels_are_shared_not_copied():
    """the new translation unit includes the shared device headers and defines none of their kernels; the head the two distillation updates run is one kernel"""
    csrc = os.path.join(capi.REPO_ROOT, "go2_sim2real_locomotion_rl_amd", "csrc")
    txt = open(os.path.join(csrc, "go2sim_rdistill.hip")).read()
    for hdr in ("go2sim_lstm_dev.h", "go2sim_train_dev.h", "go2sim_distill_dev.h", "go2sim_trainer_host.h"):
        assert '#include "%s"' % hdr in txt, hdr
    for k in ("k_lstm_cell", "k_lstm_bptt", "k_train_forward", "k_bwd_dw", "k_bwd_db", "k_bwd_da", "k_reduce_partials", "k_sumsq", "k_adam", "k_distill_head",
              "k_distill_accumulate"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\b", txt) is None, k
    assert "k_lstm_cell<true>" in txt and "k_lstm_cell<false>" in txt and "k_lstm_bptt" in txt and "k_distill_head" in txt
    shared = open(os.path.join(csrc, "go2sim_distill_dev.h")).read()
    assert re.search(r"__global__[^;{]*\bk_distill_head\b", shared) and re.search(r"__global__[^;{]*\bk_distill_head\b", open(os.path.join(csrc, "go2sim_distill.hip")).read()) is None
    assert "libgo2sim_cpu" not in txt and "go2sim_cpu_" not in txt                                  # no CPU twin


def test_package_exports():
    import go2_sim2real_locomotion_rl_amd as pkg
    from go2_sim2real_locomotion_rl_amd.distillation import StudentTeacherRecurrent

    assert pkg.StudentTeacherRecurrent is StudentTeacherRecurrent and pkg.rdistill_schedule is rdistill_schedule
    assert {"StudentTeacherRecurrent", "rdistill_schedule", "Distillation", "teacher_state_from_checkpoint"} <= set(pkg.__all__)
    assert StudentTeacherRecurrent.is_recurrent is True
    for bad, match in ((dict(), "StudentTeacherRecurrent.*rnn_hidden_dim"), (dict(rnn_hidden_dim=16, rnn_type="gru"), "gru"),
                       (dict(rnn_hidden_dim=16, rnn_num_layers=2), "rnn_num_layers"), (dict(rnn_hidden_dim=16, rnn_hidden_size=8), "disagree"),
                       (dict(rnn_hidden_dim=16, bogus=1), "bogus")):
        with pytest.raises(Go2SimError, match=match):                        # refused before anything touches a device
            StudentTeacherRecurrent(5, 9, 4, [8], [8], **bad)


# ---- the margins of the case table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.WINDOW_CASES))
def test_window_case_margins(name):
    c = RC.get_window_case(name)                                             # the Huber bands are asserted while the case is built
    d = c.ref["f64"][2] - torch.stack([c.ta[t] for t0, n in c.segs for t in range(t0, t0 + n)]).double()
    assert bool(((d.abs() - 1.0).abs() > 0.15).all())                        # on the window's own means too (a carried state is float32-rounded)
    if c.spec["cut"] is None:
        return
    diff, bound = c.cut_margin()
    print(f"MARGIN {name} cut {c.spec['cut']}: {diff:.3e} against a bound of {bound:.3e} = {diff / bound:.0f} x")
    assert diff >= 100 * bound
    forced = [(t, e % c.N) for t, e in c.spec["forced"]]
    assert all(int(c.dones[t, e]) == 1 for t, e in forced)
    if c.spec["cut"] == "done":                                              # a done in the middle of the window and one on its last step
        last = c.segs[-1][0] + c.segs[-1][1] - 1
        assert c.dones[last].any() and c.dones[:last].any() and not c.dones.all()


@pytest.mark.parametrize("name", sorted(RC.UPDATE_CASES))
def test_update_case_margins(name):
    u = RC.get_update_case(name)                                             # the clip margins and the distance from Huber's branch are asserted while it is built
    T, E, G = u["T"], u["E"], u["G"]
    assert len(u["f64"]["norms"]) == (E * T) // G
    assert u["dones"][T - 1].any() and u["dones"][(G - 1) % T].any() and not u["dones"].all()
    if u["hp"]["max_grad_norm"] is not None:
        assert u["hp"]["max_grad_norm"] > 0
