"""module_core.py without a GPU: the constructors' initial draws against a restatement of the draw order (and against the digests recorded from the
build before the modules shared a core, tests/golden/module_trace.json), and MemoryState -- one memory's [h, c, spare h] -- under an eager and a
deferred user against two plain arrays."""
import importlib.util
import json
import os

import pytest
import torch

from go2_sim2real_locomotion_rl_amd import module_core as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_recorder():
    spec = importlib.util.spec_from_file_location("record_module_trace", os.path.join(ROOT, "tools", "record_module_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = load_recorder()
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "module_trace.json")))
N_OBS, N_PRIV, N_ACT, HIDDEN, H, HT = REC.N_OBS, REC.N_PRIV, REC.N_ACT, REC.HIDDEN, REC.H, REC.HT
assert (N_OBS, N_PRIV, N_ACT, HIDDEN, H, HT) == (5, 7, 3, [6, 4], 4, 5)

# pairing -> ([(prefix, layer sizes)], [(prefix, (n_in, H))], init_noise_std of the class's default): what the recorder's constructors are given
SIZES = {
    "ActorCritic": ([("actor", [N_OBS, *HIDDEN, N_ACT]), ("critic", [N_PRIV, *HIDDEN, 1])], [], 1.0),
    "ActorCriticRecurrent": ([("actor", [H, *HIDDEN, N_ACT]), ("critic", [H, *HIDDEN, 1])], [("memory_a", (N_OBS, H)), ("memory_c", (N_PRIV, H))], 1.0),
    "StudentTeacher": ([("student", [N_OBS, *HIDDEN, N_ACT]), ("teacher", [N_PRIV, *HIDDEN, N_ACT])], [], 0.1),
    "StudentTeacherRecurrent": ([("student", [H, *HIDDEN, N_ACT]), ("teacher", [N_PRIV, *HIDDEN, N_ACT])], [("memory_s", (N_OBS, H))], 0.1),
    "StudentTeacherRecurrent+teacher": ([("student", [H, *HIDDEN, N_ACT]), ("teacher", [HT, *HIDDEN, N_ACT])], [("memory_s", (N_OBS, H)), ("memory_t", (N_PRIV, HT))], 0.1),
}


def pure_initial_state(pairing, seed):
    """the module class's pure initial-state function at the recorder's sizes"""
    nets, mems, noise = SIZES[pairing]
    (_, d0), (_, d1) = nets
    if pairing == "ActorCritic":
        return mc.actor_critic_init(d0, d1, noise, seed)
    if pairing == "ActorCriticRecurrent":
        return mc.actor_critic_recurrent_init(d0, d1, (mems[0][1], mems[1][1]), noise, seed)
    if pairing == "StudentTeacher":
        return mc.student_teacher_init(d0, d1, noise, seed)
    return mc.student_teacher_recurrent_init(d0, d1, mems[0][1], mems[1][1] if len(mems) > 1 else None, noise, seed)


def restated_initial_state(pairing, seed):
    """The draw order written out: one generator seeded `seed` for the linears, prefix by prefix, layer by layer, weight before bias; one seeded
    `seed + 0x5eed` for the memories, prefix by prefix, weight_ih, weight_hh, bias_ih, bias_hh."""
    nets, mems, noise = SIZES[pairing]
    sd = {}
    g = torch.Generator().manual_seed(seed)
    for prefix, dims in nets:
        for l in range(len(dims) - 1):
            n_in, n_out = dims[l], dims[l + 1]
            sd[f"{prefix}.{2 * l}.weight"] = (torch.rand(n_out, n_in, generator=g) * 2 - 1) * (1.0 / n_in ** 0.5)
            sd[f"{prefix}.{2 * l}.bias"] = (torch.rand(n_out, generator=g) * 2 - 1) * (1.0 / n_in ** 0.5)
    g = torch.Generator().manual_seed(seed + 0x5eed)
    for prefix, (n_in, h) in mems:
        sd[f"{prefix}.rnn.weight_ih_l0"] = (torch.rand(4 * h, n_in, generator=g) * 2 - 1) / h ** 0.5
        sd[f"{prefix}.rnn.weight_hh_l0"] = (torch.rand(4 * h, h, generator=g) * 2 - 1) / h ** 0.5
        sd[f"{prefix}.rnn.bias_ih_l0"] = (torch.rand(4 * h, generator=g) * 2 - 1) / h ** 0.5
        sd[f"{prefix}.rnn.bias_hh_l0"] = (torch.rand(4 * h, generator=g) * 2 - 1) / h ** 0.5
    sd["std"] = noise * torch.ones(N_ACT)
    return sd


@pytest.mark.parametrize("seed", REC.SEEDS)
@pytest.mark.parametrize("pairing", REC.PAIRINGS)
def test_initial_state_is_the_restated_draw_order_and_the_parents(pairing, seed):
    got, want = pure_initial_state(pairing, seed), restated_initial_state(pairing, seed)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert REC.state_digest(want) == GOLDEN[f"{pairing}/seed{seed}/B3"]["init"], "the restatement is not what the parent's constructor drew"
    assert REC.state_digest(got) == GOLDEN[f"{pairing}/seed{seed}/B3"]["init"]


@pytest.mark.parametrize("seed", REC.SEEDS)
@pytest.mark.parametrize("pairing", REC.PAIRINGS)
def test_initial_state_is_within_the_torch_default_bounds(pairing, seed):
    """nn.Linear: uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weight and bias; nn.LSTM: uniform(-1 / sqrt(H), 1 / sqrt(H)) for all four.  The draw is
    u * b or u / s with |u| <= 1 in float32, and float32 rounding is monotone: no entry exceeds the float32 value of the bound itself."""
    nets, mems, noise = SIZES[pairing]
    sd = pure_initial_state(pairing, seed)
    seen = {"std"}
    for prefix, dims in nets:
        for l in range(len(dims) - 1):
            bound = torch.tensor(1.0 / dims[l] ** 0.5, dtype=torch.float32)
            for k in (f"{prefix}.{2 * l}.weight", f"{prefix}.{2 * l}.bias"):
                assert sd[k].abs().max() <= bound, k
                seen.add(k)
    for prefix, (n_in, h) in mems:
        bound = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(h ** 0.5, dtype=torch.float32)
        for k, shape in mc.memory_keys(prefix, n_in, h):
            assert tuple(sd[k].shape) == shape and sd[k].abs().max() <= bound, k
            seen.add(k)
    assert seen == set(sd)
    assert torch.equal(sd["std"], noise * torch.ones(N_ACT))


def test_initial_state_functions_take_any_std_and_follow_the_seed():
    a, b = mc.student_teacher_init([5, 4, 3], [7, 4, 3], 0.25, 1), mc.student_teacher_init([5, 4, 3], [7, 4, 3], 0.25, 2)
    assert torch.equal(a["std"], torch.full((3,), 0.25)) and not torch.equal(a["student.0.weight"], b["student.0.weight"])
    g = torch.Generator().manual_seed(3)
    assert list(mc.linear_init(g, "n", [2, 3, 1])) == ["n.0.weight", "n.0.bias", "n.2.weight", "n.2.bias"]
    assert list(mc.lstm_init(g, "m", 2, 3)) == [k for k, _ in mc.memory_keys("m", 2, 3)] == ["m.rnn." + k for k in mc.LSTM_KEYS]


# ---- MemoryState ------------------------------------------------------------------------------------------------------------------------------------------
STEPS = 8


def toy_cell(x, h_in, c_in, h_out, c_out, reset):
    """what the cell launch does with its arguments: the rows of `reset` enter with h = c = 0; h' = tanh(x + h) into h_out, c' = c + x in place"""
    assert h_out is not h_in and h_out.data_ptr() != h_in.data_ptr(), "h_out must not be h_in"
    assert c_out is c_in, "c is stepped in place"
    if reset is not None:
        h_in = h_in.masked_fill(reset.reshape(-1, 1) != 0, 0.0)
        c_in.masked_fill_(reset.reshape(-1, 1) != 0, 0.0)
    h_out.copy_(torch.tanh(x + h_in))
    c_out.add_(x)


def patterns(B):
    """name -> ({step: [masks of the reset calls after that step]}, steps after whose resets a reader that is not the cell step looks)"""
    row0, last, ones, zeros = torch.zeros(B), torch.zeros(B), torch.ones(B), torch.zeros(B)
    row0[0], last[B - 1] = 1.0, 1.0
    return {"done_at_the_first_step": ({0: [row0]}, ()),
            "done_at_every_step": ({k: [ones] for k in range(STEPS)}, ()),
            "never_done": ({k: [zeros] for k in range(STEPS)}, ()),
            "two_resets_without_a_step": ({2: [row0, last], 5: [ones, zeros]}, ()),
            "reset_then_a_reader": ({1: [last], 3: [row0], 6: [ones]}, (3, 6))}


def run_user(kind, B, resets, readers, xs):
    """-> (h, c after every step, copies of the entering state before every step, the views at the readers)"""
    state = mc.MemoryState(4, torch.device("cpu"))
    assert state.B == 0 and state.pending is None
    after, entering, views = [], [], []
    for k in range(STEPS):
        copy = (torch.full((B, 4), 9.0), torch.full((B, 4), 9.0))
        state.rows(B).copy_entering(*copy)
        entering.append(copy)
        reset = state.take_pending() if kind == "deferred" else None
        assert state.pending is None
        toy_cell(xs[k], *state.advance(), reset)
        after.append((state.h.clone(), state.c.clone()))
        for mask in resets.get(k, ()):
            if kind == "deferred":
                state.defer(mask.to(torch.uint8))
            else:
                state.zero(mask)
        if k in readers:
            copy = (torch.empty(B, 4), torch.empty(B, 4))
            state.copy_entering(*copy)                                   # does not write the live state; the views then apply what is pending
            h, c = state.views()
            assert h.shape == (1, B, 4) and h.data_ptr() == state.h.data_ptr() and c.data_ptr() == state.c.data_ptr() and state.pending is None
            views.append((copy[0], copy[1], h.clone(), c.clone()))
    return after, entering, views


def run_plain(B, resets, readers, xs):
    """the same in two arrays, rows zeroed by hand"""
    h, c = torch.zeros(B, 4), torch.zeros(B, 4)
    after, entering, views = [], [], []
    for k in range(STEPS):
        entering.append((h.clone(), c.clone()))
        h, c = torch.tanh(xs[k] + h), c + xs[k]
        after.append((h.clone(), c.clone()))
        for mask in resets.get(k, ()):
            for b in range(B):
                if mask[b] != 0:
                    h[b], c[b] = 0.0, 0.0
        if k in readers:
            views.append((h.clone(), c.clone(), h.clone().unsqueeze(0), c.clone().unsqueeze(0)))
    return after, entering, views


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("name", sorted(patterns(1)))
def test_memory_state_eager_and_deferred_are_the_plain_arrays(name, B):
    resets, readers = patterns(B)[name]
    xs = torch.randn(STEPS, B, 4, generator=torch.Generator().manual_seed(11))
    eager, deferred, plain = run_user("eager", B, resets, readers, xs), run_user("deferred", B, resets, readers, xs), run_plain(B, resets, readers, xs)
    for what, e, d, p in zip(("after a step", "entering a step", "at a reader"), eager, deferred, plain):
        assert len(e) == len(d) == len(p)
        for k, (te, td, tp) in enumerate(zip(e, d, p)):
            for a, b, c in zip(te, td, tp):
                assert torch.equal(a, b) and torch.equal(a, c), f"{what}, {k}"
    assert len(plain[2]) == len(readers)
    assert any(bool((t[0] == 0).all(dim=1).any()) for t in plain[1][1:]) == (name != "never_done"), "the pattern zeroes a row that was not zero"


def test_memory_state_another_row_count_allocates_afresh():
    state = mc.MemoryState(4, torch.device("cpu")).rows(3)
    toy_cell(torch.ones(3, 4), *state.advance(), None)
    state.defer(torch.ones(3, dtype=torch.uint8))
    old = state.h
    assert bool(state.h.any()) and state.pending is not None and state.rows(3).h is old
    state.rows(1)
    assert state.B == 1 and state.h.shape == (1, 4) and state.c.shape == (1, 4) and not state.h.any() and not state.c.any() and state.pending is None
    state.replace(torch.ones(1, 2, 4), 2 * torch.ones(1, 2, 4))             # the shapes of views(): [1][B][H]
    assert state.B == 2 and torch.equal(state.h, torch.ones(2, 4)) and torch.equal(state.c, 2 * torch.ones(2, 4)) and state.pending is None
    state.defer(torch.tensor([1, 0], dtype=torch.uint8))
    state.zero()                                                             # everything, now: the pending mask goes with it
    assert not state.h.any() and not state.c.any() and state.pending is None
    assert mc.hidden_state_views((mc.MemoryState(4, torch.device("cpu")), None)) == (None, None)
    h, none = mc.hidden_state_views((state, None))
    assert none is None and h[0].shape == (1, 2, 4)
