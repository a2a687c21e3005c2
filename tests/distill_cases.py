"""The case table of the distillation tests (tests/test_distill_gpu.py): student networks, shapes and inputs.  The student nets are the actor shapes of
tests/ppo_cases.py.  The inputs have margins, so that no entry is ever excluded from a comparison:
  * the residuals student(obs) - teacher_actions come from [0, 0.8] u [1.25, 3] with both signs in both bands (Huber's branch at |d| = 1); they are set
    through teacher_actions from the float64 student forward and are float32-exact (every side reads the same float32 teacher_actions);
  * the clip cases have ||g|| of every window at least 20 % away from max_grad_norm, one case on each side.
The margins are held with asserts here, on the CPU.  A case's float64 and float32 evaluations are computed once and shared by the tests that need them."""
import functools
import math

import torch

import distill_ref as R
import ppo_cases as PC

ROW_CHUNK = PC.ROW_CHUNK
NETS = {name: dims[0] for name, dims in PC.NETS.items()}                  # the actor shapes
TEACHER = {"one_layer": [7, 4], "small": [104, 24, 16], "six_layers": [5, 9, 4], "full": [100, 64, 12]}
LOSSES = ("mse", "huber")
ENVS = (1, 15, 16, 17, 37)
# (net, N envs, G pairs in the window, loss type, kind); kind "plain": the window is steps G-1 .. 0 of a storage of G + 1 steps (the last is never read),
# "dup": T = 2, the window (0,0), (0,1), (1,0) holds step 0 twice
GRAD_CASES = [(net, n, (1, 3)[(i + j) % 2], LOSSES[(i + (j + 1) // 2) % 2], "plain") for i, net in enumerate(("one_layer", "small", "six_layers")) for j, n in enumerate(ENVS)]
GRAD_CASES += [("small", 37, 3, "mse", "plain"), ("small", 16, 1, "mse", "plain"),
               ("full", 16, 5, "huber", "plain"),                           # the full widths at 80 rows only
               ("small", 2 * ROW_CHUNK + 37, 1, "mse", "plain"),            # one window across chunk boundaries
               ("small", 17, 3, "mse", "dup"), ("six_layers", 37, 3, "huber", "dup")]
assert len(set(GRAD_CASES)) == len(GRAD_CASES)
for _net in ("one_layer", "small", "six_layers"):                        # every net sees both window lengths and both losses
    assert {c[2] for c in GRAD_CASES if c[0] == _net} == {1, 3} and {c[3] for c in GRAD_CASES if c[0] == _net} == set(LOSSES)


def case_id(c):
    return "-".join(str(x) for x in c)


def init_state(sdims, tdims, gen, std=0.1):
    """nn.Linear's default init (uniform +- 1 / sqrt(fan_in)) for both networks, std = init_noise_std; float32"""
    sd = {}
    for prefix, dims in (("student", sdims), ("teacher", tdims)):
        for l in range(len(dims) - 1):
            bound = 1.0 / math.sqrt(dims[l])
            sd[f"{prefix}.{2 * l}.weight"] = ((torch.rand(dims[l + 1], dims[l], generator=gen) * 2 - 1) * bound).float()
            sd[f"{prefix}.{2 * l}.bias"] = ((torch.rand(dims[l + 1], generator=gen) * 2 - 1) * bound).float()
    sd["std"] = torch.full((sdims[-1],), std).float()
    return sd


BANDS = ((0.0, 0.8), (1.25, 3.0))


def make_storage(sdims, tdims, state, T, N, seed):
    """obs [T][N][Ds] and teacher_actions [T][N][A] (float32) with the residual margins above under `state`"""
    g = torch.Generator().manual_seed(seed)
    A = sdims[-1]
    m64 = R.make_model(sdims, tdims, state, torch.float64)
    obs = torch.randn(T, N, sdims[0], generator=g).float()
    with torch.no_grad():
        mu = m64.student(obs.double())
    u = torch.rand(T, N, A, generator=g).double()
    k = torch.arange(T * N * A).reshape(T, N, A)
    band = k % 2                                                           # the band alternates entry by entry, the sign every two entries
    lo = torch.where(band == 0, BANDS[0][0], BANDS[1][0])
    hi = torch.where(band == 0, BANDS[0][1], BANDS[1][1])
    d = (lo + (hi - lo) * u) * torch.where((k // 2) % 2 == 0, 1.0, -1.0)
    ta = (mu - d).float()
    check_margins(m64, obs, ta)
    return obs, ta


def check_margins(m64, obs, ta):
    """The construction's promise, on the float32-rounded teacher_actions: no residual within 0.19 of Huber's branch, both signs in both bands (given enough entries)."""
    with torch.no_grad():
        d = m64.student(obs.double()) - ta.double()
    assert bool(((d.abs() - 1.0).abs() > 0.19).all()), float((d.abs() - 1.0).abs().min())
    assert float(d.abs().max()) < 3.01
    if d.numel() >= 4:
        for inner in (True, False):
            sel = d[(d.abs() < 1.0) == inner]
            assert bool((sel > 0).any()) and bool((sel < 0).any())


class Case:
    """One window: the state, the storage, the window's steps and the float64 / float32 evaluations of the law."""

    def __init__(self, net, N, G, loss_type, kind, seed):
        self.net, self.N, self.G, self.loss_type, self.kind = net, N, G, loss_type, kind
        self.sdims, self.tdims = NETS[net], TEACHER[net]
        g = torch.Generator().manual_seed(seed)
        self.state = init_state(self.sdims, self.tdims, g)
        if kind == "dup":
            assert G == 3
            self.T, self.steps = 2, [0, 1, 0]
        else:
            self.T, self.steps = G + 1, list(range(G - 1, -1, -1))
        self.obs, self.ta = make_storage(self.sdims, self.tdims, self.state, self.T, N, seed + 1)
        if kind != "dup":                                                  # the storage's last step belongs to no window: nothing may read it
            self.obs[-1] = float("nan"); self.ta[-1] = float("nan")
        self.idx = torch.cat([t * N + torch.arange(N) for t in self.steps]).to(torch.int32)
        self.ref = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = R.make_model(self.sdims, self.tdims, self.state, dt)
            grads, losses = R.window_grad(m, self.obs.to(dt), self.ta.to(dt), self.steps, loss_type)
            with torch.no_grad():
                mu = m.student(self.obs.to(dt)[self.steps].reshape(-1, self.sdims[0]))
            self.ref[name] = (grads, losses, mu)


@functools.lru_cache(maxsize=None)
def get_case(net, N, G, loss_type, kind):
    c = (net, N, G, loss_type, kind)
    return Case(*c, seed=3000 + 17 * GRAD_CASES.index(c) if c in GRAD_CASES else 99)


# ---- whole updates on the small student: (T, E, G) -------------------------------------------------------------------------------------------------
SCHEDULES = [(3, 1, 3), (4, 1, 3), (3, 2, 4), (2, 2, 3), (2, 1, 5)]
UPDATE_ENVS = (17, 37)
# the clip of a case is "none", "below" or "above"; max_grad_norm: not given / half the smallest window norm (every window clipped) / twice the largest (none is)
UPDATE_CASES = [(s, n, "none") for s in SCHEDULES for n in UPDATE_ENVS] + [((3, 2, 4), 17, "below"), ((3, 2, 4), 37, "above"), ((4, 1, 3), 37, "below")]


def update_id(c):
    return "T%dE%dG%d-N%d-%s" % (*c[0], c[1], c[2])


@functools.lru_cache(maxsize=None)
def get_update_case(sched, N, clip):
    T, E, G = sched
    sdims, tdims = NETS["small"], TEACHER["small"]
    g = torch.Generator().manual_seed(5000 + 100 * SCHEDULES.index(sched) + N)
    state = init_state(sdims, tdims, g)
    obs, ta = make_storage(sdims, tdims, state, T, N, 5001 + 100 * SCHEDULES.index(sched) + N)
    hp = dict(R.HP)
    if clip != "none":
        _, norms = R.update(R.make_model(sdims, tdims, state, torch.float64), obs.double(), ta.double(), E, G, hp)
        hp["max_grad_norm"] = 0.5 * min(norms) if clip == "below" else 2.0 * max(norms)
    out = dict(sdims=sdims, tdims=tdims, state=state, obs=obs, ta=ta, T=T, E=E, G=G, N=N, hp=hp)
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = R.make_model(sdims, tdims, state, dt)
        loss, norms = R.update(m, obs.to(dt), ta.to(dt), E, G, hp)
        out[prec] = dict(params={k: p.detach().clone() for k, p in R.ordered_params(m)}, loss=loss, norms=norms)
    mgn = hp["max_grad_norm"]
    if clip == "below":                                                    # the margin of the clip decision, on the run that was clipped
        assert all(n >= 1.2 * mgn for n in out["f64"]["norms"]), (out["f64"]["norms"], mgn)
    elif clip == "above":
        assert all(n <= 0.8 * mgn for n in out["f64"]["norms"]), (out["f64"]["norms"], mgn)
    return out
