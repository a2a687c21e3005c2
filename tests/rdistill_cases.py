"""The case table of the recurrent distillation tests (tests/test_rdistill_gpu.py): memories, students, shapes, dones and inputs.  The inputs have margins, so
that no entry is ever excluded from a comparison and no decision hangs on rounding:
  * the residuals mean - teacher_actions come from the bands of distill_cases (BANDS: [0, 0.8] u [1.25, 3], both signs in both bands; Huber's branch at 1);
    they are set through teacher_actions from the float64 forward under the initial parameters, and a whole update's float64 run reports how close any
    residual of any epoch came to the branch;
  * the clip cases have ||g|| of every window at least 20 % away from max_grad_norm, one case on each side;
  * every case built to exercise a cut has a float64 gradient of memory_s.weight_hh that differs, with the cut and without it, by at least 100 times
    the bound the GPU test applies: a kernel that ignores the cut cannot pass.
The margins are held with asserts (tests/test_rdistill_ref.py runs them on the CPU).  A case's float64 and float32 evaluations are computed once."""
import functools
import math

import torch

import distill_cases as DC
import rdistill_ref as R

C_GRAD = 16
EPS = 2.0 ** -24
ROW_CHUNK = DC.ROW_CHUNK
A = 12


def init_state(n_in, sdims, gen):
    """nn.Linear's and nn.LSTM's default inits; float32"""
    sd = {}
    for l in range(len(sdims) - 1):
        bound = 1.0 / math.sqrt(sdims[l])
        sd[f"student.{2 * l}.weight"] = ((torch.rand(sdims[l + 1], sdims[l], generator=gen) * 2 - 1) * bound).float()
        sd[f"student.{2 * l}.bias"] = ((torch.rand(sdims[l + 1], generator=gen) * 2 - 1) * bound).float()
    H = sdims[0]
    for k, shape in (("weight_ih_l0", (4 * H, n_in)), ("weight_hh_l0", (4 * H, H)), ("bias_ih_l0", (4 * H,)), ("bias_hh_l0", (4 * H,))):
        sd[f"memory_s.rnn.{k}"] = ((torch.rand(*shape, generator=gen) * 2 - 1) / math.sqrt(H)).float()
    return sd


def make_dones(T, N, forced, gen):
    """uint8 [T][N]: one env in four done at random, plus the forced (t, env) entries"""
    d = (torch.rand(T, N, generator=gen) < 0.25).to(torch.uint8)
    for t, e in forced:
        d[t, e % N] = 1
    return d


def residuals(shape, gen):
    """distill_cases.make_storage's construction: the band alternates entry by entry, the sign every two entries"""
    n = 1
    for s in shape:
        n *= s
    u = torch.rand(*shape, generator=gen).double()
    k = torch.arange(n).reshape(shape)
    lo = torch.where(k % 2 == 0, DC.BANDS[0][0], DC.BANDS[1][0])
    hi = torch.where(k % 2 == 0, DC.BANDS[0][1], DC.BANDS[1][1])
    return (lo + (hi - lo) * u) * torch.where((k // 2) % 2 == 0, 1.0, -1.0)


def check_bands(d):
    """the promise of distill_cases.check_margins on a tensor of residuals"""
    assert bool(((d.abs() - 1.0).abs() > 0.19).all()), float((d.abs() - 1.0).abs().min())
    assert float(d.abs().max()) < 3.01
    if d.numel() >= 4:
        for inner in (True, False):
            sel = d[(d.abs() < 1.0) == inner]
            assert bool((sel > 0).any()) and bool((sel < 0).any())


def rollout_means(m64, obs, dones, S):
    """the float64 means of one pass through the rollout from S -> [T][N][A], and the state entering every step"""
    h, c = S
    mus, states = [], []
    with torch.no_grad():
        for t in range(obs.shape[0]):
            states.append((h, c))
            h, c = R.cell(m64, obs[t], h, c)
            mus.append(m64.student(h))
            h, c = R.masked(h, dones[t]), R.masked(c, dones[t])
    return torch.stack(mus), states


def make_storage(n_in, sdims, state, T, N, dones, gen):
    """obs [T][N][I], teacher_actions [T][N][A] (float32) with the residual margins under `state`, and S, a non-zero state [N][H] x 2"""
    m64 = R.make_model(n_in, sdims, state, torch.float64)
    obs = torch.randn(T, N, n_in, generator=gen).float()
    S = tuple((0.5 * torch.randn(N, sdims[0], generator=gen)).float() for _ in range(2))
    mu, _ = rollout_means(m64, obs.double(), dones, tuple(s.double() for s in S))
    ta = (mu - residuals(mu.shape, gen)).float()
    check_bands(mu - ta.double())
    return obs, ta, S


# ---- one window ----------------------------------------------------------------------------------------------------------------------------------------
# name: I, H, N, T, segments (t0, n), forced dones (t, env), loss, cut exercised (None, "done", "epoch", "first"), sub_envs of the handle (0: the default)
WINDOW_CASES = {
    "plain":     dict(I=5, H=16, N=17, T=3, segs=[(0, 3)], forced=[], loss="mse", cut=None, sub=0, no_dones=True),
    "one_row":   dict(I=49, H=20, N=1, T=1, segs=[(0, 1)], forced=[], loss="huber", cut=None, sub=0, no_dones=True),
    # a done in the middle of the window, one on its last step (which is T - 1 too)
    "done_cut":  dict(I=5, H=20, N=37, T=4, segs=[(0, 4)], forced=[(1, 3), (1, 20), (3, 5), (3, 36)], loss="huber", cut="done", sub=0),
    # the window of (T, E, G) = (3, 2, 4): across the epoch boundary, a done on T - 1
    "epoch_cut": dict(I=49, H=48, N=17, T=3, segs=[(0, 3), (0, 1)], forced=[(2, 4), (0, 9)], loss="mse", cut="epoch", sub=0),
    # a window that opens inside an epoch: its first pair continues the carried state, some envs enter it done
    "first_cut": dict(I=5, H=48, N=37, T=4, segs=[(1, 3)], forced=[(0, 2), (2, 30)], loss="mse", cut="first", sub=0),
    # 2 x 512 + 37 rows in one block: the window's rows run across chunk boundaries
    "chunks":    dict(I=5, H=16, N=2 * ROW_CHUNK + 37, T=1, segs=[(0, 1)], forced=[(0, 600)], loss="mse", cut=None, sub=2048),
    # the training widths once, at 16 envs
    "full":      dict(I=49, H=256, N=16, T=3, segs=[(0, 3)], forced=[(1, 7)], loss="mse", cut="done", sub=0, hidden=[32]),
}


def sdims_of(spec):
    return [spec["H"], *spec.get("hidden", [24]), A]


class WindowCase:
    def __init__(self, name):
        spec = WINDOW_CASES[name]
        self.name, self.spec = name, spec
        self.I, self.N, self.T, self.segs, self.loss_type, self.sub = spec["I"], spec["N"], spec["T"], list(spec["segs"]), spec["loss"], spec["sub"]
        self.sdims = sdims_of(spec)
        g = torch.Generator().manual_seed(7000 + 31 * sorted(WINDOW_CASES).index(name))
        self.state = init_state(self.I, self.sdims, g)
        self.dones = torch.zeros(self.T, self.N, dtype=torch.uint8) if spec.get("no_dones") else make_dones(self.T, self.N, spec["forced"], g)
        self.obs, self.ta, self.S = make_storage(self.I, self.sdims, self.state, self.T, self.N, self.dones, g)
        self.P = sum(n for _, n in self.segs)
        m64 = R.make_model(self.I, self.sdims, self.state, torch.float64)
        _, states = rollout_means(m64, self.obs.double(), self.dones, tuple(s.double() for s in self.S))
        t0 = self.segs[0][0]
        # the carried state a window that opens at t0 > 0 continues: h', c' of step t0 - 1, unmasked (the float32 rounding of the float64 run, so that every
        # side reads the same values); poisoned when nothing may read it
        if t0 > 0:
            with torch.no_grad():
                hc = R.cell(m64, self.obs[t0 - 1].double(), *states[t0 - 1])
            self.carried = tuple(x.float() for x in hc)
        else:
            self.carried = tuple(torch.full((self.N, self.sdims[0]), float("nan")) for _ in range(2))
        self.ref = {}
        for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = R.make_model(self.I, self.sdims, self.state, dt)
            self.ref[prec] = R.window_grad(m, self.obs.to(dt), self.ta.to(dt), self.dones, tuple(s.to(dt) for s in self.S), tuple(s.to(dt) for s in self.carried),
                                           self.segs, self.loss_type)

    def bound(self, key):
        """what the GPU test allows on gradient tensor `key`"""
        g64, g32 = self.ref["f64"][0][key], self.ref["f32"][0][key]
        return C_GRAD * max(float((g32.double() - g64).abs().max()), EPS * float(g64.abs().max()))

    def cut_margin(self):
        """-> (difference of the float64 weight_hh gradient with and without the case's cut, the GPU test's bound on that tensor)"""
        key = "memory_s.rnn.weight_hh_l0"
        m = R.make_model(self.I, self.sdims, self.state, torch.float64)
        S = tuple(s.double() for s in self.S)
        g_uncut = R.window_grad(m, self.obs.double(), self.ta.double(), self.dones, S, tuple(s.double() for s in self.carried), self.segs, self.loss_type,
                                uncut=self.spec["cut"])[0][key]
        return float((g_uncut - self.ref["f64"][0][key]).abs().max()), self.bound(key)


@functools.lru_cache(maxsize=None)
def get_window_case(name):
    return WindowCase(name)


# ---- whole updates -----------------------------------------------------------------------------------------------------------------------------------------
# name: I, H, N, (T, E, G), clip ("none", "below", "above"), loss, sub_envs
UPDATE_CASES = {
    "T3E2G4":        dict(I=5, H=16, N=17, sched=(3, 2, 4), clip="none", loss="mse", sub=0),       # one window across the epoch boundary, a tail of two pairs
    "T4E1G3-below":  dict(I=49, H=20, N=37, sched=(4, 1, 3), clip="below", loss="huber", sub=0),   # a tail of one pair
    "T2E2G3-above":  dict(I=5, H=48, N=17, sched=(2, 2, 3), clip="above", loss="mse", sub=0),
    "T2E1G5":        dict(I=5, H=20, N=37, sched=(2, 1, 5), clip="none", loss="mse", sub=0),       # no window closes: everything is tail
    "T3E1G1-one":    dict(I=49, H=16, N=1, sched=(3, 1, 1), clip="none", loss="huber", sub=0),     # every pair a window, one env
    "T4E2G4-blocks": dict(I=5, H=20, N=37, sched=(4, 2, 4), clip="none", loss="mse", sub=16),      # three env blocks, two windows, no tail
}


@functools.lru_cache(maxsize=None)
def get_update_case(name):
    spec = UPDATE_CASES[name]
    T, E, G = spec["sched"]
    I, N = spec["I"], spec["N"]
    sdims = sdims_of(spec)
    g = torch.Generator().manual_seed(9000 + 13 * sorted(UPDATE_CASES).index(name))
    state = init_state(I, sdims, g)
    # a done on T - 1 and one on the first window's last step
    dones = make_dones(T, N, [(T - 1, 0), ((G - 1) % T, 1), (0, 2)], g)
    obs, ta, S = make_storage(I, sdims, state, T, N, dones, g)
    hp = dict(R.HP, loss_type=spec["loss"])
    if spec["clip"] != "none":
        norms = R.update(R.make_model(I, sdims, state, torch.float64), obs.double(), ta.double(), dones, tuple(s.double() for s in S), E, G, hp)["norms"]
        hp["max_grad_norm"] = 0.5 * min(norms) if spec["clip"] == "below" else 2.0 * max(norms)
    out = dict(name=name, I=I, N=N, T=T, E=E, G=G, sdims=sdims, state=state, obs=obs, ta=ta, dones=dones, S=S, hp=hp, sub=spec["sub"])
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = R.make_model(I, sdims, state, dt)
        res = R.update(m, obs.to(dt), ta.to(dt), dones, tuple(s.to(dt) for s in S), E, G, hp)
        out[prec] = dict(res, params={k: p.detach().clone() for k, p in R.ordered_params(m)})
    assert out["f64"]["margin"] > 0.1, out["f64"]["margin"]              # no residual of any epoch near Huber's branch
    mgn = hp["max_grad_norm"]
    if spec["clip"] == "below":
        assert all(n >= 1.2 * mgn for n in out["f64"]["norms"]), (out["f64"]["norms"], mgn)
    elif spec["clip"] == "above":
        assert all(n <= 0.8 * mgn for n in out["f64"]["norms"]), (out["f64"]["norms"], mgn)
    return out
