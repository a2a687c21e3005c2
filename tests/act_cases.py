"""The case builders of the activation tests (tests/test_act_gpu.py; tests/test_act_cases.py builds every case on the CPU).  Every condition below is
asserted on the float64 reference alone, before the library is run:

  * forward cases with fewer than 8 outputs (a critic at one row): the yardstick's few samples are no outliers (`yardstick_is_no_outlier`);
  * forward cases: every hidden layer's float64 pre-activations have at least a fifth on each side of 0 (names with a branch at 0), or at least a tenth
    with |v| < 0.5 and a tenth with |v| > 3 (tanh, sigmoid: the linear and the saturated regime);
  * update cases of relu, lrelu and selu, whose derivative jumps at 0: NO hidden float64 pre-activation, in any forward pass of the float64 reference,
    lies within 64 x 2^-24 x (that layer's sum_k |x_k w_k| + |b|) of 0.  A pre-activation that rounds to the other side of 0 in float32 is a legitimate
    O(1) difference of the gradient, not a kernel error; the condition excludes it.  It is watched with forward hooks on the reference model's hidden
    Linear layers, so it covers every mini-batch of a whole update as well.

A builder walks seeds upward from a fixed start until its condition holds and records the seed it used (`.seed`; tests/test_act_cases.py prints them).
The first seed passes for every case of the tables below but one: the relu update on the wider pair (21 760 hidden pre-activations in each of its three
forward passes) takes the third.

The float64 references are the torch models of tests/ppo_ref.py, tests/ppo_rnn_ref.py and tests/distill_ref.py with their nn.ELU modules swapped for
the module of the name (`swapped`): those files stay as they are.  The per-row PPO inputs and the distillation residuals are built by the existing
builders (tests/ppo_cases.py, tests/ppo_rnn_cases.py, tests/distill_cases.py) from the swapped float64 forward, with their margins."""
import contextlib
import functools
import math

import numpy as np
import torch
from torch import nn

import act_ref as AR
import distill_cases as DC
import distill_ref as DR
import ppo_cases as PC
import ppo_ref as R
import ppo_rnn_cases as RC
import ppo_rnn_ref as RR

TORCH_ACT = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "identity": nn.Identity}
NEW_NAMES = tuple(n for n in AR.NAMES if n != "elu")
U24 = AR.U24


# ---- the swap ------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def swapped(name):
    """Inside: the `mlp` builders of ppo_ref (which ppo_rnn_ref uses too) and distill_ref return their nn.Sequential with every nn.ELU replaced by the
    module of `name`."""
    def wrap(orig):
        def mlp(dims):
            net = orig(dims)
            for i, m in enumerate(net):
                if isinstance(m, nn.ELU):
                    net[i] = TORCH_ACT[name]()
            return net
        return mlp
    saved = (R.mlp, DR.mlp)
    R.mlp, DR.mlp = wrap(saved[0]), wrap(saved[1])
    try:
        yield
    finally:
        R.mlp, DR.mlp = saved


class ZeroWatch:
    """Forward hooks on the hidden Linear layers of the given nn.Sequential nets: .margin is the smallest |v| / (64 x 2^-24 (sum|x w| + |b|)) seen"""

    def __init__(self, *nets):
        self.margin, self.handles = math.inf, []
        for net in nets:
            linears = [m for m in net if isinstance(m, nn.Linear)]
            for lin in linears[:-1]:
                self.handles.append(lin.register_forward_hook(self._hook))

    def _hook(self, lin, inputs, out):
        with torch.no_grad():
            x = inputs[0].detach()
            mag = x.abs() @ lin.weight.detach().abs().T + lin.bias.detach().abs()
            self.margin = min(self.margin, float((out.detach().abs() / (64 * U24 * mag)).min()))

    def close(self):
        for h in self.handles:
            h.remove()


def walk_seeds(build, start, tries=20):
    """build(seed) -> case or None (condition not met); -> the first case, with .seed set"""
    for seed in range(start, start + tries):
        case = build(seed)
        if case is not None:
            case.seed = seed
            return case
    raise AssertionError(f"no seed in {start} .. {start + tries - 1} meets the case's condition")


# ---- 1. elementwise -----------------------------------------------------------------------------------------------------------------------------
EDGES = [0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, 1e-7, -1e-7, 20.0, -20.0, 43.6, -43.6, 44.0, -44.0, 87.0, -87.0, 88.5, -88.5, 100.0, -100.0, 3e38, -3e38,
         float("inf"), float("-inf"), float("nan")]


@functools.lru_cache(maxsize=None)
def elementwise_inputs():
    """[rows][16] float32: a sweep over [-30, 30], normal draws at unit scale and near 0, and the finite edge values"""
    rng = np.random.default_rng(12)
    v = np.concatenate([np.linspace(-30.0, 30.0, 3001), rng.standard_normal(1000), rng.standard_normal(500) * 1e-3, np.asarray([e for e in EDGES if math.isfinite(e)])])
    v = np.concatenate([v, np.zeros(-len(v) % 16)]).astype(np.float32).reshape(-1, 16)
    v.setflags(write=False)
    return v


def identity_params(n=16):
    eye = np.eye(n, dtype=np.float32)
    return np.concatenate([eye.reshape(-1), np.zeros(n, np.float32), eye.reshape(-1), np.zeros(n, np.float32)])


# ---- 2. forward ---------------------------------------------------------------------------------------------------------------------------------
FWD_DIMS = {"w24": [19, 24, 8],                              # a width that is no multiple of 16, mlp_layer<1>
            "w96": [45, 96, 40, 12],                         # mlp_layer<2> then <1>
            "w224": [49, 224, 96, 16],                       # mlp_layer<4>
            "nohidden": [7, 5]}                              # no hidden layer: the activation is not applied
CRITIC_DIMS = {"c96": [60, 96, 40, 1]}                       # the critic next to "w96" in one policy_act launch
FWD_DIMS_ALL = dict(FWD_DIMS, **CRITIC_DIMS)
FWD_ROWS = (1, 37)


def tile_group(width):
    per_wave = ((width + 15) // 16 + 3) // 4
    return 4 if per_wave >= 4 else 2 if per_wave >= 2 else 1


assert [tile_group(w) for w in (24, 96, 40, 224)] == [1, 2, 1, 4]


def conditioned(name, pre):
    for v in pre[:-1]:
        if name in AR.SATURATING:
            if min((np.abs(v) < 0.5).mean(), (np.abs(v) > 3.0).mean()) < 0.1:
                return False
        elif name in AR.PIECEWISE:
            if min((v > 0).mean(), (v < 0).mean()) < 0.2:
                return False
    return True


def yardstick_is_no_outlier(name, dims, params, x, pre, y64):
    """With fewer than 8 outputs E32 is a maximum over a handful of rounding-error samples, at one row of a critic over a single one, and a single
    |mlp32_plain - mlp64| is now and then far below its usual size (down to exactly 0): a ratio against it then says nothing about any evaluation.  Such
    a case is accepted only if some output's sample (E32 is their maximum) is at least a quarter of 2^-24 x (the last layer's sum_k |a_k w_k| + |b|), the
    rounding a float32 evaluation of that dot product spends on the size of its terms (numpy's own order has its median at 0.4 of it).  A condition on the reference alone,
    as the existing one-row, one-output case d2_t5 of tests/policy_cases.py is held to C_MLP."""
    if y64.size >= 8:
        return True
    W, b = AR.split_params(dims, params)[-1]
    a = AR.act64(name, pre[-2]) if len(pre) > 1 else np.asarray(x, np.float64)
    mag = np.abs(a) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))
    sample = np.abs(AR.mlp32_plain(name, dims, params, x).astype(np.float64) - y64)
    return bool((sample >= 0.25 * U24 * mag).any())


def shaped_net(name, dims, x, seed):
    """nn.Linear's default draws; then every hidden layer is shifted to a zero median and scaled to a standard deviation of 2.2 of its float64
    pre-activations, so that both sides of 0, the linear regime and the saturated one all occur"""
    rng = np.random.default_rng(seed)
    chunks, a = [], np.asarray(x, np.float64)
    for l in range(len(dims) - 1):
        bound = 1.0 / math.sqrt(dims[l])
        W, b = rng.uniform(-bound, bound, (dims[l + 1], dims[l])), rng.uniform(-bound, bound, dims[l + 1])
        if l < len(dims) - 2:
            v = a @ W.T + b
            b = b - np.median(v)
            s = 2.2 / max(float((v - np.median(v)).std()), 1e-12)
            W, b = (W * s).astype(np.float32), (b * s).astype(np.float32)
            a = AR.act64(name, a @ W.astype(np.float64).T + b.astype(np.float64))
        chunks += [np.asarray(W, np.float32).reshape(-1), np.asarray(b, np.float32)]
    return np.concatenate(chunks)


class FwdCase:
    pass


@functools.lru_cache(maxsize=None)
def fwd_case(name, shape, rows):
    dims = FWD_DIMS_ALL[shape]

    def build(seed):
        x = np.random.default_rng(1000 + seed).standard_normal((rows, dims[0])).astype(np.float32)
        params = shaped_net(name, dims, x, seed)
        pre = []
        y64 = AR.mlp64(name, dims, params, x, pre)
        if not conditioned(name, pre) or not yardstick_is_no_outlier(name, dims, params, x, pre, y64):
            return None
        c = FwdCase()
        c.name, c.dims, c.rows, c.x, c.params, c.y64 = name, dims, rows, x, params, y64
        c.e32 = AR.mlp_yardstick(name, dims, params, x)[1]
        for a in (x, params, y64):
            a.setflags(write=False)
        return c
    return walk_seeds(build, fwd_start(shape, rows))


def fwd_start(shape, rows):
    return 100 * list(FWD_DIMS_ALL).index(shape) + rows


# ---- 4. PPO gradients and updates ---------------------------------------------------------------------------------------------------------------
PPO_NETS = {"w24": ([19, 24, 8], [23, 24, 1]), "w96": ([45, 96, 40, 12], [60, 96, 40, 1])}
# (name, net, rows per mini-batch); 530 rows once: more than one GO2SIM_PPO_ROW_CHUNK
PPO_GRAD_CASES = [(n, net, 80) for n in NEW_NAMES for net in sorted(PPO_NETS)] + [("relu", "w24", 530)]
# (name, net): 80 rows, one epoch of two mini-batches of 40 rows
PPO_UPDATE_CASES = [(n, net) for n in NEW_NAMES for net in sorted(PPO_NETS)]


def case_id(c):
    return "-".join(str(x) for x in c)


class PpoCase:
    pass


@functools.lru_cache(maxsize=None)
def ppo_grad_case(name, net, n_rows):
    adims, cdims = PPO_NETS[net]
    kl_case = ("down", "up", "keep")[NEW_NAMES.index(name) % 3]

    def build(seed):
        with swapped(name):
            g = torch.Generator().manual_seed(seed)
            state = PC.init_state(adims, cdims, g)
            total = n_rows + 3                               # the mini-batch is a selection of a longer rollout, as in ppo_cases.Case
            idx = torch.randperm(total, generator=g)[:n_rows].to(torch.int32)
            ro = PC.make_rollout(adims, cdims, state, n_rows, kl_case, seed + 1)
            rollout = {k: torch.full((total,) + tuple(x.shape[1:]), float("nan")) for k, x in ro.items()}
            for k, x in ro.items():
                rollout[k][idx.long()] = x
            ref = {}
            for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
                m = R.make_model(adims, cdims, state, dt)
                assert all(isinstance(mod, (nn.Linear, TORCH_ACT[name])) for mod in list(m.actor) + list(m.critic))
                watch = ZeroWatch(m.actor, m.critic) if prec == "f64" else None
                grads, scal = R.minibatch_grad(m, R.rows_of(rollout, idx.long(), dt))
                if watch is not None:
                    watch.close()
                    if name in AR.JUMP and not watch.margin > 1.0:
                        return None
                ref[prec] = (grads, scal, m)
        c = PpoCase()
        c.name, c.adims, c.cdims, c.n, c.kl_case, c.state, c.idx, c.rollout, c.ref = name, adims, cdims, n_rows, kl_case, state, idx, rollout, ref
        return c
    return walk_seeds(build, 20000 + 101 * PPO_GRAD_CASES.index((name, net, n_rows)))


@functools.lru_cache(maxsize=None)
def ppo_update_case(name, net):
    adims, cdims = PPO_NETS[net]
    rows, epochs, n_mb = 80, 1, 2

    def build(seed):
        with swapped(name):
            g = torch.Generator().manual_seed(seed)
            state = PC.init_state(adims, cdims, g)
            ro = PC.make_rollout(adims, cdims, state, rows, "keep", seed + 1)
            perm = torch.randperm(rows, generator=g).to(torch.int32)
            out = {}
            for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
                m = R.make_model(adims, cdims, state, dt)
                watch = ZeroWatch(m.actor, m.critic) if prec == "f64" else None
                means, lr, kls = R.update(m, ro, perm, epochs, n_mb)
                if watch is not None:
                    watch.close()
                    if name in AR.JUMP and not watch.margin > 1.0:
                        return None
                out[prec] = dict(params={k: p.detach().clone() for k, p in R.ordered_params(m)}, means=means, lr=lr, kls=kls)
        c = PpoCase()
        c.name, c.adims, c.cdims, c.state, c.rollout, c.perm, c.rows, c.epochs, c.n_mb = name, adims, cdims, state, ro, perm, rows, epochs, n_mb
        c.f64, c.f32 = out["f64"], out["f32"]
        return c
    return walk_seeds(build, 40000 + 101 * PPO_UPDATE_CASES.index((name, net)))


# ---- 5. recurrent (tanh) and distillation (relu) ------------------------------------------------------------------------------------------------
# the shape of ppo_rnn_cases' "h16-t3-n37-step0" (H 16, inputs 5 / 49, T 3, 37 envs, dones at step 0, a non-zero saved state) with the three-layer MLPs
# of that table behind the memories: that case's own MLPs have no hidden layer, and with none no activation is ever applied
RNN_NAME, RNN_SHAPE = "tanh", dict(H=16, Ia=5, Ic=49, T=3, nb=37, pattern="step0", init_kind="nonzero", depth=3)


class RnnCase:
    pass


@functools.lru_cache(maxsize=None)
def rnn_grad_case():
    s = RNN_SHAPE
    H, Ia, Ic, T, nb = s["H"], s["Ia"], s["Ic"], s["T"], s["nb"]
    adims, cdims = RC.dims_of(H, s["depth"])
    seed = 61000
    c = RnnCase()
    with swapped(RNN_NAME):
        g = torch.Generator().manual_seed(seed)
        state = RC.init_state(H, Ia, Ic, adims, cdims, g)
        ro, init = RC.make_block(H, Ia, Ic, adims, cdims, state, T, nb, s["pattern"], s["init_kind"], "down", seed + 1)
        c.B, c.e0 = nb + 3, RC.E0
        c.rollout, c.init = RC.embed(ro, init, nb, c.e0, c.B)
        c.ref = {}
        for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = RR.make_model(Ia, Ic, adims, cdims, state, dt)
            assert sum(isinstance(mod, nn.Tanh) for mod in m.actor) == 2 and not any(isinstance(mod, nn.ELU) for mod in list(m.actor) + list(m.critic))
            if prec == "f64":
                RC.check_margins(m, c.rollout, c.init, c.e0, nb, "down")
            c.ref[prec] = RR.minibatch_grad(m, c.rollout, c.init, c.e0, nb)
    c.seed, c.H, c.Ia, c.Ic, c.T, c.nb, c.adims, c.cdims, c.mdims, c.state = seed, H, Ia, Ic, T, nb, adims, cdims, ((Ia, H), (Ic, H)), state
    return c


@functools.lru_cache(maxsize=None)
def rnn_update_case():
    """one epoch of two mini-batches of 37 envs each, random dones"""
    s = RNN_SHAPE
    H, Ia, Ic, T, nb, n_mb, epochs = s["H"], s["Ia"], s["Ic"], s["T"], s["nb"], 2, 1
    adims, cdims = RC.dims_of(H, s["depth"])
    seed = 62000
    c = RnnCase()
    with swapped(RNN_NAME):
        g = torch.Generator().manual_seed(seed)
        state = RC.init_state(H, Ia, Ic, adims, cdims, g)
        ro, init = RC.make_block(H, Ia, Ic, adims, cdims, state, T, nb * n_mb, "random", "nonzero", "keep", seed + 1)
        m64 = RR.make_model(Ia, Ic, adims, cdims, state, torch.float64)
        for i in range(n_mb):
            RC.check_margins(m64, ro, init, i * nb, nb, None)
        for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = RR.make_model(Ia, Ic, adims, cdims, state, dt)
            means, lr, kls = RR.update(m, ro, init, epochs, n_mb)
            setattr(c, prec, dict(params={k: p.detach().clone() for k, p in RR.ordered_params(m)}, means=means, lr=lr, kls=kls))
    c.seed, c.H, c.Ia, c.Ic, c.T, c.nb, c.B, c.n_mb, c.epochs = seed, H, Ia, Ic, T, nb, nb * n_mb, n_mb, epochs
    c.adims, c.cdims, c.mdims, c.state, c.rollout, c.init = adims, cdims, ((Ia, H), (Ic, H)), state, ro, init
    return c


DISTILL_NAME = "relu"
DISTILL_SDIMS, DISTILL_TDIMS = [45, 96, 40, 12], [60, 24, 12]


class DistillCase:
    pass


@functools.lru_cache(maxsize=None)
def distill_grad_case():
    """one window of three steps over 37 envs (111 rows), Huber loss"""
    N, G, loss_type = 37, 3, "huber"

    def build(seed):
        c = DistillCase()
        with swapped(DISTILL_NAME):
            g = torch.Generator().manual_seed(seed)
            c.state = DC.init_state(DISTILL_SDIMS, DISTILL_TDIMS, g)
            c.T, c.steps = G + 1, list(range(G - 1, -1, -1))
            c.obs, c.ta = DC.make_storage(DISTILL_SDIMS, DISTILL_TDIMS, c.state, c.T, N, seed + 1)
            c.obs[-1] = float("nan"); c.ta[-1] = float("nan")                # the storage's last step belongs to no window
            c.idx = torch.cat([t * N + torch.arange(N) for t in c.steps]).to(torch.int32)
            c.ref = {}
            for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
                m = DR.make_model(DISTILL_SDIMS, DISTILL_TDIMS, c.state, dt)
                assert sum(isinstance(mod, nn.ReLU) for mod in m.student) == 2
                watch = ZeroWatch(m.student) if prec == "f64" else None
                c.ref[prec] = DR.window_grad(m, c.obs.to(dt), c.ta.to(dt), c.steps, loss_type)
                if watch is not None:
                    watch.close()
                    if not watch.margin > 1.0:
                        return None
        c.N, c.G, c.loss_type, c.sdims, c.tdims = N, G, loss_type, DISTILL_SDIMS, DISTILL_TDIMS
        return c
    return walk_seeds(build, 63000)


@functools.lru_cache(maxsize=None)
def distill_update_case():
    """T = 4 steps, one epoch, windows of 2 steps: two optimizer steps over 37 envs"""
    T, E, G, N = 4, 1, 2, 37

    def build(seed):
        c = DistillCase()
        with swapped(DISTILL_NAME):
            g = torch.Generator().manual_seed(seed)
            c.state = DC.init_state(DISTILL_SDIMS, DISTILL_TDIMS, g)
            c.obs, c.ta = DC.make_storage(DISTILL_SDIMS, DISTILL_TDIMS, c.state, T, N, seed + 1)
            for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
                m = DR.make_model(DISTILL_SDIMS, DISTILL_TDIMS, c.state, dt)
                watch = ZeroWatch(m.student) if prec == "f64" else None
                loss, norms = DR.update(m, c.obs.to(dt), c.ta.to(dt), E, G, DR.HP)
                if watch is not None:
                    watch.close()
                    if not watch.margin > 1.0:
                        return None
                setattr(c, prec, dict(params={k: p.detach().clone() for k, p in DR.ordered_params(m)}, loss=loss, norms=norms))
        c.T, c.E, c.G, c.N, c.sdims, c.tdims = T, E, G, N, DISTILL_SDIMS, DISTILL_TDIMS
        return c
    return walk_seeds(build, 64000)
