"""The case table of the random-network-distillation tests (tests/test_rnd_ref.py on the CPU, tests/test_rnd_gpu.py on the GPU): networks, shapes, inputs and
the float64 / float32 evaluations of the law (tests/rnd_ref.py), computed once per case and shared.

The shapes are the smallest at which the kernels can go wrong: rows N in {1, 17, 37, 257, 1000} (one lane, an odd count below a 32-row tile, above it, one row
past the 256-row chunk of the moments, four chunks with a short last one), state widths {3, 45, 49} (none a multiple of 16), embedding widths {1, 12, 20, 32},
a predictor deeper than the target and the reverse, one hidden width of 272 (more than one 256 tile) and two activations (elu, tanh: both with a continuous
derivative, so that a pre-activation that rounds across zero moves no gradient by a jump)."""
import functools

import torch

import ppo_cases as PC
import rnd_ref as R

ROW_CHUNK = PC.ROW_CHUNK
# name: (predictor layer sizes, target layer sizes, activation)
NETS = {
    "tiny_e1": ([3, 8, 1], [3, 5, 4, 1], "elu"),                 # the target deeper; one output
    "obs45_e12": ([45, 32, 24, 12], [45, 20, 12], "tanh"),       # the predictor deeper
    "wide_e20": ([49, 272, 20], [49, 49, 20], "elu"),            # a hidden width past one 256 tile
    "default_e32": ([49, 49, 32], [49, 49, 32], "tanh"),         # rnd_cfg's default hidden_dims [-1]
}
ROWS = (1, 17, 37, 257, 1000)
STEP_CASES = [(net, n) for net in NETS for n in ROWS]
# (net, rows of the mini-batch, kind of index list): "perm" a permutation of all stored rows, "dup" rows drawn with repetition from a larger storage
GRAD_CASES = [("tiny_e1", 17, "perm"), ("tiny_e1", 37, "dup"), ("obs45_e12", 17, "dup"), ("obs45_e12", 37, "perm"), ("wide_e20", 17, "perm"), ("wide_e20", 37, "dup"),
              ("default_e32", 37, "perm"), ("obs45_e12", ROW_CHUNK + 37, "dup"), ("default_e32", ROW_CHUNK + 37, "perm")]
UPDATE_SCHEDULES = [(1, 1), (2, 2), (5, 4)]                      # (epochs, mini-batches)
UPDATE_CASES = [(net, sched) for net in ("tiny_e1", "obs45_e12", "wide_e20") for sched in UPDATE_SCHEDULES]
UPDATE_ROWS = 4 * 37                                             # mini-batches of 148, 74 and 37 rows


def case_id(c):
    return "-".join("x".join(str(v) for v in x) if isinstance(x, tuple) else str(x) for x in c)


def net_state(net, seed):
    pdims, tdims, _ = NETS[net]
    return R.init_state(pdims, tdims, torch.Generator().manual_seed(seed))


def states(net, n, seed):
    """n rows of rnd_state, float32"""
    return torch.randn(n, NETS[net][0][0], generator=torch.Generator().manual_seed(seed)).float()


class GradCase:
    def __init__(self, net, n, kind, seed):
        self.net, self.n, self.kind = net, n, kind
        self.pdims, self.tdims, self.act = NETS[net]
        self.state = net_state(net, seed)
        g = torch.Generator().manual_seed(seed + 1)
        n_store = n if kind == "perm" else n + 11
        self.s = states(net, n_store, seed + 2)
        self.idx = (torch.randperm(n, generator=g) if kind == "perm" else torch.randint(0, n_store, (n,), generator=g)).to(torch.int32)
        if kind == "dup":
            self.idx[-1] = self.idx[0]                           # at least one row twice
        self.ref = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = R.make_model(self.pdims, self.tdims, self.act, self.state, dt)
            grads, loss, dp, p, t = R.minibatch_grad(m, self.s.to(dt), self.idx)
            self.ref[name] = dict(grads=grads, loss=loss, dp=dp, p=p, t=t)


@functools.lru_cache(maxsize=None)
def get_grad_case(net, n, kind):
    c = (net, n, kind)
    return GradCase(*c, seed=7000 + 13 * GRAD_CASES.index(c) if c in GRAD_CASES else 77)


@functools.lru_cache(maxsize=None)
def get_update_case(net, sched):
    E, nmb = sched
    pdims, tdims, act = NETS[net]
    seed = 9000 + 100 * list(NETS).index(net) + 10 * E + nmb
    state = net_state(net, seed)
    s = states(net, UPDATE_ROWS, seed + 1)
    idx = torch.randperm(UPDATE_ROWS, generator=torch.Generator().manual_seed(seed + 2)).to(torch.int32)
    out = dict(net=net, pdims=pdims, tdims=tdims, act=act, state=state, s=s, idx=idx, E=E, nmb=nmb, n=UPDATE_ROWS)
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = R.make_model(pdims, tdims, act, state, dt)
        loss = R.update(m, s.to(dt), idx, UPDATE_ROWS, E, nmb)
        out[prec] = dict(params={k: p.detach().clone() for k, p in R.ordered_params(m)}, loss=loss)
    return out
