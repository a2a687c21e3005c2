"""The case table of the PPO-update tests (tests/test_ppo_gpu.py): networks, row counts and inputs.  The inputs are constructed from the float64
forward so that every branch decision of the law has a margin (no row is ever excluded from a comparison):
  * target ratios from [0.5, 0.75] u [0.85, 1.15] u [1.25, 2], set through old_log_prob, both signs of advantage in every band;
  * |v - target_values| from [0, 0.15] u [0.25, 1];  returns at least 0.05 away from the midpoint of v and v_clipped;
  * kl_mean at least 20 % away from desired_kl / 2 and 2 desired_kl (three schedule cases: "down", "up", "keep").
Everything is float32-exact: the float64 reference, the float32 yardstick and the HIP library read the same numbers.
A case's float64 and float32 evaluations are computed once and shared by the tests that need them."""
import functools
import math

import torch

import ppo_ref as R

ROW_CHUNK = 512                                             # GO2SIM_PPO_ROW_CHUNK (tests/test_ppo_capi.py checks the header says the same)
NETS = {
    "one_layer": ([5, 4], [7, 1]),                          # no hidden backward at all
    "small": ([49, 32, 16], [104, 32, 1]),
    "six_layers": ([3, 17, 33, 16, 15, 20, 4], [3, 17, 33, 16, 15, 20, 1]),   # no width a multiple of 16
    "full": ([45, 512, 256, 128, 12], [100, 512, 256, 128, 1]),
}
ROWS = (1, 15, 16, 17, 37, 2 * ROW_CHUNK + 37)
KL_TARGET = {"down": 0.05, "up": 0.002, "keep": 0.01}       # desired_kl = 0.01: thresholds 0.02 and 0.005
# (net, rows per mini-batch, schedule case); the full widths at 80 rows only
GRAD_CASES = [(net, n, ("down", "up", "keep")[(i + j) % 3]) for i, net in enumerate(("one_layer", "small", "six_layers")) for j, n in enumerate(ROWS)]
GRAD_CASES.append(("full", 80, "down"))


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}"


def init_state(adims, cdims, gen, scale=1.0):
    """nn.Linear's default init (uniform +- 1 / sqrt(fan_in)) times `scale`, std in [0.5, 1.5]; float32"""
    sd = {}
    for prefix, dims in (("actor", adims), ("critic", cdims)):
        for l in range(len(dims) - 1):
            bound = scale / math.sqrt(dims[l])
            sd[f"{prefix}.{2 * l}.weight"] = ((torch.rand(dims[l + 1], dims[l], generator=gen) * 2 - 1) * bound).float()
            sd[f"{prefix}.{2 * l}.bias"] = ((torch.rand(dims[l + 1], generator=gen) * 2 - 1) * bound).float()
    sd["std"] = (0.5 + torch.rand(adims[-1], generator=gen)).float()
    return sd


def _bands(u, bands):
    """u in [0, 1) -> a value in one of the intervals, cycling through them by row"""
    out = torch.empty_like(u)
    for i in range(u.numel()):
        lo, hi = bands[i % len(bands)]
        out[i] = lo + (hi - lo) * u[i]
    return out


def make_rollout(adims, cdims, state, n_rows, kl_case, seed, hp=R.HP):
    """`n_rows` rollout rows (float32 tensors by key) whose branch decisions have the margins above under `state`."""
    g = torch.Generator().manual_seed(seed)
    A, clip = adims[-1], hp["clip_param"]
    m64 = R.make_model(adims, cdims, state, torch.float64)
    obs = torch.randn(n_rows, adims[0], generator=g).float()
    cobs = torch.randn(n_rows, cdims[0], generator=g).float()
    with torch.no_grad():
        mu = m64.actor(obs.double())
        v = m64.critic(cobs.double()).squeeze(-1)
    sigma = state["std"].double()
    actions = (mu + sigma * torch.randn(n_rows, A, generator=g).double()).float()
    old_sigma = (sigma * (0.9 + 0.2 * torch.rand(n_rows, A, generator=g).double())).float()
    # kl_mean(c) with old_mu = mu + c sigma noise is c^2 q + k0: place it on the target
    noise = torch.randn(n_rows, A, generator=g).double()
    k0 = float((torch.log(sigma / old_sigma.double() + 1e-5) + old_sigma.double() ** 2 / (2 * sigma ** 2) - 0.5).sum(-1).mean())
    q = float((noise ** 2 / 2).sum(-1).mean())
    target = KL_TARGET[kl_case]
    if k0 >= target:                                        # the sigma part alone is too large for this target: old_sigma = sigma
        old_sigma = sigma.float().expand(n_rows, A).contiguous()
        k0 = A * math.log(1 + 1e-5)
    old_mu = (mu + math.sqrt(max(target - k0, 0.0) / q) * sigma * noise).float()
    with torch.no_grad():
        logp = torch.distributions.Normal(mu, mu * 0 + sigma).log_prob(actions.double()).sum(-1)
    i = torch.arange(n_rows)
    ratio = _bands(torch.rand(n_rows, generator=g).double(), [(0.5, 0.75), (0.85, 1.15), (1.25, 2.0)])
    old_log_prob = (logp - torch.log(ratio)).float()
    sign = torch.where((i // 3) % 2 == 0, 1.0, -1.0).double()                   # both signs in every band (the band cycles with i % 3)
    adv = (sign * (0.2 + 1.8 * torch.rand(n_rows, generator=g).double())).float()
    dv = _bands(torch.rand(n_rows, generator=g).double(), [(0.0, 0.15), (0.25, 1.0)]) * torch.where((i // 2) % 2 == 0, 1.0, -1.0).double()
    tv = (v - dv).float()
    vc = tv.double() + (v - tv.double()).clamp(-clip, clip)
    ret = ((v + vc) / 2 + torch.where((i // 4) % 2 == 0, 1.0, -1.0).double() * (0.05 + 0.95 * torch.rand(n_rows, generator=g).double())).float()
    ro = dict(obs=obs, critic_obs=cobs, actions=actions, target_values=tv, returns=ret, advantages=adv, old_log_prob=old_log_prob, old_mu=old_mu,
              old_sigma=old_sigma)
    check_margins(m64, ro, kl_case, hp)
    return ro


def check_margins(m64, ro, kl_case, hp=R.HP):
    """The construction's promise, on the float32-rounded inputs."""
    clip, dkl = hp["clip_param"], hp["desired_kl"]
    with torch.no_grad():
        _, t = R.loss_terms(m64, {k: x.double() for k, x in ro.items()}, hp)
    ratio, v = t["ratio"], t["v"]
    assert bool((((ratio - (1 - clip)).abs() > 0.04) & ((ratio - (1 + clip)).abs() > 0.04)).all())
    d = (v - ro["target_values"].double()).abs()
    assert bool(((d - clip).abs() > 0.04).all())
    vc = ro["target_values"].double() + (v - ro["target_values"].double()).clamp(-clip, clip)
    assert bool(((ro["returns"].double() - (v + vc) / 2).abs() > 0.049).all())
    kl = float(t["kl_mean"])
    if kl_case == "down":
        assert kl > 1.2 * 2 * dkl, kl
    elif kl_case == "up":
        assert 0 < kl < 0.8 * dkl / 2, kl
    else:
        assert 1.2 * dkl / 2 < kl < 0.8 * 2 * dkl, kl


class Case:
    """One mini-batch: the state, the rollout, the index array and the float64 / float32 evaluations of the law."""

    def __init__(self, net, n_rows, kl_case, seed):
        self.net, self.n, self.kl_case = net, n_rows, kl_case
        self.adims, self.cdims = NETS[net]
        total = n_rows + 3                                  # the mini-batch is a selection of a longer rollout: rows are read through the index
        g = torch.Generator().manual_seed(seed)
        self.state = init_state(self.adims, self.cdims, g)
        perm = torch.randperm(total, generator=g)
        self.idx = perm[:n_rows].to(torch.int32)
        ro = make_rollout(self.adims, self.cdims, self.state, n_rows, kl_case, seed + 1)
        # scatter the constructed rows to their places; the other rows hold values no mini-batch may read
        self.rollout = {k: torch.full((total,) + tuple(x.shape[1:]), float("nan")) for k, x in ro.items()}
        for k, x in ro.items():
            self.rollout[k][self.idx.long()] = x
        self.ref = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = R.make_model(self.adims, self.cdims, self.state, dt)
            grads, scal = R.minibatch_grad(m, R.rows_of(self.rollout, self.idx.long(), dt))
            self.ref[name] = (grads, scal, m)


@functools.lru_cache(maxsize=None)
def get_case(net, n_rows, kl_case):
    return Case(net, n_rows, kl_case, seed=1000 + 17 * GRAD_CASES.index((net, n_rows, kl_case)) if (net, n_rows, kl_case) in GRAD_CASES else 77)


# ---- whole updates on the small pair: (rows, epochs, mini-batches) ------------------------------------------------------------------------------
UPDATE_CASES = {
    "2x2": (74, 2, 2),                                      # 37 rows per mini-batch
    "3x7": (21, 1, 4),                                      # T = 3, B = 7: 5 rows per mini-batch, the permutation's last row is dropped
}


@functools.lru_cache(maxsize=None)
def get_update_case(name):
    rows, epochs, n_mb = UPDATE_CASES[name]
    adims, cdims = NETS["small"]
    g = torch.Generator().manual_seed(4242 + rows)
    state = init_state(adims, cdims, g)
    ro = make_rollout(adims, cdims, state, rows, "keep", 4243 + rows)
    used = n_mb * (rows // n_mb)
    perm = torch.randperm(used, generator=g).to(torch.int32)          # PPO.update: randperm(num_mini_batches * mini_batch_size)
    for k in ro:                                                       # rows beyond it are dropped: nothing may read them
        ro[k][used:] = float("nan")
    out = dict(adims=adims, cdims=cdims, state=state, rollout=ro, perm=perm, rows=rows, epochs=epochs, n_mb=n_mb)
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = R.make_model(adims, cdims, state, dt)
        means, lr, kls = R.update(m, ro, perm, epochs, n_mb)
        out[prec] = dict(params={k: p.detach().clone() for k, p in R.ordered_params(m)}, means=means, lr=lr, kls=kls)
    return out
