"""The case table of the recurrent PPO tests (tests/test_ppo_rnn_ref.py, tests/test_ppo_rnn_gpu.py): memories, networks, rollouts of T x B rows, done
patterns and saved states, at the smallest shapes where each piece can go wrong:
  H   16 (one tile), 20 (padding), 48          I   5, 49          T   1, 3, 8          envs per mini-batch   1, 17, 37, 70
  (T = 8 with 70 envs: 560 rows, across a 512-row chunk; 37 and 70 envs: more than one 32-row tile)
  and, past the first column group of the LSTM kernels (a workgroup owns NWAVE x 16 = 64 hidden units, blockIdx.y walks the further groups):
  H   80 (a second group with one live wavefront), 68 (the padded tile lies in the second group), 256 (the product width, four groups, with the
  product's input widths 49 and 104), 512 (GO2SIM_MLP_MAX_WIDTH, eight groups);   I   64 (no input padding), 104;   envs per mini-batch   5, 33.
  dones: none | the last step only | step 0 | one env on every step | random at rate 0.2;   a zero and a non-zero saved state;   MLP depths 1 and 3.
The observations are scaled so that the gate pre-activations have a standard deviation near 2: saturated and linear gate regimes both occur
(check_regimes: at least a tenth of them on each side of +-2).  The per-row PPO inputs are built as in tests/ppo_cases.py, from the float64 forward, so
that every branch decision of the law has a margin.  The block sits at env offset 2 of a rollout of nb + 3 envs; the other envs hold NaN.
Everything is float32-exact; a case's float64 and float32 evaluations are computed once and shared."""
import functools
import math

import torch

import ppo_cases as PC
import ppo_ref as R
import ppo_rnn_ref as RR

A = 3
E0 = 2                                                      # the block's first env
PATTERNS = ("none", "last", "step0", "every", "random")
# name: (H, I actor, I critic, T, envs per mini-batch, dones, saved state, MLP depth, schedule case)
GRAD_CASES = {
    "h16-t1-n1": (16, 5, 5, 1, 1, "none", "zero", 1, "keep"),
    "h20-t3-n17-last": (20, 5, 49, 3, 17, "last", "nonzero", 3, "down"),
    "h20-t3-n17-none": (20, 5, 49, 3, 17, "none", "nonzero", 3, "down"),     # the same numbers without the dones at the last step
    "h48-t8-n37-random": (48, 49, 5, 8, 37, "random", "nonzero", 1, "up"),
    "h20-t8-n70-every": (20, 49, 49, 8, 70, "every", "nonzero", 3, "keep"),
    "h16-t3-n37-step0": (16, 5, 49, 3, 37, "step0", "nonzero", 1, "down"),
    "h48-t8-n17-none": (48, 5, 5, 8, 17, "none", "zero", 3, "up"),
    "h20-t1-n70-random": (20, 49, 5, 1, 70, "random", "nonzero", 1, "keep"),
    "h16-t8-n1-random": (16, 49, 49, 8, 1, "random", "zero", 3, "down"),
    # the further column groups
    "h80-i64-t2-n33-step0": (80, 64, 49, 2, 33, "step0", "nonzero", 1, "keep"),
    "h68-t3-n17-random": (68, 49, 5, 3, 17, "random", "nonzero", 3, "down"),
    "h256-i104-t2-n5-step0": (256, 49, 104, 2, 5, "step0", "nonzero", 3, "up"),
    "h512-t2-n1-none": (512, 5, 5, 2, 1, "none", "nonzero", 1, "keep"),
}
# A case's seed comes from its position in one of these two lists, never from the table's size: a new name leaves every earlier case's inputs alone.
SEED_NAMES_0 = ("h16-t1-n1", "h16-t3-n37-step0", "h16-t8-n1-random", "h20-t1-n70-random", "h20-t3-n17-last", "h20-t3-n17-none", "h20-t8-n70-every",
                "h48-t8-n17-none", "h48-t8-n37-random")                       # the first nine, sorted: seed 5000 + 31 index
SEED_NAMES_1 = ("h80-i64-t2-n33-step0", "h68-t3-n17-random", "h256-i104-t2-n5-step0", "h512-t2-n1-none")      # seed 9000 + 31 index; append only
NWAVE = 4                                                   # wavefronts (16-unit column tiles) of a k_lstm_cell / k_lstm_bptt workgroup
# name: 2 epochs x 2 mini-batches, random dones, non-zero state
UPDATE_CASES = {
    "h20-t3-n17": dict(H=20, Ia=5, Ic=49, T=3, nb=17, n_mb=2, epochs=2, depth=3, seed=777),      # mini-batches of 51 rows
    "h80-i64-t2-n17": dict(H=80, Ia=64, Ic=49, T=2, nb=17, n_mb=2, epochs=2, depth=1, seed=877),  # the second column group through whole updates
}
UPDATE_CASE = UPDATE_CASES["h20-t3-n17"]


def dims_of(H, depth):
    return ([H, 17, 33, A], [H, 17, 33, 1]) if depth == 3 else ([H, A], [H, 1])


def init_state(H, Ia, Ic, adims, cdims, gen):
    sd = PC.init_state(adims, cdims, gen)
    for prefix, n_in in (("memory_a", Ia), ("memory_c", Ic)):        # nn.LSTM's default init
        for k, shape in (("weight_ih_l0", (4 * H, n_in)), ("weight_hh_l0", (4 * H, H)), ("bias_ih_l0", (4 * H,)), ("bias_hh_l0", (4 * H,))):
            sd[f"{prefix}.rnn.{k}"] = ((torch.rand(*shape, generator=gen) * 2 - 1) / math.sqrt(H)).float()
    return sd


def make_dones(pattern, T, n, gen):
    d = torch.zeros(T, n, dtype=torch.uint8)
    if pattern == "last":
        d[T - 1, ::2] = 1
    elif pattern == "step0":
        d[0, ::2] = 1
    elif pattern == "every":
        d[:, 0] = 1
    elif pattern == "random":
        d = (torch.rand(T, n, generator=gen) < 0.2).to(torch.uint8)
    return d


def obs_scale(n_in, H):
    """x ~ N(0, s^2) with W_ih uniform(+- 1 / sqrt(H)): the pre-activation's standard deviation from x is s sqrt(n_in / (3 H)); s makes it 2"""
    return 2.0 * math.sqrt(3.0 * H / n_in)


def check_regimes(z):
    frac = float((z.abs() > 2.0).double().mean())
    assert 0.1 <= frac <= 0.9, frac


def make_block(H, Ia, Ic, adims, cdims, state, T, n, pattern, init_kind, kl_case, seed, hp=R.HP):
    """A rollout of T x n rows ([T][n][...] float32 tensors by key + "dones") and the saved state, with the margins of tests/ppo_cases.py under `state`."""
    g = torch.Generator().manual_seed(seed)
    clip = hp["clip_param"]
    m64 = RR.make_model(Ia, Ic, adims, cdims, state, torch.float64)
    ro = dict(obs=(obs_scale(Ia, H) * torch.randn(T, n, Ia, generator=g)).float(), critic_obs=(obs_scale(Ic, H) * torch.randn(T, n, Ic, generator=g)).float(),
              dones=make_dones(pattern, T, n, g))
    mk = (lambda: (0.5 * torch.randn(n, H, generator=g)).float()) if init_kind == "nonzero" else (lambda: torch.zeros(n, H))
    init = dict(h_a=mk().clamp(-0.9, 0.9), c_a=mk(), h_c=mk().clamp(-0.9, 0.9), c_c=mk())
    with torch.no_grad():
        mu, v, (za, zc) = RR.forward(m64, ro, init, 0, n)
    check_regimes(za); check_regimes(zc)
    rows = T * n
    sigma = state["std"].double()
    actions = (mu + sigma * torch.randn(rows, A, generator=g).double()).float()
    old_sigma = (sigma * (0.9 + 0.2 * torch.rand(rows, A, generator=g).double())).float()
    noise = torch.randn(rows, A, generator=g).double()
    k0 = float((torch.log(sigma / old_sigma.double() + 1e-5) + old_sigma.double() ** 2 / (2 * sigma ** 2) - 0.5).sum(-1).mean())
    q = float((noise ** 2 / 2).sum(-1).mean())
    target = PC.KL_TARGET[kl_case]
    if k0 >= target:
        old_sigma = sigma.float().expand(rows, A).contiguous()
        k0 = A * math.log(1 + 1e-5)
    old_mu = (mu + math.sqrt(max(target - k0, 0.0) / q) * sigma * noise).float()
    with torch.no_grad():
        logp = torch.distributions.Normal(mu, mu * 0 + sigma).log_prob(actions.double()).sum(-1)
    i = torch.arange(rows)
    ratio = PC._bands(torch.rand(rows, generator=g).double(), [(0.5, 0.75), (0.85, 1.15), (1.25, 2.0)])
    old_log_prob = (logp - torch.log(ratio)).float()
    sign = torch.where((i // 3) % 2 == 0, 1.0, -1.0).double()
    adv = (sign * (0.2 + 1.8 * torch.rand(rows, generator=g).double())).float()
    dv = PC._bands(torch.rand(rows, generator=g).double(), [(0.0, 0.15), (0.25, 1.0)]) * torch.where((i // 2) % 2 == 0, 1.0, -1.0).double()
    tv = (v - dv).float()
    vc = tv.double() + (v - tv.double()).clamp(-clip, clip)
    ret = ((v + vc) / 2 + torch.where((i // 4) % 2 == 0, 1.0, -1.0).double() * (0.05 + 0.95 * torch.rand(rows, generator=g).double())).float()
    flat = dict(actions=actions, target_values=tv, returns=ret, advantages=adv, old_log_prob=old_log_prob, old_mu=old_mu, old_sigma=old_sigma)
    for k, x in flat.items():
        ro[k] = x.reshape((T, n) + tuple(x.shape[1:])).contiguous()
    return ro, init


def check_margins(m64, ro, init, e0, nb, kl_case, hp=R.HP):
    """The construction's promise on the float32-rounded inputs (kl_case None: the per-row margins only)"""
    clip, dkl = hp["clip_param"], hp["desired_kl"]
    with torch.no_grad():
        _, t = RR.loss_terms(m64, ro, init, e0, nb, hp)
    rows = RR.block_rows(ro, e0, nb, torch.float64)
    ratio, v = t["ratio"], t["v"]
    assert bool((((ratio - (1 - clip)).abs() > 0.04) & ((ratio - (1 + clip)).abs() > 0.04)).all())
    d = (v - rows["target_values"]).abs()
    assert bool(((d - clip).abs() > 0.04).all())
    vc = rows["target_values"] + (v - rows["target_values"]).clamp(-clip, clip)
    assert bool(((rows["returns"] - (v + vc) / 2).abs() > 0.049).all())
    kl = float(t["kl_mean"])
    if kl_case == "down":
        assert kl > 1.2 * 2 * dkl, kl
    elif kl_case == "up":
        assert 0 < kl < 0.8 * dkl / 2, kl
    elif kl_case == "keep":
        assert 1.2 * dkl / 2 < kl < 0.8 * 2 * dkl, kl


def embed(ro, init, n, e0, total):
    """The block at envs [e0, e0 + n) of a rollout of `total` envs; the other envs hold values no mini-batch may read (NaN, dones set)"""
    big = {}
    for k, x in ro.items():
        shape = (x.shape[0], total) + tuple(x.shape[2:])
        big[k] = torch.ones(shape, dtype=torch.uint8) if k == "dones" else torch.full(shape, float("nan"))
        big[k][:, e0:e0 + n] = x
    big_init = {}
    for k, x in init.items():
        big_init[k] = torch.full((total, x.shape[1]), float("nan"))
        big_init[k][e0:e0 + n] = x
    return big, big_init


class Case:
    """One recurrent mini-batch: state, rollout [T][B], saved state [B][H], block (E0, nb), and the float64 / float32 evaluations"""

    def __init__(self, name, seed):
        self.name = name
        self.H, self.Ia, self.Ic, self.T, self.nb, self.pattern, self.init_kind, self.depth, self.kl_case = GRAD_CASES[name]
        self.adims, self.cdims = dims_of(self.H, self.depth)
        self.mdims = ((self.Ia, self.H), (self.Ic, self.H))
        self.B, self.e0 = self.nb + 3, E0
        g = torch.Generator().manual_seed(seed)
        self.state = init_state(self.H, self.Ia, self.Ic, self.adims, self.cdims, g)
        ro, init = make_block(self.H, self.Ia, self.Ic, self.adims, self.cdims, self.state, self.T, self.nb, self.pattern, self.init_kind, self.kl_case, seed + 1)
        self.rollout, self.init = embed(ro, init, self.nb, self.e0, self.B)
        self.ref = {}
        for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
            m = RR.make_model(self.Ia, self.Ic, self.adims, self.cdims, self.state, dt)
            if prec == "f64":
                check_margins(m, self.rollout, self.init, self.e0, self.nb, self.kl_case)
            grads, scal = RR.minibatch_grad(m, self.rollout, self.init, self.e0, self.nb)
            self.ref[prec] = (grads, scal, m)

    def unrolled(self, dt):
        """{"a": (h' [T][nb][H], c after the last step), "c": ...} of the two memories over the block in `dt`"""
        m = RR.make_model(self.Ia, self.Ic, self.adims, self.cdims, self.state, dt)
        sl = slice(self.e0, self.e0 + self.nb)
        out = {}
        with torch.no_grad():
            for key, lstm, x in (("a", m.memory_a.rnn, self.rollout["obs"]), ("c", m.memory_c.rnn, self.rollout["critic_obs"])):
                hs, (_, c), _ = RR.unroll(lstm, x[:, sl].to(dt), self.init["h_" + key][sl].to(dt), self.init["c_" + key][sl].to(dt), self.rollout["dones"][:, sl])
                out[key] = (hs, c)
        return out


@functools.lru_cache(maxsize=None)
def get_case(name):
    # the "last" / "none" pair shares its seed: the dones at the last step must not change anything within the rollout
    key = name.replace("-last", "-none") if name.endswith("-last") else name
    seed = 5000 + 31 * SEED_NAMES_0.index(key) if key in SEED_NAMES_0 else 9000 + 31 * SEED_NAMES_1.index(key)
    return Case(name, seed)


@functools.lru_cache(maxsize=None)
def get_update_case(name="h20-t3-n17"):
    u = UPDATE_CASES[name]
    H, Ia, Ic, T, nb, n_mb = u["H"], u["Ia"], u["Ic"], u["T"], u["nb"], u["n_mb"]
    adims, cdims = dims_of(H, u["depth"])
    g = torch.Generator().manual_seed(u["seed"])
    state = init_state(H, Ia, Ic, adims, cdims, g)
    ro, init = make_block(H, Ia, Ic, adims, cdims, state, T, nb * n_mb, "random", "nonzero", "keep", u["seed"] + 1)
    m64 = RR.make_model(Ia, Ic, adims, cdims, state, torch.float64)
    for i in range(n_mb):
        check_margins(m64, ro, init, i * nb, nb, None)
    out = dict(H=H, Ia=Ia, Ic=Ic, adims=adims, cdims=cdims, mdims=((Ia, H), (Ic, H)), state=state, rollout=ro, init=init, T=T, B=nb * n_mb, nb=nb, n_mb=n_mb,
               epochs=u["epochs"])
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = RR.make_model(Ia, Ic, adims, cdims, state, dt)
        means, lr, kls = RR.update(m, ro, init, u["epochs"], n_mb)
        out[prec] = dict(params={k: p.detach().clone() for k, p in RR.ordered_params(m)}, means=means, lr=lr, kls=kls)
    return out
