"""Float64 reference of the policy step and the rollout returns (include/go2sim_policy.h), in plain numpy.  It imports nothing of the project:
the networks are the published nn.Sequential(Linear, ELU, ..., Linear), the noise is Philox4x32-10 (Salmon et al., SC'11; the Random123 known
answers pin it) through Box-Muller with the counter layout the header states, the distribution is torch.distributions.Normal and the returns are
the rsl_rl 2.2.4 formulas the header quotes.  tests/policy_cases.py holds the cases and assertions that both the oracle builds
(tests/test_policy_ref.py) and the HIP library (tests/test_policy_gpu.py) are run through, so an answer that is wrong on both sides fails on both.

The constants below are the bounds of those assertions.  Each is twice the worst ratio the two oracle builds reach over the case tables of
policy_cases.py, rounded up to an integer, the ratio being taken against a yardstick of this reference alone (DESIGN.md "Policy step against
float64" has the tables).  The HIP library is bit-equal to the fast oracle on every case, so its own worst ratios are the fast oracle's."""
import math

import numpy as np

U24 = 2.0 ** -24
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)            # 0.9189385332046727

# bound = constant x yardstick                                      worst ratio measured: strict oracle / fast oracle / HIP library
C_MLP = 7         # x E32 (mlp_yardstick)                            3.07 / 3.07 / 3.07          (case d2_t31)
C_SAMPLE = 56     # x 2^-24 (|mean| + std max(1, |n|))               27.91 / 27.91 / 27.91      (A = 17, 70000 rows)
C_LOGP = 5        # x 2^-24 sum_a(z^2 / 2 + |log std| + 0.919)       2.27 / 2.27 / 2.27         (A = 3, 70000 rows)
C_GAE = 5         # x 2^-24 x magnitude of the summed terms          2.35 / 2.35 / 2.35         (5 x 257)
C_NORM = 6        # x 2^-24 (|adv| + |mean|) / std                   2.52 / 2.52 / 2.52         (24 x 513, dones all 0)
ELU_ABS = 4 * U24  # derived, not measured: dm_exp is held below 2 ulp of a value <= 1 (tests/test_detmath.py), plus the rounding of "- 1";
#                    measured 0.33 x 2^-24 on all three
MOMENTS_REL = 1e-12


# ---- the networks ------------------------------------------------------------------------------------------------------------------------
def split_params(dims, params):
    """[(W [out][in], b [out]), ...] of the flat state-dict order [W0, b0, W1, b1, ...] (policy.flatten_sequential)."""
    out, o = [], 0
    for l in range(len(dims) - 1):
        din, dout = dims[l], dims[l + 1]
        W = np.asarray(params[o:o + din * dout]).reshape(dout, din); o += din * dout
        b = np.asarray(params[o:o + dout]); o += dout
        out.append((W, b))
    assert o == len(params)
    return out


def _mlp(dims, params, x, dt, pre=None):
    a = np.asarray(x, dt).reshape(-1, dims[0])
    layers = split_params(dims, params)
    with np.errstate(all="ignore"):
        for l, (W, b) in enumerate(layers):
            v = a @ W.astype(dt).T + b.astype(dt)
            if pre is not None:
                pre.append(v)
            a = v if l == len(layers) - 1 else np.where(v > 0, v, np.expm1(v))
    return a


def mlp64(dims, params, x, pre=None):
    """y = mlp(x) in float64; `pre` (a list) receives every layer's pre-activations."""
    return _mlp(dims, params, x, np.float64, pre)


def mlp32_plain(dims, params, x):
    """The same net in float32, in numpy's own summation order: what a plain fp32 evaluation loses against float64."""
    return _mlp(dims, params, x, np.float32)


def mlp_yardstick(dims, params, x):
    """(y64, E32): E32 = max(max|mlp32_plain - mlp64|, 2^-24 max|mlp64|), a quantity of the reference alone."""
    y64 = mlp64(dims, params, x)
    e = float(np.abs(mlp32_plain(dims, params, x).astype(np.float64) - y64).max())
    return y64, max(e, U24 * float(np.abs(y64).max()))


# ---- Philox4x32-10 on uint64 arrays ---------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _LO = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on counter (c0..c3) and key (k0, k1); every word is a uint64 array holding a 32-bit value."""
    c = [np.asarray(v, np.uint64) & _LO for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _LO, (p0 >> _S32) ^ c[3] ^ k1, p0 & _LO]
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c


def u01(r):
    return (np.asarray(r, np.uint64) >> np.uint64(8)).astype(np.float64) * U24


def box_muller(r0, r1):
    """Two standard normals from two words: u in (0,1], v in [0,1)."""
    u, v = 1.0 - u01(r0), u01(r1)
    rad = np.sqrt(-2.0 * np.log(u))
    return rad * np.cos(2.0 * math.pi * v), rad * np.sin(2.0 * math.pi * v)


def noise64(B, A, seed, step):
    """n[B][A]: the header's stream -- key = (low, high) word of the seed, counter = (row, step, purpose 11, block); a block of four
    actions takes the four words of one counter in order, two Box-Muller pairs."""
    nblk = (A + 3) // 4
    row = np.arange(B, dtype=np.uint64)[:, None]
    blk = np.arange(nblk, dtype=np.uint64)[None, :]
    r = philox4x32(row, np.uint64(step), np.uint64(11), blk, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    n0, n1 = box_muller(r[0], r[1])
    n2, n3 = box_muller(r[2], r[3])
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(B, 4 * nblk)[:, :A]


# ---- Normal(mean, std) ------------------------------------------------------------------------------------------------------------------------
def act64(mean, std, n):
    return np.asarray(mean, np.float64) + np.asarray(std, np.float64) * n


def logprob64(actions, mean, std):
    """(Normal(mean, std).log_prob(actions).sum(-1), its yardstick sum_a(z^2/2 + |log std| + 0.919))."""
    std = np.asarray(std, np.float64)
    z = (np.asarray(actions, np.float64) - np.asarray(mean, np.float64)) / std
    return (-0.5 * z * z - np.log(std) - HALF_LOG_2PI).sum(-1), (0.5 * z * z + np.abs(np.log(std)) + HALF_LOG_2PI).sum(-1)


# ---- rollout returns ---------------------------------------------------------------------------------------------------------------------------
def gae64(rew, val, don, tmo, last, gamma, lam):
    """(returns, advantages, magnitude) [T][B]: PPO.process_env_step's time-out bootstrap + RolloutStorage.compute_returns in float64.  `magnitude`
    is the same recursion over absolute values: the size of the terms that were summed into returns[t] (and advantages[t])."""
    rew, val, last = (np.asarray(v, np.float64) for v in (rew, val, last))
    T, B = rew.shape
    mag_r = np.abs(rew)
    if tmo is not None:
        rew = rew + gamma * val * np.asarray(tmo, np.float64)
        mag_r = mag_r + gamma * np.abs(val * np.asarray(tmo, np.float64))
    ret, mag = np.zeros((T, B)), np.zeros((T, B))
    adv, madv = np.zeros(B), np.zeros(B)
    for t in reversed(range(T)):
        nv = last if t == T - 1 else val[t + 1]
        nt = 1.0 - np.asarray(don[t], np.float64)
        adv = rew[t] + nt * gamma * nv - val[t] + nt * gamma * lam * adv
        madv = mag_r[t] + nt * gamma * np.abs(nv) + np.abs(val[t]) + nt * gamma * lam * madv
        ret[t] = adv + val[t]
        mag[t] = madv + np.abs(val[t])
    return ret, ret - val, mag


def moments64(a):
    """(mean, unbiased variance, count), two passes."""
    a = np.asarray(a, np.float64).reshape(-1)
    m = math.fsum(a) / a.size
    d = a - m
    m2 = math.fsum(d * d) - math.fsum(d) ** 2 / a.size      # the second term corrects the rounding of m
    return m, m2 / max(a.size - 1, 1), a.size


def normalize64(a):
    """(advantages - mean) / (std + 1e-8), unbiased std; also (mean, std)."""
    m, var, _ = moments64(a)
    sd = math.sqrt(var)
    return (np.asarray(a, np.float64) - m) / (sd + 1e-8), m, sd
