"""The float64 reference of the policy step (tests/policy_ref.py) pinned to published definitions, then the two oracle builds run through the cases of
tests/policy_cases.py against it.  tests/test_policy_gpu.py runs the HIP library through the same cases."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import policy_cases as PC
import policy_ref as R


# ---- the reference against published definitions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [[7, 5, 3], [49, 80, 208, 12], [16, 512]])
def test_mlp64_matches_torch_double(dims):
    params = PC.make_net(dims, 3, 2.0)
    layers, o = [], 0
    for l in range(len(dims) - 1):
        lin = torch.nn.Linear(dims[l], dims[l + 1]).double()
        n = dims[l] * dims[l + 1]
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(params[o:o + n].reshape(dims[l + 1], dims[l]).astype(np.float64)))
            lin.bias.copy_(torch.from_numpy(params[o + n:o + n + dims[l + 1]].astype(np.float64)))
        o += n + dims[l + 1]
        layers += [lin] + ([torch.nn.ELU()] if l < len(dims) - 2 else [])
    x = 3.0 * np.random.default_rng(1).standard_normal((9, dims[0]))
    ref = torch.nn.Sequential(*layers)(torch.from_numpy(x)).detach().numpy()
    got = R.mlp64(dims, params, x)
    assert np.abs(got - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    assert np.abs(R.mlp32_plain(dims, params, x) - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32(*[np.uint64(c) for c in ctr], *key)
        assert tuple(int(g) for g in got) == want
    c = np.array([0, 0xffffffff, 0x243f6a88], np.uint64)                   # and as arrays: element i is the scalar answer
    got = R.philox4x32(c, c, c, c, 0, 0)
    assert int(got[0][0]) == 0x6627e8d5 and got[0].shape == (3,)


def _kolmogorov(z):
    z = np.sort(z.reshape(-1))
    cdf = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in z])
    i = np.arange(1, z.size + 1)
    return max((i / z.size - cdf).max(), (cdf - (i - 1) / z.size).max())


def test_noise64_is_standard_normal_and_independent():
    B, A = 12500, 16                                                      # 2e5 draws
    n = R.noise64(B, A, 5, 7)
    assert n.shape == (B, A) and np.all(np.isfinite(n))
    assert _kolmogorov(n) < 1.63 / math.sqrt(n.size)                      # the 1 % point of the Kolmogorov distance
    lim = 4.0 / math.sqrt(n.size)
    corr = lambda a, b: abs(float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]))
    assert corr(n[:-1], n[1:]) < lim                                      # neighbouring rows
    assert corr(n, R.noise64(B, A, 5, 8)) < lim                           # steps
    assert corr(n[:, :-4], n[:, 4:]) < lim                                # blocks of four actions
    assert corr(n[:, 0::2], n[:, 1::2]) < lim                             # the two normals of one Box-Muller pair
    assert corr(n, R.noise64(B, A, 6, 7)) < lim                           # seeds: low word
    assert corr(n, R.noise64(B, A, (9 << 32) | 5, 7)) < lim               # seeds: high word
    assert not np.array_equal(R.noise64(10, A, 5, 3)[9], R.noise64(10, A, 5, 9)[3])    # row and step are different words of the counter
    assert np.array_equal(R.noise64(B, 5, 5, 7), n[:, :5]) and np.array_equal(R.noise64(100, A, 5, 7), n[:100])
    u = R.u01(np.array([0, 255, 256, 0xffffffff], np.uint64))
    assert u[0] == 0 and u[1] == 0 and u[2] == 2.0 ** -24 and u[3] == 1 - 2.0 ** -24


def test_act64_logprob64_are_torch_normal():
    rng = np.random.default_rng(2)
    mean, std, n = rng.standard_normal((50, 12)), np.exp(rng.uniform(-6, 1.5, 12)), rng.standard_normal((50, 12))
    a = R.act64(mean, std, n)
    d = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(std).expand(50, 12))
    lp, unit = R.logprob64(a, mean, std)
    assert np.abs(lp - d.log_prob(torch.from_numpy(a)).sum(-1).numpy()).max() <= 1e-12 * unit.max()
    assert np.allclose((a - mean) / std, n, rtol=0, atol=1e-9)


def test_gae64_closed_forms():
    T, B, r, c, g, lam = 12, 3, 0.3, 0.7, 0.99, 0.95
    rew, val, last = np.full((T, B), r), np.full((T, B), c), np.full(B, c)
    don, tmo = np.zeros((T, B), np.uint8), np.zeros((T, B))
    delta, x = r + g * c - c, g * lam
    ret, adv, mag = R.gae64(rew, val, don, tmo, last, g, lam)
    geo = np.array([(1 - x ** (T - t)) / (1 - x) for t in range(T)])
    assert np.abs(adv - delta * geo[:, None]).max() < 1e-13 and np.abs(ret - adv - c).max() < 1e-15 and np.all(mag >= np.abs(ret))
    m = 7                                                                 # a reset in the middle: env 1 plain, env 2 with a time-out
    don[m, 1:] = 1; tmo[m, 2] = 1
    ret, adv, _ = R.gae64(rew, val, don, tmo, last, g, lam)
    assert np.abs(adv[:, 0] - delta * geo).max() < 1e-13
    for b, at_reset in ((1, r - c), (2, r + g * c - c)):
        want = [delta * (1 - x ** (T - t)) / (1 - x) if t > m else delta * (1 - x ** (m - t)) / (1 - x) + x ** (m - t) * at_reset for t in range(T)]
        assert np.abs(adv[:, b] - np.array(want)).max() < 1e-13
    assert np.array_equal(R.gae64(rew, val, don, None, last, g, lam)[0][:, 1], ret[:, 1])


def test_moments64_normalize64():
    a = (1000.0 + 0.01 * np.random.default_rng(3).standard_normal(300)).astype(np.float32)
    fr = [Fraction(float(v)) for v in a]
    mean = sum(fr) / len(fr)
    var = sum((v - mean) ** 2 for v in fr) / (len(fr) - 1)
    m, v, n = R.moments64(a)
    assert n == 300 and abs(m - float(mean)) <= 1e-15 * float(mean) and abs(v - float(var)) <= 1e-14 * float(var)
    t = torch.from_numpy(a).double()
    got, _, sd = R.normalize64(a)
    assert np.abs(got - ((t - t.mean()) / (t.std() + 1e-8)).numpy()).max() < 1e-8 and abs(sd - math.sqrt(float(var))) < 1e-15
    assert R.moments64(np.float32([2.5]))[1] == 0.0


# ---- the two oracle builds through the shared cases -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sides(oracle_strict_lib, oracle_fast_lib):
    return {"strict": PC.Side(oracle_strict_lib, False), "fast": PC.Side(oracle_fast_lib, False)}


BUILDS = ("strict", "fast")


def test_case_table_reaches_every_branch():
    """What the MLP case table is there for, asserted from ceil(width / 16)."""
    hidden = [w for dims, *_ in PC.MLP_CASES.values() for w in dims[1:-1]]
    last = [dims[-1] for dims, *_ in PC.MLP_CASES.values()]
    assert {PC.tiles(w) for w in hidden if PC.tile_group(w) == 2} >= {5, 7, 9, 11}
    assert {PC.tiles(w) for w in hidden if PC.tile_group(w) == 4} >= {13, 14, 15, 17, 25, 31, 32}
    assert all(PC.short_last_group(w) for w in hidden if PC.tiles(w) in (5, 7, 9, 11, 13, 14, 15, 17, 25, 31))
    assert {72, 200, 504, 512} <= set(hidden) and any(PC.tiles(w) < 4 for w in hidden)
    assert {dims[0] for dims, *_ in PC.MLP_CASES.values()} >= {1, 3, 15, 16, 17, 49, 511, 512}
    assert set(last) >= {1, 2, 12, 15, 16, 17, 33, 512} and any(PC.short_last_group(w) and w % 16 for w in last)
    assert {len(dims) - 1 for dims, *_ in PC.MLP_CASES.values()} == {1, 2, 3, 4, 5, 6}
    assert {rows for _, rows, *_ in PC.MLP_CASES.values()} == {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97}
    assert {(xs, ws) for _, _, xs, ws, *_ in PC.MLP_CASES.values()} == {(1, 1), (100, 1), (1, 3), (100, 3)}


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", sorted(PC.MLP_CASES))
def test_oracle_mlp_case(sides, build, name):
    PC.check_mlp(sides[build], name)


@pytest.mark.parametrize("build", BUILDS)
def test_oracle_mlp_edges(sides, build):
    PC.check_zero_rows(sides[build])
    PC.check_elu_edges(sides[build])
    for dims in PC.NONFINITE_NETS:
        PC.check_nonfinite(sides[build], dims)
    for dims, rows in PC.SUBNORMAL_NETS:
        PC.check_subnormal(sides[build], dims, rows)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", sorted(PC.FUSED_CASES))
def test_oracle_policy_act_unequal_nets(sides, build, name):
    PC.check_fused(sides[build], name)


@pytest.mark.parametrize("build", BUILDS)
def test_oracle_policy_act_paths(sides, build):
    PC.check_scratch_mean(sides[build])
    PC.check_deterministic(sides[build])


@pytest.mark.parametrize("B", PC.SAMPLE_ROWS)
@pytest.mark.parametrize("A", PC.SAMPLE_A)
def test_oracle_sampling_against_noise64(sides, A, B):
    outs = [PC.check_sampling(sides[b], A, B)[0] for b in BUILDS]          # both builds in one test: they share the reference's draws
    PC.assert_same_bits(outs[0], outs[1], "strict oracle")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("variant", PC.ROLLOUT_VARIANTS)
@pytest.mark.parametrize("T,B", PC.ROLLOUT_SHAPES)
def test_oracle_rollout_returns(sides, build, T, B, variant):
    PC.check_rollout(sides[build], T, B, variant)


@pytest.mark.parametrize("build", BUILDS)
def test_oracle_rollout_moments(sides, build):
    PC.check_offset_moments(sides[build])
    for c in (1.5, 0.1):
        PC.check_constant_advantages(sides[build], c)


@pytest.mark.parametrize("build", BUILDS)
def test_oracle_status_codes(sides, build):
    codes = PC.status_codes(sides[build])
    assert len(codes) >= 35 and all(rc == PC.BADARG for rc in codes.values()), {k: v for k, v in codes.items() if v != PC.BADARG}
