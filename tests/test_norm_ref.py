"""The two references of the empirical observation normaliser (tests/norm_ref.py) against each other, on the CPU: the numpy float64 law and the literal
torch restatement of rsl_rl 2.2.4's module agree over the case table to float32 rounding; Chan's merge of shards gives the whole batch's moments to float64
rounding; the first update from the initial state gives the batch's own mean and biased variance."""
import numpy as np
import pytest
import torch

import norm_cases as NC
import norm_ref as R

CHUNK = 256          # the table's row chunk; tests/test_norm_capi.py checks it is the header's


def torch_state(m):
    sd = m.state_dict()
    return {"mean": sd["_mean"].reshape(-1).numpy().copy(), "var": sd["_var"].reshape(-1).numpy().copy(), "std": sd["_std"].reshape(-1).numpy().copy(),
            "count": int(sd["count"])}


@pytest.mark.parametrize("case", NC.cases(CHUNK), ids=lambda c: f"{c[0]}-d{c[1]}-{len(c[2])}")
def test_references_agree_to_float32_rounding(case):
    """One step at a time from the torch module's own float32 state: the float64 law lands within norm_ref.state_bounds with the float32 unit roundoff
    (the module sums n float32 terms), and the module's output within output_bound."""
    name, d, ns = case
    m = R.TorchEmpiricalNormalization([d], eps=R.EPS, until=1e8)
    worst = {}
    for k, n in enumerate(ns):
        x = NC.case_data(name, d, n, k)
        prior = torch_state(m)
        y = m(torch.from_numpy(x)).numpy()
        new = torch_state(m)
        new64 = R.update(prior, x)
        assert new["count"] == new64["count"] == prior["count"] + n
        tol = R.state_bounds(prior, x, new64, u=R.U32, std_of_stored_var=True)
        for key in ("mean", "var", "std"):
            worst[key] = max(worst.get(key, 0.0), float((np.abs(new[key] - new64[key]) / tol[key]).max()))
        y64 = R.normalize(new64, x)
        ytol = R.output_bound(new64, x, y64, tol["mean"], tol["std"])
        worst["y"] = max(worst.get("y", 0.0), float((np.abs(y - y64) / ytol).max()))
    print(f"torch restatement vs float64 law, {name} d={d}: worst ratio " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("d,n,cuts", [(49, 4096, (2048,)), (104, 775, (1, 300)), (3, 65, (64,)), (257, 1024, (256, 512, 768)), (1, 7, (3, 3))])
def test_merged_shards_give_the_whole_batch_moments(d, n, cuts):
    """Chan's fold of the shards' two-pass moments against the whole batch's, to float64 rounding: the bounds are norm_ref.state_bounds' E_mean and the
    variance's sum terms, times n for M2.  An empty shard (a repeated cut) is passed over."""
    x = NC.case_data("seq-const-tiny-offset", d, n, 0)
    edges = [0, *cuts, n]
    acc = (0.0, np.zeros(d), np.zeros(d))
    for lo, hi in zip(edges[:-1], edges[1:]):
        acc = R.merge(acc, R.moments(x[lo:hi]) if hi > lo else (0.0, np.zeros(d), np.zeros(d)))
    nw, mw, qw = R.moments(x)
    assert acc[0] == nw == n
    x64 = x.astype(np.float64)
    A, D = np.abs(x64).max(axis=0), np.abs(x64 - mw).max(axis=0)
    k = R.C_SUM * (n + 16) * R.U64
    e_mean = k * A
    e_m2 = n * (2.0 * D * e_mean + k * D * D) + R.TINY32
    print(f"merge d={d} n={n} cuts={cuts}: mean {float((np.abs(acc[1] - mw) / (e_mean + R.TINY32)).max()):.4f}, M2 {float((np.abs(acc[2] - qw) / e_m2).max()):.4f} of the bound")
    assert np.all(np.abs(acc[1] - mw) <= e_mean + R.TINY32) and np.all(np.abs(acc[2] - qw) <= e_m2)


@pytest.mark.parametrize("d,n", [(49, 64), (104, 4096), (1, 1), (3, 2)])
def test_first_update_gives_the_batch_moments(d, n):
    x = NC.case_data("seq-const-tiny-offset", d, n, 0)
    new = R.update(R.initial_state(d), x)
    _, mean_b, m2 = R.moments(x)
    var_b = m2 / n
    assert new["count"] == n
    assert np.array_equal(new["mean"], mean_b)                                    # rate = 1: 0 + 1 (mean_b - 0)
    assert np.all(np.abs(new["var"] - var_b) <= 4 * R.U64 * np.maximum(1.0, var_b))      # 1 + (var_b - 1 + 0): two roundings at size max(1, var_b)
    assert np.all(np.abs(new["std"] ** 2 - new["var"]) <= 4 * R.U64 * new["var"])
    if n == 1:
        assert np.all(new["var"] == 0.0) and np.all(new["std"] == 0.0)
    m = R.TorchEmpiricalNormalization([d])
    m.update(torch.from_numpy(x))
    tol = R.state_bounds(R.initial_state(d), x, new, u=R.U32)
    assert np.all(np.abs(m.mean.numpy() - mean_b) <= tol["mean"]) and int(m.count) == n


def test_until_counts_the_crossing_batch_whole():
    s = R.initial_state(3)
    x = NC.case_data("single", 3, 10, 0)
    s1 = R.rounded(R.update(s, x, until=15))
    s2 = R.rounded(R.update(s1, x, until=15))
    s3 = R.update(s2, x, until=15)
    assert (s1["count"], s2["count"], s3["count"]) == (10, 20, 20)
    assert np.array_equal(s3["mean"], s2["mean"].astype(np.float64))
    m = R.TorchEmpiricalNormalization([3], until=15)
    for _ in range(3):
        m.update(torch.from_numpy(x))
    assert int(m.count) == 20
