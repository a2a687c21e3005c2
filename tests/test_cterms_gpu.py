"""k_cterms_step on its own (include/go2sim_cterms.h) on the HIP library, on synthetic forces (tests/cterms_ref.py: random rows of 0 to 50 N, the
threshold's edges, NaN and infinity).

Counts: inside the float64 reference's admissible set (a link whose norm lies within 3u n of the threshold may count either way; at most 1 % of
link-rows) and equal to the float32 law in the kernel's order.  Stumble: within u (4 sum n + 10 pen64) of the float64 value and bit-equal to the
float32 law.  1, 63, 64, 65, 255 and 257 envs (lane and workgroup tails), the pool's SoA layout and a row-major [B][L][3] tensor, four masks."""
import ctypes

import numpy as np
import pytest
import torch

import cterms_ref as R
from go2_sim2real_locomotion_rl_amd import Go2SimError
from go2_sim2real_locomotion_rl_amd.contact_terms import ContactTerms
from go2_sim2real_locomotion_rl_amd.go2_env import _as_device_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NL = 14                                                                     # the model's links: the ground, then the robot's 13
SIZES = [1, 63, 64, 65, 255, 257]
BODY_SCALE, STUMBLE_SCALE = -2.0, -1.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """bit-equal, a NaN matching any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


@pytest.fixture(scope="module")
def table():
    """every kind of row, shared and left unchanged: edges, special values, random"""
    rows = np.concatenate([R.edge_rows(R.BODY_THRESHOLD, R.THIGHS)[0], R.special_rows(), R.edge_rows(R.STUMBLE_THRESHOLD, (R.NON_FEET[0], R.NON_FEET[-1]))[0],
                           R.random_rows(300, seed=11)])
    rows.setflags(write=False)
    return rows


def rows_for(table, n, offset=0):
    return table[(np.arange(n) * 7 + offset) % len(table)] if n > 1 else table[[60]]         # one env: a random row


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def lay_out(F, layout):
    """robot forces [n][13][3] -> (device tensor, strides) with the ground's link 0 in front: the pool's SoA [link * 3 + comp][n] or row-major [n][14][3]"""
    n = len(F)
    full = np.concatenate([np.full((n, 1, 3), 1.0e6, np.float32), F], axis=1)        # a loaded ground link: no mask may read it
    if layout == "soa":
        return dev(full.reshape(n, NL * 3).T.copy()), (n, 3 * n, 1)
    return dev(full), (1, 3, 3 * NL)


def handle(n, body=R.THIGHS, stumble=R.NON_FEET, body_scale=BODY_SCALE, stumble_scale=STUMBLE_SCALE, body_thr=R.BODY_THRESHOLD, stumble_thr=R.STUMBLE_THRESHOLD):
    return ContactTerms(n, body_mask=R.model_mask(body), stumble_mask=R.model_mask(stumble), body_contact_scale=body_scale, stumble_scale=stumble_scale,
                        body_contact_threshold=body_thr, stumble_threshold=stumble_thr, device=DEV)


def run(h, F, layout, rew0=None, reset=None, with_rew=True):
    cf, strides = lay_out(F, layout)
    rew = dev(np.zeros(len(F), np.float32) if rew0 is None else rew0)
    count = torch.full((len(F),), -7.0, device=DEV)
    h.step(cf, strides, None if reset is None else dev(np.asarray(reset, np.uint8)), rew if with_rew else None, count)
    torch.cuda.synchronize()
    return rew.cpu().numpy(), count.cpu().numpy()


def want_rew(rew0, count, pen, body_scale=BODY_SCALE, stumble_scale=STUMBLE_SCALE):
    """float32 numpy in the launch's order: body_contact, then stumble"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.asarray(rew0, np.float32)
        if body_scale:
            r = r + count * R.inc32(body_scale)
        if stumble_scale:
            r = r + pen * R.inc32(stumble_scale)
    return r.astype(np.float32)


@pytest.mark.parametrize("layout", ["soa", "row_major"])
@pytest.mark.parametrize("n", SIZES)
def test_counts_penalties_and_add_order(table, n, layout):
    F = rows_for(table, n, offset=n)
    rew0 = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    finite = np.isfinite(F).all((1, 2))
    for name, links in R.MASK_SETS.items():
        count32, pen32 = R.law32(F, links, links)
        rew, count = run(handle(n, links, links), F, layout, rew0)
        assert same(count, count32) and same(rew, want_rew(rew0, count32, pen32)), (name, n, layout)     # both scales on: body_contact then stumble
        lo, hi, amb = R.body_count_sets(F[finite], links, R.BODY_THRESHOLD)
        assert amb.mean() <= 0.01 and np.all((lo <= count[finite]) & (count[finite] <= hi))
        # inc = f32(50 * 0.02) = 1: the reward of a zero start is the penalty itself
        pen, _ = run(handle(n, links, links, body_scale=0.0, stumble_scale=50.0), F, layout)
        pen64, bound = R.stumble64(F[finite], links, R.STUMBLE_THRESHOLD)
        err = np.abs(pen[finite].astype(np.float64) - pen64)
        print(f"{name}, {n} envs, {layout}: stumble worst error / bound {np.max(err / np.maximum(bound, 1e-300)) if err.size else 0.0:.3f}")
        assert same(pen, pen32) and np.all(err <= bound)


def test_threshold_edges_and_threshold_zero(table):
    F, over = R.edge_rows(R.BODY_THRESHOLD, R.THIGHS)
    _, count = run(handle(len(F)), F, "soa")
    assert np.array_equal(count, over.astype(np.float32))                   # at the threshold 0, one float32 above it 1; x, y, z, both signs
    Fs, over_s = R.edge_rows(R.STUMBLE_THRESHOLD, (R.NON_FEET[0], R.NON_FEET[-1]))
    pen, _ = run(handle(len(Fs), body_scale=0.0, stumble_scale=50.0), Fs, "soa")
    step = np.nextafter(np.float32(5), np.float32(9)) - np.float32(5)
    assert np.array_equal(pen, np.where(over_s, step, np.float32(0)))
    Z = np.concatenate([R.random_rows(40, seed=3), np.zeros((1, 13, 3), np.float32)])
    rew, count = run(handle(len(Z), R.ALL_LINKS, R.ALL_LINKS, body_thr=0.0, stumble_thr=0.0), Z, "row_major")
    count32, pen32 = R.law32(Z, R.ALL_LINKS, R.ALL_LINKS, 0.0, 0.0)
    assert same(count, count32) and same(rew, want_rew(np.zeros(len(Z), np.float32), count32, pen32))
    assert np.array_equal(count, (R.norms64(Z) > 0).sum(1)) and count[-1] == 0 and rew[-1] == 0       # no force: not above a threshold of 0


def test_nan_and_infinity():
    F = R.special_rows()
    rew, count = run(handle(len(F)), F, "soa")
    assert count.tolist() == [0.0, 1.0, 1.0, 2.0, 0.0]                      # a NaN norm compares false, an infinite one true
    pen, _ = run(handle(len(F), body_scale=0.0, stumble_scale=50.0), F, "soa")
    assert np.isnan(pen[[0, 1, 4]]).all() and np.isposinf(pen[[2, 3]]).all()
    assert np.isnan(rew[[0, 1, 4]]).all() and np.isneginf(rew[[2, 3]]).all()
    only_body, _ = run(handle(len(F), stumble_scale=0.0), F, "soa")         # without stumble the NaN does not reach the reward
    assert same(only_body, want_rew(np.zeros(len(F), np.float32), count, None, stumble_scale=0.0))


def test_rew_null_leaves_the_sums(table):
    n = 65
    F = rows_for(table, n)
    h = handle(n)
    run(h, F, "soa", reset=np.zeros(n, np.uint8))
    before = [t.numpy().copy() for t in h.state()]
    _, count = run(h, F, "soa", reset=np.ones(n, np.uint8), with_rew=False)
    assert same(count, R.law32(F, R.THIGHS, R.NON_FEET)[0])                 # the count is written all the same
    assert all(np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32)) for a, b in zip(before, h.state())) and before[1].max() == 1


@pytest.mark.parametrize("scales", [(BODY_SCALE, STUMBLE_SCALE), (BODY_SCALE, 0.0), (0.0, STUMBLE_SCALE)])
def test_reset_hand_over_and_clear(table, scales):
    n, T = 70, 6
    finite = table[np.isfinite(table).all((1, 2))]
    flags = [np.zeros(n, np.uint8), np.zeros(n, np.uint8), (np.arange(n) % 3 == 0).astype(np.uint8), np.zeros(n, np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint8)]
    h, model = handle(n, body_scale=scales[0], stumble_scale=scales[1]), R.Episode(n)
    ep_dev = [_as_device_tensor(p, (n,), torch.float32, torch.device(DEV)) for p in h.ep_ptrs]
    assert h.incs == (float(R.inc32(scales[0])), float(R.inc32(scales[1]))) and h.active == (scales[0] != 0, scales[1] != 0)
    rew = np.zeros(n, np.float32)
    for t in range(T):
        F = finite[(np.arange(n) * 5 + 31 * t) % len(finite)]
        count32, pen32 = R.law32(F, R.THIGHS, R.NON_FEET)
        terms = {k: v for k, v in ((0, count32 * R.inc32(scales[0])), (1, pen32 * R.inc32(scales[1]))) if scales[k] != 0}
        want = model.step(rew, terms, flags[t])
        rew, _ = run(h, F, "soa", rew, flags[t])
        assert same(rew, want)
        s, k, e = (x.numpy() for x in h.state())
        assert np.array_equal(bits(s), bits(model.sum)) and np.array_equal(k, model.steps) and np.array_equal(bits(e), bits(model.ep)), t
        assert all(np.array_equal(bits(ep_dev[i].cpu().numpy()), bits(model.ep[i])) for i in range(2))
    assert model.steps.max() == 1 and (model.ep != 0).any()
    idx = np.array([3, 99, -1, 7, n, 68], np.int32)                         # entries outside [0, n) are passed over
    h.clear(dev(idx))
    model.clear([3, 7, 68])
    s, k, e = (x.numpy() for x in h.state())
    assert np.array_equal(bits(s), bits(model.sum)) and np.array_equal(k, model.steps) and np.array_equal(bits(e), bits(model.ep))
    assert k[:, 3].tolist() == [0, 0] and k[:, 4].tolist() == [int(scales[0] != 0), int(scales[1] != 0)]
    h.clear()
    model.clear(range(n))
    s, k, e = (x.numpy() for x in h.state())
    assert not s.any() and not k.any() and np.array_equal(bits(e), bits(model.ep))


def test_state_round_trip_to_the_bit():
    n = 257
    rng = np.random.default_rng(5)
    s = rng.integers(0, 2 ** 32, (2, n), dtype=np.uint64).astype(np.uint32).view(np.float32)       # any bit pattern, NaN payloads included
    e = rng.integers(0, 2 ** 32, (2, n), dtype=np.uint64).astype(np.uint32).view(np.float32)
    k = rng.integers(-2 ** 31, 2 ** 31, (2, n), dtype=np.int64).astype(np.int32)
    h = handle(n)
    h.set_state(torch.from_numpy(s), torch.from_numpy(k), torch.from_numpy(e))
    s2, k2, e2 = h.state()
    assert np.array_equal(s2.numpy().view(np.uint32), s.view(np.uint32)) and np.array_equal(k2.numpy(), k) and np.array_equal(e2.numpy().view(np.uint32), e.view(np.uint32))
    with pytest.raises(Go2SimError, match="shape"):
        h.set_state(torch.zeros(2, n - 1), torch.zeros(2, n - 1, dtype=torch.int32), torch.zeros(2, n - 1))


def test_replayed_calls_and_two_streams_give_equal_bits(table):
    n = 257
    F = rows_for(table, n, offset=2)
    cf, strides = lay_out(F, "soa")
    rew0 = dev(np.random.default_rng(1).standard_normal(n).astype(np.float32))
    reset = dev((np.arange(n) % 4 == 1).astype(np.uint8))
    start = [torch.full((2, n), 0.25), torch.full((2, n), 3, dtype=torch.int32), torch.zeros(2, n)]

    def once(h):
        h.set_state(*start)
        rew, count = rew0.clone(), torch.zeros(n, device=DEV)
        h.step(cf, strides, reset, rew, count)
        return [rew.cpu().numpy().view(np.uint32), count.cpu().numpy().view(np.uint32)] + [x.numpy().view(np.uint32) for x in h.state()]

    h = handle(n)
    first = once(h)
    for _ in range(49):
        assert all(np.array_equal(a, b) for a, b in zip(first, once(h)))
    for _ in range(2):                                                      # two streams of their own, a handle each
        with torch.cuda.stream(torch.cuda.Stream(DEV)):
            assert all(np.array_equal(a, b) for a, b in zip(first, once(handle(n))))


def test_bad_arguments_launch_nothing(table):
    n = 64
    F = rows_for(table, n)
    h = handle(n)
    cf, strides = lay_out(F, "soa")
    rew, count = torch.full((n,), 2.5, device=DEV), torch.full((n,), -7.0, device=DEV)
    before = [t.numpy().copy() for t in h.state()]
    for bad in ((-1, 3 * n, 1), (n, -1, 1), (n, 3 * n, -1)):
        with pytest.raises(Go2SimError):
            h.step(cf, bad, None, rew, count)
    with pytest.raises(Go2SimError):
        h.step(None, strides, None, rew, count)
    L = h._L
    for hh, nn in ((ctypes.c_void_p(0), n), (h.h, n - 1), (h.h, n + 1)):
        rc = L.fn("cterms_step")(hh, ctypes.c_int(nn), ctypes.c_void_p(cf.data_ptr()), ctypes.c_longlong(n), ctypes.c_longlong(3 * n), ctypes.c_longlong(1),
                                 None, ctypes.c_void_p(rew.data_ptr()), ctypes.c_void_p(count.data_ptr()), None)
        assert rc == -1
    torch.cuda.synchronize()
    assert (rew == 2.5).all() and (count == -7.0).all()
    assert all(np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32)) for a, b in zip(before, h.state()))
    for kw in (dict(body_mask=1 << NL), dict(stumble_mask=1 << 31), dict(dt=0.0), dict(n_links=33)):
        with pytest.raises(Go2SimError):
            ContactTerms(n, **{"body_mask": 0xC0, "stumble_mask": 0x3FE, **kw}, device=DEV)
