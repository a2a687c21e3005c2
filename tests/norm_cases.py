"""The case table of the empirical observation normaliser and the checks every case goes through (tests/test_norm_gpu.py on the HIP library; the table
also feeds tests/test_norm_ref.py, which compares the two references of tests/norm_ref.py on the CPU).

A case is (name, d, [n_rows of every update in turn]).  `check_case` steps a handle through the updates; before each call it reads the device's float32
state, computes the reference step from exactly that state, and asserts the new state and the output against norm_ref's derived bounds, printing the worst
ratio to the bound first.  It returns the final state's arrays for the bit comparisons between handles."""
import ctypes

import numpy as np

import norm_ref as R

D_ALL = (1, 3, 45, 49, 104, 178, 257)


def n_rows_all(chunk):
    return (1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7, 4096)


def case_data(name, d, n, k):
    """float32 [n][d] of update k of a case: columns of unequal location and scale, and the special columns the name announces"""
    rng = np.random.default_rng(1000003 * d + 7919 * n + 31 * k + sum(map(ord, name)))
    loc = rng.uniform(-3.0, 3.0, d)
    scale = np.exp(rng.uniform(-2.0, 2.0, d))
    x = loc + scale * rng.standard_normal((n, d))
    if "const" in name:
        x[:, 0] = 2.5                                        # a constant column
    if "tiny" in name:
        x[:, d // 2] = rng.choice([0.0, 1.0e-42, -3.0e-41, 1.0e-39], n)     # zeros and float32 denormals
    if "offset" in name:
        x[:, d - 1] = 1.0e4 + rng.standard_normal(n)         # mean 1e4, unit spread: sum x^2 - n mean^2 loses it
    return np.ascontiguousarray(x.astype(np.float32))


def cases(chunk):
    """every d with every n_rows as one update from the initial state, then sequences of at least 4 updates with changing n_rows and the special columns"""
    out = [(f"single-d{d}-n{n}", d, [n]) for d in D_ALL for n in n_rows_all(chunk)]
    out += [("seq-const-tiny-offset", 49, [64, 1, chunk + 1, 7, 3 * chunk + 7]), ("seq-const-tiny-offset", 104, [4096, 63, 2, chunk]),
            ("seq-const-tiny-offset", 3, [1, 1, 2, 65, chunk - 1]), ("seq-offset", 1, [5, 4096, 1, 64]),
            ("seq-const-tiny-offset", 257, [65, chunk, 2, 3 * chunk + 7]), ("seq-const-tiny-offset", 45, [2, 63, 4096, 1]),
            ("seq-const-tiny-offset", 178, [chunk + 1, 1, 64, 4096])]
    return out


# ---- one handle of the product library -------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


class Side:
    """a go2sim_norm handle on the raw C ABI; device tensors are torch's"""

    def __init__(self, lib, d, eps=R.EPS, until=1e8, device="cuda:0"):
        import torch

        self.L, self.d, self.eps, self.until, self.dev, self.torch = lib, d, eps, until, device, torch
        h = ctypes.c_void_p()
        lib.check(lib.fn("norm_create")(ctypes.c_int(0), ctypes.c_int(d), ctypes.c_double(eps), ctypes.c_double(until), ctypes.byref(h)), "norm_create")
        self.h = h

    def close(self):
        if self.h:
            self.L.fn("norm_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def get_state(self):
        mean, var, std = (np.empty(self.d, np.float32) for _ in range(3))
        cnt = ctypes.c_int64()
        self.L.check(self.L.fn("norm_get_state")(self.h, mean.ctypes.data_as(ctypes.c_void_p), var.ctypes.data_as(ctypes.c_void_p),
                                                 std.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt), self.stream()), "norm_get_state")
        return {"mean": mean, "var": var, "std": std, "count": cnt.value}

    def set_state(self, s):
        arrs = [np.ascontiguousarray(s[k], np.float32) for k in ("mean", "var", "std")]
        self.L.check(self.L.fn("norm_set_state")(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in arrs), ctypes.c_int64(int(s["count"])), self.stream()),
                     "norm_set_state")

    def device_x(self, x, misalign=False):
        """x on the device; misalign: a view that starts 4 bytes past a 16-byte boundary"""
        t = self.torch
        x = np.ascontiguousarray(x, np.float32)
        if not misalign:
            return t.from_numpy(x).to(self.dev)
        buf = t.empty(x.size + 8, dtype=t.float32, device=self.dev)
        off = ((16 - buf.data_ptr() % 16) % 16) // 4 + 1
        v = buf[off:off + x.size].view(x.shape)
        v.copy_(t.from_numpy(x))
        assert v.data_ptr() % 16 == 4
        return v

    def step(self, x_dev, update=True, other=None, x_other=None):
        """go2sim_norm_step; -> y (and the other normaliser's y) as numpy"""
        t = self.torch
        n = x_dev.shape[0]
        y = t.full((n, self.d), float("nan"), device=self.dev)
        yo = t.full((n, other.d), float("nan"), device=self.dev) if other is not None else None
        self.L.check(self.L.fn("norm_step")(self.h, _p(x_dev), _p(y), other.h if other is not None else None, _p(x_other), _p(yo), ctypes.c_int(n),
                                            ctypes.c_int(int(update)), self.stream()), "norm_step")
        return (y.cpu().numpy(), yo.cpu().numpy()) if other is not None else y.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(s1, s2):
    return s1["count"] == s2["count"] and all(np.array_equal(bits(s1[k]), bits(s2[k])) for k in ("mean", "var", "std"))


def check_step(prior, x, new_dev, y_dev, until=1e8, ref64=None):
    """One counted (or refused by `until`) step from the device's own prior float32 state: asserts state and output against the derived bounds.
    ref64: the reference's new state when it does not come from the whole batch's two-pass moments (the sharded path).  -> worst ratios."""
    new64 = R.update(prior, x, until=until) if ref64 is None else ref64
    assert new_dev["count"] == new64["count"], (new_dev["count"], new64["count"])
    worst = {}
    if new64["count"] == prior["count"]:                      # not counted: the state's bits stay
        assert same_bits(prior, new_dev)
        tol = {k: np.zeros(len(prior["mean"])) for k in ("mean", "var", "std")}
    else:
        tol = R.state_bounds(prior, x, new64)
        for k in ("mean", "var", "std"):
            fin = np.isfinite(new64[k])
            assert np.array_equal(np.isfinite(new_dev[k]), fin), (k, "finite columns differ")
            err = np.abs(new_dev[k].astype(np.float64) - new64[k])[fin]
            worst[k] = float((err / tol[k][fin]).max()) if fin.any() else 0.0
    y64 = R.normalize(new64, x)
    fin = np.isfinite(y64)
    assert np.array_equal(np.isfinite(y_dev), fin), "finite outputs differ"
    ytol = R.output_bound(new64, x, y64, tol["mean"], tol["std"])
    worst["y"] = float((np.abs(y_dev.astype(np.float64) - y64)[fin] / ytol[fin]).max()) if fin.any() else 0.0
    return worst


def check_case(lib, case, misalign=False):
    """-> (final state, [y of every update], worst ratios)"""
    name, d, ns = case
    side = Side(lib, d)
    worst, ys = {}, []
    for k, n in enumerate(ns):
        x = case_data(name, d, n, k)
        prior = side.get_state()
        y = side.step(side.device_x(x, misalign))
        new = side.get_state()
        w = check_step(prior, x, new, y)
        for key, v in w.items():
            worst[key] = max(worst.get(key, 0.0), v)
        ys.append(y)
    final = side.get_state()
    side.close()
    print(f"norm {name} d={d} n={ns}{' misaligned' if misalign else ''}: worst ratio to the bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    return final, ys, worst
