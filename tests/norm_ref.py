"""References of the empirical observation normaliser (include/go2sim_norm.h) and the bounds its tests assert.

Two references:
  * numpy float64: `update` (the law of the header from a float32 state, the batch moments two-pass over the whole batch, nothing rounded to float32),
    `normalize`, `merge` (Chan's pairwise formula) and `moments`;
  * `TorchEmpiricalNormalization`: a literal torch-CPU restatement of rsl_rl 2.2.4's module (float32 buffers, torch.var / torch.mean, in-place updates).

Bounds.  u32 = 2^-24 and u64 = 2^-53 are the unit roundoffs.  All bounds are per column and derived below from the formats and the operation counts; none is
a measured figure.  The tests compare ONE step at a time: the reference starts from the float32 state the device held before the call, so no bound has to
carry the history of earlier roundings.
"""
import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY32 = 2.0 ** -149                      # a float32 result below 2^-126 is rounded to this spacing instead of relatively
EPS = 1e-2

# C_SUM: the device's float64 moments are sums of n terms taken in another order than numpy's (lanes, chunks of 256 rows, the fold of the chunk moments), the reference's own
# pairwise sum has an error of its own, and the law adds about a dozen float64 operations.  Each n-term sum is within (n - 1) u64 sum|terms| of the exact
# one whatever its order (Higham, Accuracy and Stability, eq. 4.4), so two of them differ by at most 2 (n - 1) u64 sum|terms|; the chunk fold adds three
# products, three additions and a subtraction per chunk, i.e. < 8 roundings per chunk of 256 rows = n / 32 more; the law's own operations are the "+ 16".
# 2 (n - 1) + n / 32 + 16 < C_SUM (n + 16) with C_SUM = 4 leaves a factor of almost two for the terms' own roundings (the squares, the centring).
C_SUM = 4.0


def initial_state(d):
    return {"mean": np.zeros(d, np.float32), "var": np.ones(d, np.float32), "std": np.ones(d, np.float32), "count": 0}


def moments(x):
    """(n, mean_b[d], M2_b[d]) in float64, two passes over the whole batch"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    return float(x.shape[0]), mean, ((x - mean) ** 2).sum(axis=0)


def merge(a, b):
    """Chan et al.: the moments of the union of two sets from theirs; an empty set is passed over"""
    (na, ma, qa), (nb, mb, qb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    delta = mb - ma
    return n, ma + delta * (nb / n), qa + qb + delta * delta * (na * nb / n)


def update_from_moments(state, n, mean_b, M2_b, until=1e8):
    """The law in float64 from the float32 state; -> the new state in float64 (NOT rounded: the bounds below include the one float32 rounding)."""
    m, v, cnt = state["mean"].astype(np.float64), state["var"].astype(np.float64), int(state["count"])
    if n == 0 or (until is not None and until > 0 and cnt >= until):
        return {"mean": m, "var": v, "std": state["std"].astype(np.float64), "count": cnt}
    cnt1 = cnt + int(n)
    rate = n / cnt1
    dm = mean_b - m
    m1 = m + rate * dm
    with np.errstate(invalid="ignore"):
        v1 = v + rate * (M2_b / n - v + dm * (mean_b - m1))
        v1 = np.where(v1 < 0.0, 0.0, v1)                    # a NaN stays a NaN
        return {"mean": m1, "var": v1, "std": np.sqrt(v1), "count": cnt1}


def update(state, x, until=1e8):
    return update_from_moments(state, *moments(x), until=until)


def rounded(state64):
    """the float32 state a float64 result is stored as"""
    return {"mean": state64["mean"].astype(np.float32), "var": state64["var"].astype(np.float32), "std": state64["std"].astype(np.float32),
            "count": state64["count"]}


def normalize(state, x, eps=EPS):
    """(x - mean) / (std + eps) in float64; eps is the float32 the library holds"""
    return (np.asarray(x, np.float64) - state["mean"].astype(np.float64)) / (state["std"].astype(np.float64) + float(np.float32(eps)))


def state_bounds(state, x, new64, u=U64, std_of_stored_var=False):
    """Per-column bounds on |device float32 state - new64| after one counted update of `state` (float32) with the batch x.  `u` is the unit roundoff of the
    arithmetic under test: u64 for the library; u32 gives the same bounds for an implementation that sums in float32 (the torch restatement).

    mean':  one float32 rounding, u32 |mean'|, plus the float64 error.  mean_b is a sum of n terms of size <= A = max|x| divided by n: within
            C_SUM (n + 16) u64 A, and mean' = m + rate (mean_b - m) with rate <= 1 passes that on undiminished at worst, with roundings of size u64 max(A, |m|):
                E_mean = C_SUM (n + 16) u64 S,   S = max(A, |m|)
    var':   one float32 rounding, u32 var', plus the float64 error of  v + rate (M2 / n - v + dm (mean_b - mean')):
              - M2 / n is a mean of n squares (x - mean_b)^2 <= D^2, D = max|x - mean_b|: its sum contributes C_SUM (n + 16) u64 D^2, and the error of the
                centre moves every term by at most 2 D E_mean (the exact first-order cancellation of a two-pass sum is not claimed);
              - dm (mean_b - mean') with |dm| = G, |mean_b - mean'| <= G: each factor is off by at most 2 E_mean, so the product by 4 G E_mean, plus
                roundings of size u64 G^2;  the outer additions round at size u64 max(v, var_b, G^2)
                E_var = 2 (D + 2 G) E_mean + C_SUM (n + 16) u64 (D^2 + G^2 + v)
            The form sum x^2 - n mean^2 has an error of size n u64 A^2 instead and fails this bound as soon as A >> D.
    std':   sqrt is monotone: a var' within E_var of the reference moves sqrt by at most the larger of sqrt(var') - sqrt(max(var' - E_var, 0)) and
            sqrt(var' + E_var) - sqrt(var') (the first unless var' < E_var clips it); then one float32 rounding, u32 std', and the square root's own rounding, u std'.
            rsl_rl takes sqrt of the STORED float32 var' where the library takes it of the float64 one (std_of_stored_var): then var's float32 rounding,
            u32 var' + 2^-149, joins E_var under the root.
    Denormal results are rounded absolutely: + 2^-149 on each bound.  Columns whose reference is not finite are compared for being non-finite too.
    """
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    m, v = state["mean"].astype(np.float64), state["var"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean_b = x.mean(axis=0)
        A = np.abs(x).max(axis=0)
        D = np.abs(x - mean_b).max(axis=0)
        G = np.abs(mean_b - m)
        S = np.maximum(A, np.abs(m))
        k = C_SUM * (n + 16) * u
        e_mean = k * S
        e_var = 2.0 * (D + 2.0 * G) * e_mean + k * (D * D + G * G + v)
        root = np.sqrt(new64["var"])
        e_root = e_var + (U32 * np.abs(new64["var"]) + TINY32 if std_of_stored_var else 0.0)
        e_std = np.maximum(root - np.sqrt(np.maximum(new64["var"] - e_root, 0.0)), np.sqrt(new64["var"] + e_root) - root) + u * new64["std"]
        return {"mean": U32 * np.abs(new64["mean"]) + e_mean + TINY32, "var": U32 * np.abs(new64["var"]) + e_var + TINY32,
                "std": U32 * np.abs(new64["std"]) + e_std + TINY32}


def output_bound(ref_state, x, y_ref, tol_mean, tol_std, eps=EPS):
    """Bound on |device y - y_ref| for y = (x - mean) / (std + eps) in float32 operations, the device's float32 mean and std being within tol_mean / tol_std of
    the reference's (zero for a state both sides hold exactly).  With a = std + eps and t_a = tol_std + u32 a (the float32 addition std + eps):
      numerator:    |(x - mean)_dev - (x - mean)| <= tol_mean + u32 |x - mean_dev|        (one float32 subtraction)
      denominator:  a_dev >= a - t_a
      quotient:     |num_dev / a_dev - num / a| <= (tol_mean + u32 (|x - mean| + tol_mean)) / (a - t_a) + |y_ref| t_a / (a - t_a), then one correctly rounded
                    division, u32 |y_dev| <= u32 (|y_ref| + the above); a denormal result adds 2^-149."""
    a = ref_state["std"].astype(np.float64) + float(np.float32(eps))
    t_a = tol_std + U32 * a
    num = np.abs(np.asarray(x, np.float64) - ref_state["mean"].astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = (tol_mean + U32 * (num + tol_mean)) / (a - t_a) + np.abs(y_ref) * t_a / (a - t_a)
        return e + U32 * (np.abs(y_ref) + e) + TINY32


class TorchEmpiricalNormalization:
    """rsl_rl 2.2.4 ``modules/normalizer.py`` EmpiricalNormalization, restated literally for torch on the CPU (buffers as attributes instead of nn.Module's)."""

    def __init__(self, shape, eps=1e-2, until=None):
        self.eps, self.until, self.training = eps, until, True
        self._mean = torch.zeros(shape).unsqueeze(0)
        self._var = torch.ones(shape).unsqueeze(0)
        self._std = torch.ones(shape).unsqueeze(0)
        self.count = torch.tensor(0, dtype=torch.long)

    @property
    def mean(self):
        return self._mean.squeeze(0).clone()

    @property
    def std(self):
        return self._std.squeeze(0).clone()

    def forward(self, x):
        if self.training:
            self.update(x)
        return (x - self._mean) / (self._std + self.eps)

    __call__ = forward

    def update(self, x):
        if self.until is not None and self.count >= self.until:
            return
        count_x = x.shape[0]
        self.count += count_x
        rate = count_x / self.count
        var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(x, dim=0, keepdim=True)
        delta_mean = mean_x - self._mean
        self._mean += rate * delta_mean
        self._var += rate * (var_x - self._var + delta_mean * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)

    def inverse(self, y):
        return y * (self._std + self.eps) + self._mean

    def state_dict(self):
        return {"_mean": self._mean.clone(), "_var": self._var.clone(), "_std": self._std.clone(), "count": self.count.clone()}
