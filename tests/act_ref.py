"""Float64 reference of the hidden-layer activations (include/go2sim_activation.h), in plain numpy.  It imports nothing of the project: the seven
functions are the torch modules rsl_rl's resolve_nn_activation maps the names to (tests/test_act_ref.py holds them to torch in float64), the
derivatives are written as functions of the post-activation, as the update computes them, and the networks are those of tests/policy_ref.py with the
activation as an argument.

BOUND_ABS / BOUND_REL are the element-wise bounds the header derives (u = 2^-24): |a_hip - act64(v)| <= BOUND_ABS + BOUND_REL |act64(v)|, plus 2^-149
(the spacing of float32's subnormals) where the bound is a relative one: a product that lands below 2^-126 is rounded to that grid.  They are derived
numbers, not measured ones: dm_exp's tested 2 ulp plus the roundings of each form's own operations."""
import numpy as np

U24 = 2.0 ** -24
NAMES = ("elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "identity")
SELU_L, SELU_A = 1.0507009873554805, 1.6732632423543772
LRELU_SLOPE = 0.01
BOUND_ABS = {"elu": 4 * U24, "selu": 10 * U24, "relu": 0.0, "lrelu": 0.0, "tanh": 5 * U24, "sigmoid": 3 * U24, "identity": 0.0}
BOUND_REL = {"elu": 0.0, "selu": 2 * U24, "relu": 0.0, "lrelu": 2 * U24, "tanh": 0.0, "sigmoid": 0.0, "identity": 0.0}
PIECEWISE = ("elu", "selu", "relu", "lrelu")                 # a branch at v = 0
JUMP = ("selu", "relu", "lrelu")                            # ... whose derivative jumps there
SATURATING = ("tanh", "sigmoid")


def act64(name, v):
    """The activation in the dtype of v (float64 for the reference, float32 for the yardstick)."""
    v = np.asarray(v)
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        if name == "elu":
            return np.where(v > 0, v, np.expm1(v))
        if name == "selu":
            return np.where(v > 0, dt(SELU_L) * v, dt(SELU_L * SELU_A) * np.expm1(v))
        if name == "relu":
            return np.where(v < 0, dt(0), v)                 # NaN stays NaN
        if name == "lrelu":
            return np.where(v > 0, v, dt(LRELU_SLOPE) * v)
        if name == "tanh":
            return np.tanh(v)
        if name == "sigmoid":
            e = np.exp(-np.abs(v))
            return np.where(v >= 0, 1 / (1 + e), e / (1 + e))             # exp(-|v|) <= 1: no overflow; a NaN reaches both arms
        if name == "identity":
            return v + 0
    raise KeyError(name)


def dact64_from_a(name, a):
    """d activation / d pre-activation as a function of the post-activation a"""
    a = np.asarray(a)
    dt = a.dtype.type
    one = np.ones_like(a)
    if name == "elu":
        return np.where(a > 0, one, a + 1)
    if name == "selu":
        return np.where(a > 0, dt(SELU_L) * one, a + dt(SELU_L * SELU_A))
    if name == "relu":
        return np.where(a > 0, one, 0 * one)
    if name == "lrelu":
        return np.where(a > 0, one, dt(LRELU_SLOPE) * one)
    if name == "tanh":
        return 1 - a * a
    if name == "sigmoid":
        return a * (1 - a)
    if name == "identity":
        return one
    raise KeyError(name)


def bound(name, v):
    """The header's element-wise bound at the float32 pre-activations v; infinite where float64 is not finite (only the pattern is compared there)"""
    a = np.abs(act64(name, np.asarray(v, np.float64)))
    fin = np.isfinite(a)
    return np.where(fin, BOUND_ABS[name] + BOUND_REL[name] * np.where(fin, a, 0.0) + (2.0 ** -149 if BOUND_REL[name] else 0.0), np.inf)


# ---- the networks (tests/policy_ref.py's, with the activation as an argument) -----------------------------------------------------------------
def split_params(dims, params):
    out, o = [], 0
    for l in range(len(dims) - 1):
        din, dout = dims[l], dims[l + 1]
        W = np.asarray(params[o:o + din * dout]).reshape(dout, din); o += din * dout
        b = np.asarray(params[o:o + dout]); o += dout
        out.append((W, b))
    assert o == len(params)
    return out


def _mlp(name, dims, params, x, dt, pre=None):
    a = np.asarray(x, dt).reshape(-1, dims[0])
    layers = split_params(dims, params)
    with np.errstate(all="ignore"):
        for l, (W, b) in enumerate(layers):
            v = a @ W.astype(dt).T + b.astype(dt)
            if pre is not None:
                pre.append(v)
            a = v if l == len(layers) - 1 else act64(name, v)
    return a


def mlp64(name, dims, params, x, pre=None):
    """y = mlp(x) in float64; `pre` (a list) receives every layer's pre-activations."""
    return _mlp(name, dims, params, x, np.float64, pre)


def mlp32_plain(name, dims, params, x):
    """The same net in float32, in numpy's own summation order: what a plain fp32 evaluation loses against float64."""
    return _mlp(name, dims, params, x, np.float32)


def mlp_yardstick(name, dims, params, x):
    """(y64, E32): E32 = max(max|mlp32_plain - mlp64|, 2^-24 max|mlp64|), a quantity of the reference alone."""
    y64 = mlp64(name, dims, params, x)
    e = float(np.abs(mlp32_plain(name, dims, params, x).astype(np.float64) - y64).max())
    return y64, max(e, U24 * float(np.abs(y64).max()))


def zero_margin(name, dims, params, x):
    """min over the hidden pre-activations v (float64) of |v| / (64 x 2^-24 (sum_k |x_k w_k| + |b|)).  Above 1, a float32 evaluation of v whose error
    stays below 64 x 2^-24 of the summed magnitudes does not land on the other side of 0, where a derivative that jumps at 0 would differ by O(1).
    inf for a net without a hidden layer."""
    a = np.asarray(x, np.float64).reshape(-1, dims[0])
    worst = np.inf
    for W, b in split_params(dims, params)[:-1]:
        W, b = W.astype(np.float64), b.astype(np.float64)
        v = a @ W.T + b
        mag = np.abs(a) @ np.abs(W).T + np.abs(b)
        worst = min(worst, float((np.abs(v) / (64 * U24 * mag)).min()))
        a = act64(name, v)
    return worst
