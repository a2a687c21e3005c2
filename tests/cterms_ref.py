"""The contact terms of include/go2sim_cterms.h restated in numpy: a float64 reference with its admissible sets, the float32 law in the kernel's
operation order, the episode hand-over, and the force tables the fixture tool and the GPU tests share.

Force tables are float32 [N][13][3] over the ROBOT's links (the reference's `robot.links`: base, four hips, four thighs, four calves); the model's link
index is the robot's plus one (link 0 is the ground).

Bounds (u = 2^-24).  The float32 norm carries three rounded products, two rounded sums and one correctly rounded root: under 3u relative.
  body_contact   exact wherever no selected link's float64 norm lies within 3u n of the threshold; a link inside that band is AMBIGUOUS: both counts
                 are admissible.  At most 1 % of the link-rows of a table may be ambiguous (`check_ambiguity_cap`).
  stumble        |pen - pen64| <= u (4 sum_l n_l + 10 pen64): 3u n per norm and one rounding of the subtraction per link, eight roundings of the
                 nine-term sum.  The clamp is continuous, so no ambiguity arises.
A force with at most one non-zero component has an exact float32 norm, |F|: such a link is never ambiguous, and the threshold's own edges are
tested with such forces (`edge_rows`: at the threshold 0, one float32 above it 1)."""
import numpy as np

U = 2.0 ** -24
ROBOT_LINKS = ("base", "FL_hip", "FR_hip", "RL_hip", "RR_hip", "FL_thigh", "FR_thigh", "RL_thigh", "RR_thigh", "FL_calf", "FR_calf", "RL_calf", "RR_calf")
THIGHS = (ROBOT_LINKS.index("FR_thigh"), ROBOT_LINKS.index("FL_thigh"))       # the script's body_contact_names, robot numbering
NON_FEET = tuple(i for i, n in enumerate(ROBOT_LINKS) if not n.endswith("_calf"))
ALL_LINKS = tuple(range(len(ROBOT_LINKS)))
MASK_SETS = {"one": (THIGHS[0],), "thighs": THIGHS, "non_feet": NON_FEET, "all": ALL_LINKS}
BODY_THRESHOLD, STUMBLE_THRESHOLD, DT = 1.0, 5.0, 0.02


def model_mask(robot_links):
    """uint32 mask in the model's numbering of a set of robot links"""
    m = 0
    for l in robot_links:
        m |= 1 << (int(l) + 1)
    return m


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def norms64(F):
    F = np.asarray(F, np.float64)
    return np.sqrt((F * F).sum(-1))


def body_count_sets(F, links, thr):
    """-> (lo, hi, ambiguous [N][len(links)]): every integer count in [lo, hi] is admissible for the row.  A NaN norm counts 0."""
    with np.errstate(invalid="ignore"):
        n = norms64(F)[:, list(links)]
        t = float(np.float32(thr))
        above = n > t
        exact = (np.asarray(F)[:, list(links)] != 0).sum(-1) <= 1          # at most one component: |F| itself, no rounding
        amb = (np.abs(n - t) <= 3.0 * U * n) & ~exact
    lo = (above & ~amb).sum(1)
    return lo, lo + amb.sum(1), amb


def stumble64(F, links, thr):
    """-> (pen64 [N], bound [N]); NaN where a selected norm is NaN"""
    with np.errstate(invalid="ignore"):
        n = norms64(F)[:, list(links)]
        d = n - float(np.float32(thr))
        pen = np.where(d < 0.0, 0.0, d).sum(1)
        return pen, U * (4.0 * n.sum(1) + 10.0 * pen)


def check_ambiguity_cap(F, links, thr, cap=0.01):
    amb = body_count_sets(F, links, thr)[2]
    frac = amb.mean() if amb.size else 0.0
    assert frac <= cap, f"{amb.sum()} of {amb.size} link-rows are ambiguous ({100 * frac:.2f} %): the table must hold the cap"
    return frac


# ---- the float32 law in the kernel's order ----------------------------------------------------------------------------------------------
def norms32(F):
    F = np.asarray(F, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((F[..., 0] * F[..., 0] + F[..., 1] * F[..., 1]) + F[..., 2] * F[..., 2]).astype(np.float32)


def law32(F, body_links, stumble_links, body_thr=BODY_THRESHOLD, stumble_thr=STUMBLE_THRESHOLD):
    """-> (count float32 [N], pen float32 [N]) as k_cterms_step forms them"""
    n = norms32(F)
    with np.errstate(invalid="ignore"):
        count = (n[:, list(body_links)] > np.float32(body_thr)).sum(1).astype(np.float32)
        pen = np.zeros(len(n), np.float32)
        for l in sorted(stumble_links):
            d = n[:, l] - np.float32(stumble_thr)
            pen = pen + np.where(d < 0, np.float32(0.0), d).astype(np.float32)
    return count, pen


def inc32(scale, dt=DT):
    return np.float32(float(scale) * float(dt))


def hand_over(total, steps, dt=DT):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float32(total) / (np.float32(max(int(steps), 1)) * np.float32(dt))).astype(np.float32)


class Episode:
    """Host model of the launch's per-env state, one term order: body_contact then stumble.  terms: list of float32 [n] per applied term."""

    def __init__(self, n, n_terms=2):
        self.sum, self.steps, self.ep = np.zeros((n_terms, n), np.float32), np.zeros((n_terms, n), np.int32), np.zeros((n_terms, n), np.float32)

    def step(self, rew, terms, reset):
        """terms: {term index: float32 [n]}; -> rew after the adds, in term order"""
        rew = np.asarray(rew, np.float32).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for t in sorted(terms):
                v = np.asarray(terms[t], np.float32)
                rew = rew + v
                self.sum[t] = self.sum[t] + v
                self.steps[t] += 1
                self.clear(np.flatnonzero(np.asarray(reset) != 0), (t,))
        return rew

    def clear(self, idx, which=None):
        for t in (range(len(self.sum)) if which is None else which):
            for b in idx:
                self.ep[t, b] = hand_over(self.sum[t, b], self.steps[t, b])
                self.sum[t, b], self.steps[t, b] = 0.0, 0


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def random_rows(n, seed, top=50.0):
    """n rows of sparse random contact: every link is loaded with probability 1/2 by a force of uniform direction and a magnitude in [0, top) N"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, len(ROBOT_LINKS), 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    mag = rng.uniform(0.0, top, (n, len(ROBOT_LINKS), 1)) * (rng.random((n, len(ROBOT_LINKS), 1)) < 0.5)
    return (d * mag).astype(np.float32)


def edge_rows(thr, links):
    """Single-component forces at the threshold and one float32 above it, in x, y and z, both signs, on each of `links` (all other links unloaded)
    -> (rows [len(links) * 12][13][3], over [len(links) * 12] bool: the norm exceeds the threshold).  The norm of such a force is exact."""
    t = np.float32(thr)
    up = np.nextafter(t, np.float32(np.inf))
    rows, over = [], []
    for l in links:
        for comp in range(3):
            for sign in (1.0, -1.0):
                for v in (t, up):
                    F = np.zeros((len(ROBOT_LINKS), 3), np.float32)
                    F[l, comp] = np.float32(sign) * v
                    rows.append(F); over.append(v > t)
    return np.stack(rows), np.array(over)


def special_rows():
    """NaN and infinite components: rows [5][13][3]"""
    F = np.zeros((5, len(ROBOT_LINKS), 3), np.float32)
    a, b = THIGHS
    F[0, a] = (np.nan, 0.0, 0.0)                      # a NaN norm: count 0, stumble NaN
    F[1, a] = (3.0, np.nan, 4.0); F[1, b] = (0.0, 2.0, 0.0)
    F[2, a] = (np.inf, 0.0, 0.0)                      # an infinite norm: count 1, stumble inf
    F[3, a] = (-np.inf, 1.0, 0.0); F[3, b] = (0.0, 0.0, -7.0)
    F[4, a] = (np.inf, np.nan, 0.0)                   # inf and NaN on one link: NaN
    return F
