"""Float64 reference of the four-value stair info (include/go2sim_stairinfo.h), in plain numpy.  It imports nothing of the project but the Philox words
of tests/policy_ref.py and the cell bound of tests/lidar_ref.py.  tests/test_stairinfo_ref.py pins this file to the reference's own methods
(tests/golden/ref_stair_info.npz), tests/test_stairinfo_gpu.py runs the HIP library against it.

EXACT FLOAT32 where the law decides something: the heights h_k = f32(f32(hf) * f32(v_scale)), their differences dh_k, the compare with f32(threshold),
the midpoint (x_k + x_{k+1}) / 2 of float32 samples, and the thresholds f32(p * L) of the three masks.  A riser that equals the threshold falls on the
side its float32 heights put it.

THE ANSWER OF THE DETECTOR IS A SET.  The cell of a sample is trunc((w - origin) / h_scale); where the float64 coordinate lies within `delta` of an
integer (the bound tests/lidar_ref.py derives, with ly = 0) both neighbours are admissible, so a sample has up to four admissible heights.  The first
edge depends on the choices of all samples before it: `edge_sets` walks the samples with the set of heights that reach sample k without an edge, and
collects every (edge, dir) that some admissible choice gives.  An env-step with more than one member is "ambiguous"; the checked side must produce one
member of the set (never skipped), and the test tables keep such env-steps under 1 %.

VALUE BOUND.  With u = 2^-24 and the float32 constants (scales, stds, L) taken as the float32 values the law names, the float32 result differs from this
file's float64 one by at most
    clean entry, blackout, no-noise entry:  v s                       one rounding                                       u |v s|
    noisy entry  (v + (z std) L) s:         two products, a sum, the scale, and the float32 Box-Muller normal            |s| (4 u (|v| + |z std L|) + EZ std L)
                                            (EZ = 2^-17, derived in tests/lidar_ref.py; the clamp to [0, max_range] is 1-Lipschitz)
    stale entry  (stored / s) s:            a division and a product of float32 data                                     2 u |stored|
    direction:   +-1 or 0 times s_dir:      exact
plus 2^-40 absolute for the float64 evaluation itself.  Masks (flip, latency, blackout, reset) are exact."""
import numpy as np

import lidar_ref as LR
import policy_ref as PR

U = LR.U
EZ = LR.EZ
PURPOSE = 13
F32 = np.float32

dr_level = LR.dr_level
threshold = LR.threshold


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------
def draws(n_envs, seed, step):
    """The header's draw layout in float64: {"z_e", "z_h", "z_d", "u_flip", "u_lat", "u_black"}, [n] each."""
    env = np.arange(n_envs, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r = PR.philox4x32(env, np.uint64(step), np.uint64(PURPOSE), np.uint64(0), k0, k1)
    z_e, z_h = PR.box_muller(r[0], r[1])
    z_d = PR.box_muller(r[2], r[3])[0]
    r = PR.philox4x32(env, np.uint64(step), np.uint64(PURPOSE), np.uint64(1), k0, k1)
    return {"z_e": z_e, "z_h": z_h, "z_d": z_d, "u_flip": PR.u01(r[0]), "u_lat": PR.u01(r[1]), "u_black": PR.u01(r[2])}


# ---- the lookup ------------------------------------------------------------------------------------------------------------------------------
def height_sets(P, pos, quat, xs):
    """Admissible float32 heights of every sample: (h float32 [n][k][4], ambiguous [n][k]).  The four entries are the combinations of the two
    admissible indices per axis (tests/lidar_ref.py `raw_sets`, with the sample on the body's x axis); entries repeat where an axis is not ambiguous.
    P: {"hf" int16 [rows][cols], "origin" (x, y), "h_scale", "v_scale"}; pos [n][3], quat [n][4] float32; xs float32 [k]."""
    pos, quat = np.asarray(pos, F32).astype(np.float64), np.asarray(quat, F32).astype(np.float64)
    lx = np.asarray(xs, F32).astype(np.float64)
    w, x, y, z = quat.T
    ya, xa = 2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)
    with np.errstate(invalid="ignore"):
        yaw = np.arctan2(ya, xa)
        q2 = (quat * quat).sum(1)
        e_cs = 16.0 * U * q2 / np.maximum(np.hypot(xa, ya), 1e-300) + 6.0 * 2.0 ** -22
        c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
        wx = pos[:, 0:1] + c * lx[None]
        wy = pos[:, 1:2] + s * lx[None]
    hs, (ox, oy) = float(P["h_scale"]), P["origin"][:2]
    reach = np.abs(lx)[None]
    hf = np.asarray(P["hf"]).astype(F32) * F32(P["v_scale"])                      # float32, as the library and the reference form the field
    idx = []
    amb = np.zeros(wx.shape, bool)
    for wc, pc, o, n in ((wx, pos[:, 0:1], ox, hf.shape[0]), (wy, pos[:, 1:2], oy, hf.shape[1])):
        q = (wc - o) / hs
        delta = (reach * e_cs[:, None] + 4.0 * U * (np.abs(pc) + reach + abs(o))) / hs + 2.0 * U * np.abs(q)
        lo, hi = LR._axis_cells(q, delta, n)
        amb |= lo != hi
        idx.append((lo, hi))
    h = np.stack([hf[idx[0][i], idx[1][j]] for i in (0, 1) for j in (0, 1)], axis=-1)
    return h, amb


def edge_sets(P, pos, quat, xs, max_range, thr):
    """Per env the sorted list of admissible (edge, dir) pairs, float32 values as python floats (module docstring)."""
    h, _ = height_sets(P, pos, quat, xs)
    xs = np.asarray(xs, F32)
    thr32 = F32(thr)
    out = []
    for b in range(h.shape[0]):
        found = set()
        alive = set(h[b, 0].tolist())
        for k in range(len(xs) - 1):
            nxt = set()
            for a in alive:
                for v in set(h[b, k + 1].tolist()):
                    dh = F32(v) - F32(a)
                    if np.abs(dh) > thr32:
                        found.add((float((xs[k] + xs[k + 1]) / F32(2.0)), float(np.sign(dh))))
                    else:
                        nxt.add(v)
            alive = nxt
            if not alive:
                break
        if alive:
            found.add((float(F32(max_range)), 0.0))
        out.append(sorted(found))
    return out


# ---- the four values ---------------------------------------------------------------------------------------------------------------------------
def masks_of(N, L, d, reset=None):
    """{"flip", "latency", "blackout", "reset"} [n] as the law applies them (all False where `parameter > 0 and L > 0` fails; reset envs excluded)."""
    n = len(d["u_flip"])
    on = L > 0
    rst = np.zeros(n, bool) if reset is None else np.asarray(reset, bool)
    m = {}
    for key, u, p in (("flip", "u_flip", "direction_flip_prob"), ("latency", "u_lat", "latency_prob"), ("blackout", "u_black", "full_blackout_prob")):
        m[key] = (d[u].astype(F32) < threshold(N[p], L)) & ~rst if (on and N[p] > 0) else np.zeros(n, bool)
    m["reset"] = rst
    return m


def stair_info(P, N, pos, quat, rows, L, d, stored_prev, reset=None):
    """One step: per env a list of candidates (actor [4], actor tol [4], clean [4], clean tol [4]) -- one per admissible (edge, dir) -- and the
    masks.  N: the constants of stair_info_layout (sample_x, max_range, threshold, the four scales, the six noise constants) plus "row_heights" and
    "row_depths" (float32 tables).  `d` = draws(...), `stored_prev` the float32 stored rows [n][4] before the step, rows int [n]."""
    n = np.asarray(pos).shape[0]
    sets = edge_sets(P, pos, quat, N["sample_x"], N["max_range"], N["threshold"])
    m = masks_of(N, L, d, reset)
    on = L > 0
    Lf = float(F32(L))
    s_e, s_h, s_d, s_dir = (float(F32(N[k])) for k in ("edge_dist_scale", "height_scale", "depth_scale", "direction_scale"))
    std = {k: float(F32(N[k + "_noise_std"])) for k in ("edge", "height", "depth")}
    mr = float(F32(N["max_range"]))
    rows = np.clip(np.asarray(rows, np.int64), 0, len(N["row_heights"]) - 1)
    prev = np.asarray(stored_prev, F32).astype(np.float64)
    tiny = 2.0 ** -40
    out = []
    for b in range(n):
        if m["reset"][b]:
            out.append([(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4))])
            continue
        height, depth = float(F32(N["row_heights"][rows[b]])), float(F32(N["row_depths"][rows[b]]))
        cands = []
        for edge, dr in sets[b]:
            clean = np.array([edge * s_e, height * s_h, depth * s_d, dr * s_dir])
            clean_tol = np.array([U * abs(clean[0]), U * abs(clean[1]), U * abs(clean[2]), 0.0]) + tiny
            clean_tol[3] = 0.0
            a, tol = np.zeros(4), np.zeros(4)
            # height and depth: never stale or blacked out
            for j, v, key, z, s in ((1, height, "height", d["z_h"][b], s_h), (2, depth, "depth", d["z_d"][b], s_d)):
                if on and std[key] > 0:
                    nz = (z * std[key]) * Lf
                    a[j], tol[j] = (v + nz) * s, abs(s) * (4.0 * U * (abs(v) + abs(nz)) + EZ * std[key] * Lf) + tiny
                else:
                    a[j], tol[j] = v * s, U * abs(v * s) + tiny
            e, e_tol = edge, 0.0
            if on and std["edge"] > 0:
                nz = (d["z_e"][b] * std["edge"]) * Lf
                e = min(max(edge + nz, 0.0), mr)
                e_tol = 4.0 * U * (abs(edge) + abs(nz)) + EZ * std["edge"] * Lf
            dd = -dr if m["flip"][b] else dr
            if m["blackout"][b]:
                a[0], tol[0], a[3], tol[3] = mr * s_e, U * abs(mr * s_e) + tiny, 0.0, 0.0
            elif m["latency"][b]:
                a[0], tol[0], a[3], tol[3] = prev[b, 0], 2.0 * U * abs(prev[b, 0]) + tiny, prev[b, 3], 2.0 * U * abs(prev[b, 3]) + tiny
                if prev[b, 3] == 0.0:
                    tol[3] = 0.0
            else:
                a[0], tol[0], a[3], tol[3] = e * s_e, abs(s_e) * e_tol + U * abs(e * s_e) + tiny, dd * s_dir, 0.0
            cands.append((a, tol, clean, clean_tol))
        out.append(cands)
    return out, m


def match(got_actor, got_clean, cands):
    """(ok [n], worst ratio, chosen candidate [n]): every env's two rows lie within tol of ONE candidate.  Where tol is 0 the value must be exact."""
    got_actor, got_clean = np.asarray(got_actor, np.float64), np.asarray(got_clean, np.float64)
    n = got_actor.shape[0]
    ok, chosen, worst = np.zeros(n, bool), np.full(n, -1), 0.0
    for b in range(n):
        best = np.inf
        for ci, (a, tol, c, ctol) in enumerate(cands[b]):
            err = np.abs(np.concatenate([got_actor[b] - a, got_clean[b] - c]))
            t = np.concatenate([tol, ctol])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf)).max()
            if ratio < best:
                best, chosen[b] = ratio, ci
        ok[b] = best <= 1.0
        worst = max(worst, best)
    return ok, float(worst), chosen
