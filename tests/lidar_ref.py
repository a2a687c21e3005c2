"""Float64 reference of the LIDAR terrain scan (include/go2sim_lidar.h), in plain numpy.  It imports nothing of the project but the Philox words of
tests/policy_ref.py.  The law is the header's; float32 appears only where the law names a rounding point: the thresholds f32(p * L), and the inputs
(poses, sample points, the stored scan), which are float32 data.  tests/test_lidar_ref.py pins this file to the reference's own methods
(tests/golden/ref_lidar_scan.npz), tests/test_lidar_gpu.py runs the HIP library against it.

THE LOOKUP RETURNS SETS.  The cell of a point is trunc((w - origin) / h_scale); where the float64 coordinate q lies within `delta` of an integer a
float32 evaluation may land on either side, so both neighbours are admissible.  delta is derived, per point and axis, from the float32 evaluation
    w = p + c lx - s ly;   q = (w - origin) / h_scale
  * (c, s): the yaw's arguments y = 2 (w z + x y), x = 1 - 2 (y y + z z) carry at most 8 u |q|^2 each (u = 2^-24: three roundings of terms bounded
    by |q|^2, doubled), which moves the angle by at most 16 u |q|^2 / hypot(x, y); dm_atan2 itself, its quotient y / x included, is held to 4.5 ulp
    of its result by tests/test_detmath.py, at most 5 ulp of pi = 5 x 2^-22; the sine and cosine are held to 2.5 ulp of theirs, at most 2^-22.  So
        e_cs = 16 u |q|^2 / hypot(x, y) + 6 x 2^-22
  * w: two products (u |l| each), two sums (u (|p| + |lx| + |ly|) each), the difference with the origin (u (|w| + |origin|)) and the float32
    rounding of the origin (u |origin|): at most 4 u (|p| + |lx| + |ly| + |origin|), plus (|lx| + |ly|) e_cs from the rotation
  * the division rounds once and divides by f32(h_scale): 2 u |q|
        delta = ((|lx| + |ly|) e_cs + 4 u (|p| + |lx| + |ly| + |origin|)) / h_scale + 2 u |q|
a function of |p|, |l|, |origin|, the scale and the conditioning of the yaw; nothing in it is chosen.

VALUE BOUND.  Against an admissible cell's height h the float32 result differs from the float64 one by at most
    tol = |scale| (8 u (|h| + |p.z| + |noise| + |offset|) + EZ (std + offset_std) L) + 2^-40
8 u: the heightfield product, the subtraction, two noise products and sums, the clamp's constant and the scale, each one rounding of a term no larger
than the sum in brackets.  EZ = 2^-17 bounds a float32 Box-Muller normal against the float64 one: the radius sqrt(-2 log u') <= 5.8 times the angle's
error (the product 2 pi v rounds to u 2 pi = 3.8e-7, f32(2 pi) is off by 1.8e-7 v, the sine 2 ulp of 1) gives 5.8 x 8e-7 = 4.6e-6, the radius'
own 3 ulp at |z| <= 5.8 another 1e-6: 5.6e-6 < 2^-17 = 7.6e-6.  A stale row is clip-and-scale of float32 data: 2 u |v|."""
import numpy as np

import policy_ref as PR

U = 2.0 ** -24
EZ = 2.0 ** -17
PURPOSE = 12


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------
def draws(n_envs, n_actor, seed, step):
    """The header's draw layout in float64: {"u_lat" [n], "u_black" [n], "z_b" [n], "z" [n][n_actor], "u" [n][n_actor]}."""
    env = np.arange(n_envs, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r = PR.philox4x32(env, np.uint64(step), np.uint64(PURPOSE), np.uint64(0), k0, k1)
    out = {"u_lat": PR.u01(r[0]), "u_black": PR.u01(r[1]), "z_b": PR.box_muller(r[2], r[3])[0]}
    nblk = (n_actor + 1) // 2
    if nblk:
        r = PR.philox4x32(env[:, None], np.uint64(step), np.uint64(PURPOSE), np.arange(1, nblk + 1, dtype=np.uint64)[None, :], k0, k1)
        z0, z1 = PR.box_muller(r[0], r[1])
        out["z"] = np.stack([z0, z1], axis=-1).reshape(n_envs, 2 * nblk)[:, :n_actor]
        out["u"] = np.stack([PR.u01(r[2]), PR.u01(r[3])], axis=-1).reshape(n_envs, 2 * nblk)[:, :n_actor]
    else:
        out["z"], out["u"] = np.zeros((n_envs, 0)), np.zeros((n_envs, 0))
    return out


def dr_level(level, dr_schedule=None, curriculum_enabled=True):
    """_get_dr_level (go2_env_stair_lidar.py:1197-1220) of the curriculum level, python floats."""
    t = float(level) if curriculum_enabled else 1.0
    if dr_schedule is None:
        return t
    p1, gate = float(dr_schedule["phase1_level"]), float(dr_schedule["terrain_gate"])
    if t < gate:
        return p1
    pr = (t - gate) / max(1e-6, 1.0 - gate)
    return p1 + (1.0 - p1) * min(1.0, max(0.0, pr))


def threshold(p, L):
    """f32(p * L): the product in float64, one rounding"""
    return np.float32(float(p) * float(L))


# ---- the lookup ------------------------------------------------------------------------------------------------------------------------------
def _axis_cells(q, delta, n):
    clampi = lambda v: np.clip(np.trunc(np.clip(v, -1e15, 1e15)), 0, n - 1).astype(np.int64)
    return clampi(q - delta), clampi(q + delta)


def raw_sets(P, pos, quat, pts):
    """Admissible raw heights (before noise) of every point: (raw [n][k][4], h [n][k][4], ambiguous [n][k]).  The four entries are the combinations of
    the two admissible indices per axis; where an axis is not ambiguous its two indices coincide and entries repeat.
    P: {"hf" int16 [rows][cols], "origin" (x, y), "h_scale", "v_scale"}; pos [n][3], quat [n][4] float32; pts float32 [2][k]."""
    pos, quat = np.asarray(pos, np.float32).astype(np.float64), np.asarray(quat, np.float32).astype(np.float64)
    lx, ly = np.asarray(pts, np.float32).astype(np.float64)
    w, x, y, z = quat.T
    ya, xa = 2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)
    yaw = np.arctan2(ya, xa)
    q2 = (quat * quat).sum(1)
    e_cs = 16.0 * U * q2 / np.maximum(np.hypot(xa, ya), 1e-300) + 6.0 * 2.0 ** -22
    c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    wx = pos[:, 0:1] + c * lx[None] - s * ly[None]
    wy = pos[:, 1:2] + s * lx[None] + c * ly[None]
    hs, (ox, oy) = float(P["h_scale"]), P["origin"][:2]
    reach = (np.abs(lx) + np.abs(ly))[None]
    hf = np.asarray(P["hf"]).astype(np.float64) * float(P["v_scale"])
    idx = []
    amb = np.zeros(wx.shape, bool)
    for wc, pc, o, n in ((wx, pos[:, 0:1], ox, hf.shape[0]), (wy, pos[:, 1:2], oy, hf.shape[1])):
        q = (wc - o) / hs
        delta = (reach * e_cs[:, None] + 4.0 * U * (np.abs(pc) + reach + abs(o))) / hs + 2.0 * U * np.abs(q)
        lo, hi = _axis_cells(q, delta, n)
        amb |= lo != hi
        idx.append((lo, hi))
    h = np.stack([hf[idx[0][i], idx[1][j]] for i in (0, 1) for j in (0, 1)], axis=-1)
    return h - pos[:, 2:3, None], h, amb


def clip_scale(v, clip, scale):
    return np.clip(v, -float(clip), float(clip)) * float(scale)


def critic_scan(P, N, pos, quat, pts, reset=None):
    """(values [n][k][4], tol [n][k][4], ambiguous [n][k]); N: {"height_clip", "height_scale", ...}"""
    raw, h, amb = raw_sets(P, pos, quat, pts)
    v = clip_scale(raw, N["height_clip"], N["height_scale"])
    pz = np.abs(np.asarray(pos, np.float64)[:, 2:3, None])
    tol = abs(N["height_scale"]) * 8.0 * U * (np.abs(h) + pz) + 2.0 ** -40
    if reset is not None:
        r = np.asarray(reset, bool)
        v[r], tol[r] = 0.0, 0.0
    return v, tol, amb


def actor_scan(P, N, pos, quat, pts, L, d, stored_prev, reset=None):
    """One step of the actor scan: (values [n][k][4], tol [n][k][4], ambiguous [n][k], masks).  `d` = draws(...), `stored_prev` the float32 stored
    scan before the step (the checked side's own state: what a stale row repeats).  masks: {"dropout" [n][k], "latency" [n], "blackout" [n], "reset" [n]}
    as the law applies them (all False where the step's condition `parameter > 0 and L > 0` fails)."""
    raw, h, amb = raw_sets(P, pos, quat, pts)
    n, k = amb.shape
    on = L > 0
    std, off_std = float(np.float32(N["height_noise_std"])), float(np.float32(N["vertical_offset_std"]))
    Lf = float(np.float32(L))
    noise = np.zeros((n, k))
    if on and N["height_noise_std"] > 0:
        noise = (d["z"] * std) * Lf
    v = raw + noise[..., None]
    drop = np.zeros((n, k), bool)
    if on and N["dropout_prob"] > 0:
        drop = d["u"].astype(np.float32) < threshold(N["dropout_prob"], L)
        v[drop] = 0.0
    off = np.zeros(n)
    if on and N["vertical_offset_std"] > 0:
        off = (d["z_b"] * off_std) * Lf
    v = v + off[:, None, None]
    lat = np.zeros(n, bool)
    if on and N["latency_prob"] > 0:
        lat = d["u_lat"].astype(np.float32) < threshold(N["latency_prob"], L)
    black = np.zeros(n, bool)
    if on and N["full_blackout_prob"] > 0:
        black = d["u_black"].astype(np.float32) < threshold(N["full_blackout_prob"], L)
    sc = abs(float(N["height_scale"]))
    pz = np.abs(np.asarray(pos, np.float64)[:, 2:3, None])
    mag = np.where(drop[..., None], 0.0, np.abs(h) + pz + np.abs(noise)[..., None]) + np.abs(off)[:, None, None]
    ez = np.where(drop, 0.0, EZ * std * Lf)[..., None] + EZ * off_std * Lf * (np.abs(off) > 0)[:, None, None]
    tol = sc * (8.0 * U * mag + ez) + 2.0 ** -40
    prev = np.asarray(stored_prev, np.float32).astype(np.float64)
    v[lat] = prev[lat][..., None]
    tol[lat] = 0.0
    v[black] = 0.0
    tol[black] = 0.0
    v = clip_scale(v, N["height_clip"], N["height_scale"])
    tol[lat & ~black] = (2.0 * U * np.abs(v[lat & ~black])) + 2.0 ** -40
    rst = np.zeros(n, bool) if reset is None else np.asarray(reset, bool)
    v[rst], tol[rst] = 0.0, 0.0
    return v, tol, amb, {"dropout": drop & ~rst[:, None], "latency": lat & ~rst, "blackout": black & ~rst, "reset": rst}


def match(got, values, tol):
    """(ok [n][k], worst ratio): `got` lies within tol of one of the admissible values.  Where tol is 0 the value must be exact."""
    got = np.asarray(got, np.float64)[..., None]
    err = np.abs(got - values)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    best = ratio.min(-1)
    return best <= 1.0, float(best.max()) if best.size else 0.0
