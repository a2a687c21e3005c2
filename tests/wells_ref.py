"""Numpy restatement of the stairwell env's law (include/go2sim_wells.h): the height scan, the well spawn, the level assignment and the alive term.
It imports nothing of the project but the Philox words of tests/policy_ref.py and the admissible-set lookup of tests/lidar_ref.py.
tests/test_wells_ref.py pins this file to the reference's own methods (tests/golden/ref_wells.npz), the GPU tests run the HIP library against it.

The scan exists twice.  `scan_f32` is the law in float32 numpy: its table lookups and its subtraction are exact, its sine, cosine and arctangent are
numpy's, not the library's, so it equals another float32 evaluation wherever no point lies within rounding of a cell edge.  `scan_sets` is the float64
reference with the admissible sets of tests/lidar_ref.py: a point near a cell edge may take either neighbour's height, and nothing is left out."""
import numpy as np

import lidar_ref as LR
import policy_ref as PR

PURPOSE = 15            # GO2SIM_WELLS_RNG_PURPOSE
PURPOSE_POSE = 8        # GO2SIM_RNG_RESET_POSE (include/go2sim_rng.h): word 0 the z offset, words 1, 2 roll and pitch
JITTER = 0.3            # GO2SIM_WELLS_SPAWN_JITTER
f32 = np.float32


def grid_points(xs, ys):
    """float32 [2][nx * ny], point k = i * ny + j"""
    xs, ys = np.asarray(xs, f32), np.asarray(ys, f32)
    return np.stack([np.repeat(xs, len(ys)), np.tile(ys, len(xs))]).astype(f32)


def field(hf, info):
    return {"hf": np.asarray(hf, np.int16), "origin": tuple(info["terrain_origin"][:2]), "h_scale": info["horizontal_scale"], "v_scale": info["vertical_scale"]}


# ---- the scan ------------------------------------------------------------------------------------------------------------------------------------
def scan_f32(P, pos, quat, pts):
    """The law in float32, operation by operation: [n][k] float32."""
    pos, quat = np.asarray(pos, f32), np.asarray(quat, f32)
    lx, ly = np.asarray(pts, f32)
    w, x, y, z = quat.T
    two, one = f32(2.0), f32(1.0)
    yaw = np.arctan2(two * (w * z + x * y), one - two * (y * y + z * z)).astype(f32)
    c, s = np.cos(yaw).astype(f32)[:, None], np.sin(yaw).astype(f32)[:, None]
    wx = pos[:, 0:1] + c * lx[None] - s * ly[None]
    wy = pos[:, 1:2] + s * lx[None] + c * ly[None]
    hfm = np.asarray(P["hf"]).astype(f32) * f32(P["v_scale"])
    hs, ox, oy = f32(P["h_scale"]), f32(P["origin"][0]), f32(P["origin"][1])

    def cell(q, n):                                       # trunc toward zero, clamp; a NaN selects 0
        with np.errstate(invalid="ignore"):
            return np.where(q >= 1.0, np.where(q >= n - 1, n - 1, np.trunc(np.where(np.isfinite(q), q, 0.0))), 0).astype(np.int64)

    with np.errstate(invalid="ignore", over="ignore"):
        col, row = cell((wx - ox) / hs, hfm.shape[0]), cell((wy - oy) / hs, hfm.shape[1])
    return (hfm[col, row] - pos[:, 2:3]).astype(f32)


def scan_sets(P, pos, quat, pts):
    """(values [n][k][4], tol [n][k][4], ambiguous [n][k]): the float64 reference with admissible sets; the bound on the transcendental part is the
    one tests/lidar_ref.py states for the critic scan (no clip, scale 1)."""
    return LR.critic_scan(P, {"height_clip": np.inf, "height_scale": 1.0}, pos, quat, pts)


# ---- the level assignment (_assign_wells) ----------------------------------------------------------------------------------------------------------
def assign_levels(n, curriculum_level, n_levels, near_draw, easy_draw, perm):
    """levels [n] of the n reset envs in env order.  near_draw(lo, hi, count) / easy_draw(lo, hi, count) return integers in [lo, hi]; perm is the
    permutation: env j receives position perm[j] of the 40 / 30 / 30 list."""
    max_level = max(0, min(int(curriculum_level * (n_levels - 1)), n_levels - 1))
    levels = np.zeros(n, np.int64)
    n_frontier, n_near = int(n * 0.40), int(n * 0.30)
    levels[:n_frontier] = max_level
    if max_level >= 2:
        levels[n_frontier:n_frontier + n_near] = near_draw(max(0, max_level - 2), max(0, max_level - 1), n_near)
    else:
        levels[n_frontier:n_frontier + n_near] = max_level
    levels[n_frontier + n_near:] = easy_draw(0, max(0, max_level - 3) if max_level >= 3 else 0, n - n_frontier - n_near)
    return levels[np.asarray(perm)]


# ---- the spawn -----------------------------------------------------------------------------------------------------------------------------------
def spawn_coord(centre, u):
    """f32(centre + (-0.3 + (0.3 - (-0.3)) u)) in float64, one rounding: python's random.uniform(-0.3, 0.3) added to the centre"""
    a, b = -JITTER, JITTER
    return f32(np.float64(centre) + (a + (b - a) * np.float64(u)))


def rand_float(lo, hi, u):
    """gs_rand_float with python-float bounds: f32(hi - lo) * u + f32(lo), float32"""
    return f32(f32(hi - lo) * f32(u) + f32(lo))


def spawn_z(bottom_z, init_z, z_range=None, u=None):
    """z of the stair env's spawn: f32 centre z + f32 init z, then ((z + offset) - init_z) + init_z with init_pos_z_range"""
    iz = f32(init_z)
    z = f32(f32(bottom_z) + iz)
    if z_range is None:
        return z
    return f32(f32(f32(z + rand_float(z_range[0], z_range[1], u)) - iz) + iz)


def spawn_words(seed, envs, reset_call, purpose=PURPOSE):
    """dm_u01 of the four words of block (env, reset call, purpose, 0): float64 [4][n], each exact in float32"""
    r = PR.philox4x32(np.asarray(envs, np.uint64), np.uint64(reset_call), np.uint64(purpose), np.uint64(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([PR.u01(w) for w in r])


def spawn(centers, levels, u_x, u_y, u_yaw=None, euler_range_deg=None):
    """(x, y, yaw) float32 [n] of envs on `levels` with the three uniforms"""
    centers = np.asarray(centers, np.float64)
    x = np.array([spawn_coord(centers[l, 0], u) for l, u in zip(levels, u_x)], f32)
    y = np.array([spawn_coord(centers[l, 1], u) for l, u in zip(levels, u_y)], f32)
    yaw = np.zeros(len(x), f32)
    if euler_range_deg is not None:
        d2r = np.pi / 180.0
        yaw = np.array([rand_float(euler_range_deg[0] * d2r, euler_range_deg[1] * d2r, u) for u in u_yaw], f32)
    return x, y, yaw


# ---- the alive term ------------------------------------------------------------------------------------------------------------------------------
def alive_inc(scale, dt=0.02):
    return f32(float(scale) * float(dt))


def alive_steps(rew, resets, scale, dt=0.02):
    """rew [T][n] float32 (the core's sums), resets [T][n] bool -> (rew + inc [T][n], alive_sum [n], steps [n], alive_ep [T][n] (NaN where none was
    handed over)), float32 operation by operation"""
    rew, resets = np.asarray(rew, f32), np.asarray(resets, bool)
    inc, fdt = alive_inc(scale, dt), f32(dt)
    T, n = rew.shape
    s, k = np.zeros(n, f32), np.zeros(n, np.int32)
    out, ep = np.zeros((T, n), f32), np.full((T, n), np.nan, f32)
    for t in range(T):
        out[t] = rew[t] + inc
        s = (s + inc).astype(f32)
        k = k + 1
        r = resets[t]
        ep[t, r] = s[r] / (np.maximum(k[r], 1).astype(f32) * fdt)
        s[r], k[r] = 0.0, 0
    return out, s, k, ep


match = LR.match
