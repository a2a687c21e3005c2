"""Numpy float32 restatement of the rough-terrain env's law (include/go2sim_tiles.h): ground height, boundary, spawn, the base-height term.  Every
line is ONE IEEE binary32 operation on float32 arrays (numpy rounds each to float32), in the header's order, so the HIP library must agree bit for
bit (tests/test_tiles_gpu.py, tests/test_rough_env_gpu.py).  It imports nothing of the project but the Philox words of tests/policy_ref.py;
tests/test_tiles_ref.py pins it to the reference's own TerrainManager (tests/golden/ref_tiles_manager.npz)."""
import numpy as np

import policy_ref as PR

PURPOSE = 14
F = np.float32


def ulp32(x):
    """Spacing of float32 at |x| (of the largest entry of an array)."""
    return float(np.spacing(F(np.max(np.abs(np.asarray(x, np.float64))))))


def clip_l(q, n):
    """l = 0 unless q > 0; n - 2 if q >= n - 2; else q  -- comparisons a NaN fails"""
    q = np.asarray(q, F)
    top = F(n - 2)
    with np.errstate(invalid="ignore"):
        l = np.where(q > F(0), q, F(0))
        l = np.where(q >= top, top, l)
    return l.astype(F)


def metres(hf, vertical_scale):
    """The library's copy of an int16 field: f32(hf) * f32(vertical_scale) per cell."""
    return np.asarray(hf).astype(F) * F(vertical_scale)


def ground_height(H, origin, hs, wx, wy):
    """H float32 [rows][cols] metres, origin (x, y), hs; wx, wy float32 [n] -> float32 [n]"""
    H = np.asarray(H, F)
    rows, cols = H.shape
    ox, oy, hs = F(origin[0]), F(origin[1]), F(hs)
    wx, wy = np.asarray(wx, F), np.asarray(wy, F)
    with np.errstate(invalid="ignore", over="ignore"):
        qx = wx - ox
        qx = qx / hs
        qy = wy - oy
        qy = qy / hs
    lx, ly = clip_l(qx, rows), clip_l(qy, cols)
    ix, iy = lx.astype(np.int64), ly.astype(np.int64)
    assert ix.min(initial=0) >= 0 and ix.max(initial=0) <= rows - 2 and iy.min(initial=0) >= 0 and iy.max(initial=0) <= cols - 2
    fx = lx - ix.astype(F)
    fy = ly - iy.astype(F)
    gx = F(1) - fx
    gy = F(1) - fy
    h00, h10, h01, h11 = H[ix, iy], H[ix + 1, iy], H[ix, iy + 1], H[ix + 1, iy + 1]
    h = h00 * gx
    h = h * gy
    t = h10 * fx
    t = t * gy
    h = h + t
    t = h01 * gx
    t = t * fy
    h = h + t
    t = h11 * fx
    t = t * fy
    h = h + t
    return h.astype(F)


def out_of_bounds(bx, by, sx, sy, max_wander):
    dx = np.asarray(bx, F) - np.asarray(sx, F)
    dy = np.asarray(by, F) - np.asarray(sy, F)
    a = dx * dx
    b = dy * dy
    d = a + b
    d = np.sqrt(d)
    with np.errstate(invalid="ignore"):
        return d > F(max_wander)


def u01(word):
    """dm_u01: 24 random bits"""
    return (np.asarray(word, np.uint32) >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def spawn_words(n_envs, seed, reset_call):
    """The Philox block of every env for the spawn of reset call `reset_call` (the number of reset calls before it): uint32 [n][4]"""
    env = np.arange(n_envs, dtype=np.uint64)
    r = PR.philox4x32(env, np.uint64(reset_call), np.uint64(PURPOSE), np.uint64(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([np.asarray(w, np.uint64).astype(np.uint32) for w in r], axis=1)


def spawn(H, origin, hs, grid, words):
    """grid: dict n_rows, n_cols, size (x, y), jitter (x, y), base_z, spawn_offset (python floats, rounded to float32 here as the library rounds
    them); words uint32 [n][4] -> (pos float32 [n][3], tile_row int32 [n], tile_col int32 [n])"""
    w = np.asarray(words, np.uint32)
    row = (w[:, 0] % np.uint32(grid["n_rows"])).astype(np.int32)
    col = (w[:, 1] % np.uint32(grid["n_cols"])).astype(np.int32)

    def axis(o, tile, size, word, jitter):
        c = tile.astype(F) + F(0.5)
        c = c * F(size)
        c = F(o) + c
        if F(jitter) > F(0):
            j = u01(word) * F(2)
            j = j - F(1)
            j = j * F(jitter)
            c = c + j
        return c.astype(F)

    x = axis(origin[0], row, grid["size"][0], w[:, 2], grid["jitter"][0])
    y = axis(origin[1], col, grid["size"][1], w[:, 3], grid["jitter"][1])
    z = ground_height(H, origin, hs, x, y) + F(grid["base_z"])
    z = z + F(grid["spawn_offset"])
    return np.stack([x, y, z.astype(F)], axis=1), row, col


def base_height_term(pz, ground, target, scale_dt):
    """_reward_base_height x its scale: ((p.z - ground) - target)^2 * f32(scale * dt)"""
    d = np.asarray(pz, F) - np.asarray(ground, F)
    d = d - F(target)
    d = d * d
    return (d * F(scale_dt)).astype(F)


def height_bound(H, origin, hs, wx, wy):
    """The bound within which the reference's own query (float32 / float64 mixed, raw units interpolated and scaled last) and this restatement
    agree: 4 ulp32(max |w - origin|) / hs x D + 8 ulp32(max |h|), D the largest difference between adjacent cells."""
    H = np.asarray(H, np.float64)
    D = max(np.abs(np.diff(H, axis=0)).max(), np.abs(np.diff(H, axis=1)).max())
    w = max(np.abs(np.asarray(wx, np.float64) - origin[0]).max(), np.abs(np.asarray(wy, np.float64) - origin[1]).max())
    return 4.0 * ulp32(w) / hs * D + 8.0 * ulp32(np.abs(H).max())
