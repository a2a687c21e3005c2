"""Cases and assertions of the LIDAR scan tests (include/go2sim_lidar.h): inputs are generated from seeds here, the reference is tests/lidar_ref.py.
tests/test_lidar_ref.py checks the table's own condition (ambiguous points) without a GPU, tests/test_lidar_gpu.py runs the HIP library through it.

The heightfield is 40 x 30 cells of 5 cm, every cell a distinct multiple of the vertical scale (-3 m .. 3 m): a wrong cell is a wrong value.  Poses are
drawn around the field so that sample points leave it on all four sides, with yaw on both sides of +-pi, roll and pitch up to 0.4 rad, and heights
that put |raw| on both sides of the clip."""
import numpy as np

import lidar_ref as R

ROWS, COLS, H_SCALE, V_SCALE = 40, 30, 0.05, 0.005
ORIGIN = (-0.3, -0.75, 0.0)
STEPS = 6

GRIDS = {
    "5x3_9x5": {"actor_scan": {"x_points": [0.0, 0.15, 0.30, 0.50, 0.80], "y_points": [-0.15, 0.0, 0.15]},
                "critic_scan": {"num_x": 9, "num_y": 5, "x_range": [-0.4, 0.8], "y_range": [-0.3, 0.3]}},
    "1x1_none": {"actor_scan": {"x_points": [0.25], "y_points": [0.0]}, "critic_scan": {"num_x": 0, "num_y": 0}},
    "3x3_11x7": {"actor_scan": {"num_x": 3, "num_y": 3, "x_range": [0.0, 0.6], "y_range": [-0.2, 0.2]},
                 "critic_scan": {"num_x": 11, "num_y": 7, "x_range": [-0.5, 0.5], "y_range": [-0.3, 0.3]}},
}
ENVS = (1, 5, 67)
NOISE = {"height_noise_std": 0.02, "dropout_prob": 0.15, "full_blackout_prob": 0.05, "latency_prob": 0.1, "vertical_offset_std": 0.01}
# (name, curriculum level handed over through the device pointer, dr_schedule): L = 0, 0.35, 1 and once the two-phase mapping (L = 0.15 + 0.85 * 0.6 = 0.66)
LEVELS = (("L0", 0.0, None), ("L035", 0.35, None), ("L1", 1.0, None), ("two_phase", 0.8, {"phase1_level": 0.15, "terrain_gate": 0.5}))


def heightfield():
    return (np.arange(ROWS * COLS, dtype=np.int64).reshape(ROWS, COLS) - ROWS * COLS // 2).astype(np.int16)


def terrain():
    return {"hf": heightfield(), "origin": ORIGIN, "h_scale": H_SCALE, "v_scale": V_SCALE}


def quat_of(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=-1)


def poses(n_envs, steps, seed):
    """(pos [steps][n][3], quat [steps][n][4]) float32.  The first four envs of every step sit outside the four edges; yaw is drawn from all of
    (-pi, pi] and every third env is put within 1e-3 of +-pi; base heights put the terrain within and beyond the clip."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(ORIGIN[0] - 0.2, ORIGIN[0] + ROWS * H_SCALE + 0.2, (steps, n_envs))
    y = rng.uniform(ORIGIN[1] - 0.2, ORIGIN[1] + COLS * H_SCALE + 0.2, (steps, n_envs))
    z = rng.uniform(-2.5, 2.5, (steps, n_envs))
    yaw = rng.uniform(-np.pi, np.pi, (steps, n_envs))
    near = np.arange(n_envs) % 3 == 2
    yaw[:, near] = np.where(rng.random((steps, int(near.sum()))) < 0.5, np.pi - 1e-3 * rng.random((steps, int(near.sum()))), -np.pi + 1e-3 * rng.random((steps, int(near.sum()))))
    edge = [(ORIGIN[0] - 1.5, None), (ORIGIN[0] + ROWS * H_SCALE + 1.5, None), (None, ORIGIN[1] - 1.5), (None, ORIGIN[1] + COLS * H_SCALE + 1.5)]
    for b, (ex, ey) in enumerate(edge[:n_envs]):
        if ex is not None:
            x[:, b] = ex
        if ey is not None:
            y[:, b] = ey
    if n_envs == 1:                                                # one env: inside, then beyond each edge in turn
        x[:, 0] = [0.513, edge[0][0], edge[1][0], 0.727, 0.931, 0.218][:steps]
        y[:, 0] = [0.113, 0.017, 0.231, edge[2][1], edge[3][1], -0.317][:steps]
    roll, pitch = rng.uniform(-0.4, 0.4, (steps, n_envs)), rng.uniform(-0.4, 0.4, (steps, n_envs))
    return np.stack([x, y, z], axis=-1).astype(np.float32), quat_of(roll, pitch, yaw).astype(np.float32)


def resets(n_envs, steps):
    """uint8 [steps][n]: the chosen (env, step) pairs: env 0 at step 2 (a step after which a stale row would otherwise repeat it), the last env at steps 1 and 4"""
    r = np.zeros((steps, n_envs), np.uint8)
    r[2, 0] = 1
    r[1, n_envs - 1] = 1
    r[4, n_envs - 1] = 1
    return r


def lidar_cfg(grid, scale=1.0, clip=1.0, noise=None):
    return dict(GRIDS[grid], enabled=True, noise=dict(NOISE if noise is None else noise), height_clip=clip, height_scale=scale)


def cases():
    """(name, grid, n_envs, level name, level, dr_schedule, scale, seed)"""
    out = []
    for gi, grid in enumerate(GRIDS):
        for n in ENVS:
            for li, (lname, level, sched) in enumerate(LEVELS):
                out.append((f"{grid}-n{n}-{lname}", grid, n, lname, level, sched, 1.0, 1000 + 100 * gi + 10 * ENVS.index(n) + li))
    out.append(("5x3_9x5-n67-L1-scale05", "5x3_9x5", 67, "L1", 1.0, None, 0.5, 77))
    return out


def case_inputs(case):
    name, grid, n, lname, level, sched, scale, seed = case
    pos, quat = poses(n, STEPS, seed)
    return {"pos": pos, "quat": quat, "reset": resets(n, STEPS), "cfg": lidar_cfg(grid, scale=scale), "level": level, "dr_schedule": sched, "seed": seed}


def layout_of(cfg):
    """The sample points of a lidar cfg as float32 [2][k] arrays, by the package's own reader (torch linspace / meshgrid, as the reference forms them)."""
    from go2_sim2real_locomotion_rl_amd.lidar import lidar_layout

    return lidar_layout(cfg)


def ambiguous_fraction(case):
    """Share of (step, env, point) triples whose cell is ambiguous on either axis, over both grids."""
    inp = case_inputs(case)
    lay = layout_of(inp["cfg"])
    P = terrain()
    amb = tot = 0
    for t in range(STEPS):
        for pts in (lay["actor_xy"], lay["critic_xy"]):
            if pts.shape[1]:
                a = R.raw_sets(P, inp["pos"][t], inp["quat"][t], pts)[2]
                amb, tot = amb + int(a.sum()), tot + a.size
    return amb / max(tot, 1)


def check_step(inp, lay, t, L, stored_prev, got_actor, got_both, stats):
    """One step's outputs against lidar_ref: the admissible-set match of both scans, the stored scan being what the row holds.  Prints before it
    asserts; `stats` counts what fired."""
    P, N = terrain(), dict(inp["cfg"]["noise"], height_clip=inp["cfg"]["height_clip"], height_scale=inp["cfg"]["height_scale"])
    n = inp["pos"].shape[1]
    na, nc = lay["actor_xy"].shape[1], lay["critic_xy"].shape[1]
    d = R.draws(n, na, inp["seed"], t)
    v, tol, amb, masks = R.actor_scan(P, N, inp["pos"][t], inp["quat"][t], lay["actor_xy"], L, d, stored_prev, inp["reset"][t])
    ok, worst = R.match(got_actor, v, tol)
    print(f"step {t}: actor worst ratio {worst:.3f}, ambiguous {int(amb.sum())}/{amb.size}, dropout {int(masks['dropout'].sum())}, "
          f"latency {int(masks['latency'].sum())}, blackout {int(masks['blackout'].sum())}, reset {int(masks['reset'].sum())}")
    assert ok.all(), f"actor scan outside the admissible set at {np.argwhere(~ok)[:5].tolist()}"
    assert np.array_equal(got_both[:, :na], got_actor), "the critic row's actor columns are not the actor row's"
    for key in ("dropout", "latency", "blackout", "reset"):
        stats[key] = stats.get(key, 0) + int(masks[key].sum())
    stats["stale_nonzero"] = stats.get("stale_nonzero", 0) + int((np.abs(np.asarray(stored_prev))[masks["latency"] & ~masks["blackout"]] > 0).any(axis=-1).sum())
    stats["clipped"] = stats.get("clipped", 0) + int((np.abs(got_actor) == np.float32(abs(N["height_clip"] * N["height_scale"]))).sum())
    if nc:
        vc, tolc, ambc = R.critic_scan(P, N, inp["pos"][t], inp["quat"][t], lay["critic_xy"], inp["reset"][t])
        okc, worstc = R.match(got_both[:, na:], vc, tolc)
        print(f"step {t}: critic worst ratio {worstc:.3f}, ambiguous {int(ambc.sum())}/{ambc.size}")
        assert okc.all(), f"critic scan outside the admissible set at {np.argwhere(~okc)[:5].tolist()}"
