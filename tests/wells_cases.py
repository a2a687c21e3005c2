"""Shared cases of the stairwell tests: the three terrain dictionaries, the scan grids, the poses and the constant draw schedule of the fixture
(tools/make_ref_stairwell_fixtures.py, tests/test_wells_ref.py, tests/test_wells_gpu.py, tests/test_wells_env_gpu.py).  Plain numpy, no GPU."""
import numpy as np

# (a) the smallest terrain that has every feature: two flights with a landing, four levels on rows of three (the second well row partly empty)
TERRAIN_A = {"enabled": True, "horizontal_scale": 0.05, "vertical_scale": 0.005, "step_depth_m": 0.10, "steps_per_flight": 2, "num_flights_per_side": 2,
             "flat_landing_m": 0.1, "flat_bottom_m": 0.3, "flat_surround_m": 0.4, "step_height_min": 0.02, "step_height_max": 0.135,
             "num_difficulty_levels": 4, "wells_per_row": 3}
# (b) one flight per side (no landing), one level
TERRAIN_B = dict(TERRAIN_A, num_flights_per_side=1, num_difficulty_levels=1, steps_per_flight=3)
# (c) the training geometry (the builder's defaults) with three steps per flight and three levels
TERRAIN_C = {"enabled": True, "horizontal_scale": 0.05, "vertical_scale": 0.005, "step_depth_m": 0.39, "steps_per_flight": 3, "num_flights_per_side": 2,
             "flat_landing_m": 1.5, "flat_bottom_m": 2.0, "flat_surround_m": 4.0, "step_height_min": 0.02, "step_height_max": 0.135,
             "num_difficulty_levels": 3, "wells_per_row": 3}
TERRAINS = {"a": TERRAIN_A, "b": TERRAIN_B, "c": TERRAIN_C}

SCAN_11 = {"num_x": 11, "num_y": 11, "x_range": [-0.5, 0.5], "y_range": [-0.5, 0.5]}
GRIDS = {"11x11": SCAN_11, "16x16": {"num_x": 16, "num_y": 16, "x_range": [-0.6, 0.6], "y_range": [-0.6, 0.6]},
         "1x1": {"num_x": 1, "num_y": 1, "x_range": [0.0, 0.0], "y_range": [0.0, 0.0]},
         "3x5": {"num_x": 3, "num_y": 5, "x_range": [-0.2, 0.4], "y_range": [-0.3, 0.3]}}

# the fixture's draws: every uniform in [0, 1) the reference asks for comes from this cycle (all exact in float32, as dm_u01's values are)
U_CYCLE = np.array([0.25, 0.75, 0.0625, 0.5, 0.0, 0.999999940395355224609375, 0.3125, 0.8125], np.float64)


def with_scan(terrain, grid="11x11"):
    return dict(terrain, height_scan=dict(GRIDS[grid]))


def quat_of_yaw(yaw, roll=0.0, pitch=0.0):
    """euler (roll, pitch, yaw) -> (w, x, y, z), float64"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack(np.broadcast_arrays(cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy), -1)


def poses(n, info, seed=0):
    """n generic float32 poses over terrain `info` (random position a little beyond the field on every side, any yaw, small roll / pitch), then the
    named ones: a well's bottom, a stair edge, outside the field on all four sides, yaw 0 / pi / near +-pi.  -> (pos [m][3], quat [m][4]) float32"""
    rng = np.random.default_rng(seed)
    X, Y = info["total_x_m"], info["total_y_m"]
    pos = np.stack([rng.uniform(-0.6 * X, 0.6 * X, n), rng.uniform(-0.6 * Y, 0.6 * Y, n), rng.uniform(0.0, 0.8, n)], 1)
    quat = quat_of_yaw(rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n))
    cx, cy, cz = info["well_spawns"][0]["center"]
    hs = info["horizontal_scale"]
    edge = cx + (int(round(0.3 / hs)) // 2 + 1) * hs                      # the first riser of well 0 along +x (flat_bottom_m = 0.3 in terrains a and b)
    named_pos = [(cx, cy, cz + 0.42), (edge, cy, cz + 0.42), (-X, 0.0, 0.4), (X, 0.0, 0.4), (0.0, -Y, 0.4), (0.0, Y, 0.4),
                 (cx, cy, 0.5), (cx, cy, 0.5), (cx, cy, 0.5), (cx, cy, 0.5)]
    named_yaw = [0.3, 0.0, 1.0, -2.0, 0.5, 2.5, 0.0, np.pi, np.pi - 1e-6, -np.pi + 1e-6]
    pos = np.concatenate([pos, np.asarray(named_pos)])
    quat = np.concatenate([quat, quat_of_yaw(np.asarray(named_yaw))])
    return pos.astype(np.float32), quat.astype(np.float32)


def tile_poses(pos, quat, n):
    """the first n of the poses repeated cyclically"""
    k = np.arange(n) % len(pos)
    return np.ascontiguousarray(pos[k]), np.ascontiguousarray(quat[k])
