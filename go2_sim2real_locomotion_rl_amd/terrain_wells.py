"""The stairwell terrain of the reference's omnidirectional stair env (examples/locomotion/go2_env_stair6_Omni.py:45-215, `build_stairwell_terrain`):
a grid of inverted square pyramids, one per difficulty level, with `num_flights_per_side` flights of stairs on all four sides and a landing between
two flights.  The robot spawns on the flat bottom and climbs out in whatever direction its command points.

    hf, info = build_stairwell_terrain(env_cfg["terrain"])       # int16 [x cells][y cells], the reference's `terrain_info` keys

Own numpy restatement with the reference's defaults and keys; it prints nothing.  tests/test_wells_ref.py pins it to the reference's own output
(tests/golden/ref_wells.npz)."""
import math

import numpy as np

WELL_KEYS = ("num_difficulty_levels", "wells_per_row", "steps_per_flight", "num_flights_per_side")


def is_well_terrain_cfg(t):
    """True for an enabled terrain dictionary that carries one of the stairwell keys; no corridor or tile dictionary carries any of them."""
    return bool(t) and bool(t.get("enabled", False)) and any(k in t for k in WELL_KEYS)


def build_stairwell_terrain(terrain_cfg):
    g = terrain_cfg.get
    h_scale, v_scale = g("horizontal_scale", 0.05), g("vertical_scale", 0.005)
    step_depth_m, steps_per_flight, num_flights = g("step_depth_m", 0.39), g("steps_per_flight", 10), g("num_flights_per_side", 2)
    num_levels, wells_per_row = g("num_difficulty_levels", 9), g("wells_per_row", 3)
    cells = lambda metres: max(1, int(round(metres / h_scale)))
    step_depth, flat_bottom = cells(step_depth_m), cells(g("flat_bottom_m", 2.0))
    flat_landing, flat_surround = cells(g("flat_landing_m", 1.5)), cells(g("flat_surround_m", 4.0))
    flight = steps_per_flight * step_depth
    half_bottom = flat_bottom // 2
    radius = half_bottom + num_flights * flight + (num_flights - 1) * flat_landing          # centre to rim
    block = 2 * radius + 1 + flat_surround
    num_well_rows = math.ceil(num_levels / wells_per_row)
    total_x, total_y = wells_per_row * block + flat_surround, num_well_rows * block + flat_surround
    step_heights_m = np.linspace(g("step_height_min", 0.02), g("step_height_max", 0.135), num_levels)
    step_units = np.round(step_heights_m / v_scale).astype(np.int32)
    total_steps = steps_per_flight * num_flights
    ground = int(total_steps * step_units[-1])
    origin = (-total_x * h_scale / 2.0, -total_y * h_scale / 2.0, 0.0)

    hf = np.full((total_x, total_y), ground, dtype=np.int16)
    ix, iy = np.arange(total_x)[:, None], np.arange(total_y)[None, :]
    spawns = {}
    for level in range(num_levels):
        wy, wx = divmod(level, wells_per_row)
        sh = int(step_units[level])
        bottom = ground - total_steps * sh
        cx = flat_surround // 2 + wx * block + radius
        cy = flat_surround // 2 + wy * block + radius
        dist = np.maximum(np.abs(ix - cx), np.abs(iy - cy))                              # Chebyshev distance from the centre, in cells
        h = np.full(dist.shape, ground, dtype=np.int32)
        h[dist <= half_bottom] = bottom
        boundary, base = half_bottom, bottom
        for f in range(num_flights):
            m = (dist > boundary) & (dist <= boundary + flight)
            step_idx = np.clip((dist[m] - boundary - 1) // step_depth, 0, steps_per_flight - 1)
            h[m] = base + (step_idx + 1) * sh
            base += steps_per_flight * sh
            boundary += flight
            if f < num_flights - 1:
                h[(dist > boundary) & (dist <= boundary + flat_landing)] = base
                boundary += flat_landing
        hf = np.minimum(hf, h.astype(np.int16))                                           # the well cuts into the ground
        spawns[level] = {"center": (cx * h_scale + origin[0], cy * h_scale + origin[1], bottom * v_scale), "step_height_m": float(step_heights_m[level])}
    info = {"heightfield": hf, "horizontal_scale": h_scale, "vertical_scale": v_scale, "terrain_origin": origin,
            "total_x_m": total_x * h_scale, "total_y_m": total_y * h_scale, "num_difficulty_levels": num_levels, "well_spawns": spawns,
            "step_heights_m": step_heights_m.tolist(), "ground_height_m": ground * v_scale, "steps_per_flight": steps_per_flight,
            "num_flights_per_side": num_flights, "step_depth_m": step_depth_m}
    return hf, info


def well_centers(info):
    """[(x, y, bottom_z)] by level: what the env's row-centre table holds."""
    return [tuple(info["well_spawns"][lvl]["center"]) for lvl in range(info["num_difficulty_levels"])]


def well_scan_axes(terrain_cfg):
    """The two axes of the privileged height scan as the reference forms them (go2_env_stair6_Omni.py:384-393): float32 torch.linspace values."""
    import torch

    hs = terrain_cfg.get("height_scan", {})
    nx, ny = int(hs.get("num_x", 11)), int(hs.get("num_y", 11))
    xr, yr = hs.get("x_range", [-0.5, 0.5]), hs.get("y_range", [-0.5, 0.5])
    return (np.ascontiguousarray(torch.linspace(float(xr[0]), float(xr[1]), nx).numpy(), dtype=np.float32),
            np.ascontiguousarray(torch.linspace(float(yr[0]), float(yr[1]), ny).numpy(), dtype=np.float32))
