"""Golden fixture of the four-value stair info from the reference's OWN code (needs a checkout of the reference project; nothing of it is stored here).

    GO2SIM_REFERENCE_DIR=<reference checkout> python tools/make_ref_stairinfo_fixtures.py      # writes tests/golden/ref_stair_info.npz

examples/locomotion/go2_env_stair_lidar_2.py is loaded where it lies (importlib, on the repository's `genesis` alias package, as
tools/make_ref_lidar_fixtures.py loads its sibling).  No env is built:
  * the reference's own `build_stair_terrain` builds the small terrain of tests/stairinfo_cases.py with numpy's global generator seeded, and the depths
    it shuffled are recorded (`step_depths_m`), with the heightfield and the row centres;
  * the reference's `StairInfoConfig` is constructed from the stair_info cfg, and `Go2Env._get_terrain_height`, `_compute_edge_detection` and
    `_update_stair_info` are called as unbound methods on a plain namespace object that carries the attributes they read.  Every line of the
    detector and of the noise model that runs is the reference's.

Random numbers: the loaded module's global `torch` is replaced by a forwarder whose randn_like / rand return, in the order the reference calls them
(z_e, z_h, z_d by randn_like; u_flip, u_lat, u_black by rand), the draws of include/go2sim_stairinfo.h's layout for (seed, step), computed by the numpy
restatement of Philox in tests/stairinfo_ref.py; the tool asserts that each step consumed exactly those six.

The three reset lines of the reference's reset_idx (go2_env_stair_lidar_2.py:1705-1707: the actor buffer, its previous copy and the clean buffer of
the reset envs become 0) sit in a method that needs the whole env; THIS TOOL APPLIES THEM ITSELF after the update of a step, where `step` calls
reset_idx.

Recorded: 8 envs x 6 steps at L = 0.7 in three blocks (edge_dist_scale 3.7 and 1 at the default threshold 0.02, which row 0's riser equals and never
exceeds; edge_dist_scale 3.7 at threshold 0.105, which row 3's riser equals and its third step exceeds by float32 rounding): inputs (poses, terrain rows, reset flags, level, constants, seed),
the draws, and both buffers after every step.  The three probabilities are raised (tests/stairinfo_cases.py NOISE_BUSY) and the seed is chosen so
that in each block an edge up, an edge down, no edge, the threshold riser (not seen; in the third block also seen), both clamps of the noisy edge, a
flip, a stale row that repeats a non-zero edge, a blackout and a reset all occur; the tool asserts it."""
import importlib.util
import io
import os
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("GO2SIM_REFERENCE_DIR")
OUT = os.path.join(ROOT, "tests", "golden", "ref_stair_info.npz")
N_ENVS, LEVEL, SEED, NUMPY_SEED = 8, 0.7, 50, 4
BLOCKS = (("s37", 3.7, 0.02), ("s1", 1.0, 0.02), ("t105", 3.7, 0.105))      # (name, edge_dist_scale, threshold)
DRAW_KEYS = ("z_e", "z_h", "z_d", "u_flip", "u_lat", "u_black")


class DrawTorch:
    """Stands in for the global `torch` of the loaded module: the random functions hand out the queued draws, every other attribute is torch's."""

    def __init__(self):
        self.queue = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _next(self, kind, shape):
        want, arr = self.queue.pop(0)
        assert want == kind and tuple(arr.shape) == tuple(shape), (want, kind, arr.shape, shape)
        return torch.from_numpy(arr.astype(np.float32))

    def randn_like(self, t):
        return self._next("randn_like", t.shape)

    def rand(self, *size, **kw):
        return self._next("rand", size)


def load_reference_module():
    path = os.path.join(REF_ROOT, "examples", "locomotion", "go2_env_stair_lidar_2.py")
    spec = importlib.util.spec_from_file_location("ref_go2_env_stair_lidar_2", path)
    mod = importlib.util.module_from_spec(spec)
    with redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def reference_terrain(mod):
    import stairinfo_cases as SC

    np.random.seed(NUMPY_SEED)                                   # the reference shuffles the depths with the global generator
    with redirect_stdout(io.StringIO()):
        hf, info = mod.build_stair_terrain(dict(SC.TERRAIN_CFG))
    return hf, info


def run_block(mod, hf, info, scale, thr):
    import stairinfo_cases as SC
    import stairinfo_ref as R

    cfg = SC.stair_info_cfg(14, edge_dist_scale=scale, threshold=thr)
    with redirect_stdout(io.StringIO()):
        scfg = mod.StairInfoConfig(cfg, "cpu")
    env = types.SimpleNamespace()
    E = mod.Go2Env
    env._stair_cfg, env._use_terrain, env.num_envs, env.device = scfg, True, N_ENVS, "cpu"
    env._terrain_origin, env._h_scale = info["terrain_origin"], info["horizontal_scale"]
    env._hf_heights = torch.tensor(hf, dtype=torch.float32) * info["vertical_scale"]                  # go2_env_stair_lidar_2.py:466-473
    env._terrain_step_heights_t = torch.tensor(info["step_heights_m"], dtype=torch.float32)
    env._terrain_step_depths_t = torch.tensor(info["step_depths_m"], dtype=torch.float32)
    env._stair_noise_level = LEVEL
    env._stair_info_buf = torch.zeros(N_ENVS, 4)
    env._stair_info_prev = torch.zeros_like(env._stair_info_buf)
    env._stair_info_clean = torch.zeros_like(env._stair_info_buf)
    env._get_terrain_height = lambda x, y: E._get_terrain_height(env, x, y)
    env._compute_edge_detection = lambda: E._compute_edge_detection(env)
    fake = mod.torch = DrawTorch()
    xs = scfg.edge_sample_x.numpy()
    pos, quat, names = SC.poses(N_ENVS, SC.STEPS, SEED, xs, info["step_depths_m"], thr_row=3 if thr > 0.1 else 0)
    rows = np.clip(SC.terrain_rows(N_ENVS, SC.STEPS, SEED), 0, 3)      # torch indexing does not clamp: the fixture stays inside the table
    reset = SC.resets(N_ENVS, SC.STEPS)
    rec = {"actor": [], "clean": [], **{k: [] for k in DRAW_KEYS}}
    fired = {k: 0 for k in ("up", "down", "none", "threshold_seen", "threshold_not_seen", "clamp_lo", "clamp_hi", "flip", "stale_nonzero", "blackout", "reset")}
    nz = cfg["noise"]
    top = np.float32(np.float32(0.27) * np.float32(scale))
    for t in range(SC.STEPS):
        d = R.draws(N_ENVS, SEED, t)
        fake.queue = [("randn_like", d["z_e"]), ("randn_like", d["z_h"]), ("randn_like", d["z_d"]), ("rand", d["u_flip"]), ("rand", d["u_lat"]), ("rand", d["u_black"])]
        env.base_pos, env.base_quat = torch.from_numpy(pos[t]), torch.from_numpy(quat[t])
        env._env_terrain_row = torch.from_numpy(rows[t].astype(np.int64))
        prev = env._stair_info_buf.clone().numpy()
        E._update_stair_info(env)
        assert not fake.queue, "the reference did not consume the step's six draws"
        idx = torch.from_numpy(np.flatnonzero(reset[t]))
        env._stair_info_buf[idx] = 0.0                        # go2_env_stair_lidar_2.py:1705-1707, applied here (module docstring)
        env._stair_info_prev[idx] = 0.0
        env._stair_info_clean[idx] = 0.0
        live = reset[t] == 0
        actor, clean = env._stair_info_buf.numpy().copy(), env._stair_info_clean.numpy().copy()
        lat = (d["u_lat"].astype(np.float32) < R.threshold(nz["latency_prob"], LEVEL)) & live
        black = (d["u_black"].astype(np.float32) < R.threshold(nz["full_blackout_prob"], LEVEL)) & live
        plain = live & ~lat & ~black
        fired["up"] += int((clean[live, 3] > 0).sum()); fired["down"] += int((clean[live, 3] < 0).sum()); fired["none"] += int((clean[live, 3] == 0).sum())
        for b in np.flatnonzero(live):
            if names[t][b].startswith("threshold_"):
                fired["threshold_seen" if clean[b, 3] > 0 else "threshold_not_seen"] += 1
        fired["clamp_lo"] += int((actor[plain, 0] == 0).sum())
        fired["clamp_hi"] += int(((actor[plain, 0] == top) & (d["z_e"][plain] > 0)).sum())
        fired["flip"] += int(((d["u_flip"].astype(np.float32) < R.threshold(nz["direction_flip_prob"], LEVEL)) & plain & (clean[:, 3] != 0)).sum())
        fired["stale_nonzero"] += int(((prev[:, 0] != 0) & lat & ~black).sum())
        fired["blackout"] += int(black.sum())
        fired["reset"] += int(reset[t].sum())
        rec["actor"].append(actor); rec["clean"].append(clean)
        for k in DRAW_KEYS:
            rec[k].append(d[k].astype(np.float32))
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(pos=pos, quat=quat, rows=rows, reset=reset)
    return out, fired


def make(check=True):
    import stairinfo_cases as SC

    mod = load_reference_module()
    hf, info = reference_terrain(mod)
    cfg = SC.stair_info_cfg(14)
    scalars = {"max_range": 0.27, "height_scale": cfg["height_scale"], "depth_scale": cfg["depth_scale"],
               "direction_scale": cfg["direction_scale"]}
    data = {"hf": np.asarray(hf), "origin": np.asarray(info["terrain_origin"], np.float64), "h_scale": np.float64(info["horizontal_scale"]),
            "v_scale": np.float64(info["vertical_scale"]), "row_centers": np.asarray(info["row_centers"], np.float64),
            "step_heights_m": np.asarray(info["step_heights_m"], np.float64), "step_depths_m": np.asarray(info["step_depths_m"], np.float64),
            "numpy_seed": np.int64(NUMPY_SEED), "level": np.float64(LEVEL), "seed": np.int64(SEED), "num_samples": np.int64(14),
            "scalar_names": np.array(sorted(scalars)), "scalar_values": np.array([scalars[k] for k in sorted(scalars)], np.float64),
            "noise_names": np.array(sorted(cfg["noise"])), "noise_values": np.array([cfg["noise"][k] for k in sorted(cfg["noise"])], np.float64)}
    for name, scale, thr in BLOCKS:
        block, fired = run_block(mod, hf, info, scale, thr)
        print(f"block {name} (edge_dist_scale {scale}, threshold {thr}): {fired}")
        if check:
            assert all(v > 0 for k, v in fired.items() if k != "threshold_seen" or thr > 0.1), f"a branch did not fire: {fired}"
            assert thr > 0.1 or fired["threshold_seen"] == 0, "a riser equal to the default threshold was taken for an edge"
        data[name + "_edge_dist_scale"], data[name + "_threshold"] = np.float64(scale), np.float64(thr)
        for k, v in block.items():
            data[f"{name}_{k}"] = v
    return data


def main():
    if not REF_ROOT:
        raise SystemExit("set GO2SIM_REFERENCE_DIR to a checkout of the reference project")
    data = make()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
