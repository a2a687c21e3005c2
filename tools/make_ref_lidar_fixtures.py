"""Golden fixture of the LIDAR scan from the reference's OWN methods (needs a checkout of the reference project; nothing of it is stored here).

    GO2SIM_REFERENCE_DIR=<reference checkout> python tools/make_ref_lidar_fixtures.py      # writes tests/golden/ref_lidar_scan.npz

examples/locomotion/go2_env_stair_lidar.py is loaded where it lies (importlib, on the repository's `genesis` alias package, as
tools/make_ref_env_fixtures.py loads the env files).  No env is built: the reference's `LidarScanConfig` is constructed from the lidar cfg, and
`Go2Env._get_terrain_height`, `_compute_lidar_scan`, `_update_actor_lidar_scan` and `_update_critic_lidar_scan` are called as unbound methods on a
plain namespace object that carries the attributes they read (`_lidar`, `_use_terrain`, `_terrain_origin`, `_h_scale`, `_hf_heights`, `base_pos`,
`base_quat`, `num_envs`, `device`, `_lidar_noise_level`, the three scan buffers).  Every line of the scan that runs is the reference's.

Random numbers: the loaded module's global `torch` is replaced by a forwarder whose randn_like / rand_like / randn / rand return, in the order the
reference calls them (z [n][k], u [n][k], z_b [n][1], u_lat [n], u_black [n]), the draws of include/go2sim_lidar.h's layout for (seed, step), computed
by the numpy restatement of Philox in tests/lidar_ref.py; the tool asserts that each step consumed exactly those five.

The three reset lines of the reference's reset_idx (go2_env_stair_lidar.py:1777-1781: the actor buffer, its previous copy and the critic buffer of
the reset envs become 0) sit in a method that needs the whole env; THIS TOOL APPLIES THEM ITSELF after the two updates of a step, where `step` calls
reset_idx.

Recorded: 8 envs x 6 steps on the 40 x 30 test heightfield of tests/lidar_cases.py, default grids, the default noise at L = 0.7, in two blocks
(height_scale 1 and 0.5): inputs (heightfield, origin, scales, poses, reset flags, level, constants, seed), the draws, and both scan buffers after
every step.  The seed is chosen so that dropout, a stale row that repeats a non-zero scan, a blackout, a clipped cell and a reset all occur in each
block; the tool asserts it."""
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
OUT = os.path.join(ROOT, "tests", "golden", "ref_lidar_scan.npz")
N_ENVS, LEVEL, SEED = 8, 0.7, 5
BLOCKS = (("s1", 1.0), ("s05", 0.5))


class DrawTorch:
    """Stands in for the global `torch` of the loaded module: the four random functions hand out the queued draws, every other attribute is torch's."""

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

    def rand_like(self, t):
        return self._next("rand_like", t.shape)

    def randn(self, *size, **kw):
        return self._next("randn", size)

    def rand(self, *size, **kw):
        return self._next("rand", size)


def load_reference_module():
    path = os.path.join(REF_ROOT, "examples", "locomotion", "go2_env_stair_lidar.py")
    spec = importlib.util.spec_from_file_location("ref_go2_env_stair_lidar", path)
    mod = importlib.util.module_from_spec(spec)
    with redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def run_block(mod, scale):
    import lidar_cases as LC
    import lidar_ref as R

    cfg = LC.lidar_cfg("5x3_9x5", scale=scale)
    with redirect_stdout(io.StringIO()):
        lidar = mod.LidarScanConfig(cfg, "cpu")
    env = types.SimpleNamespace()
    E = mod.Go2Env
    env._lidar, env._use_terrain, env.num_envs, env.device = lidar, True, N_ENVS, "cpu"
    env._terrain_origin, env._h_scale = LC.ORIGIN, LC.H_SCALE
    hf = LC.heightfield()
    env._hf_heights = torch.tensor(hf, dtype=torch.float32) * LC.V_SCALE
    env._lidar_noise_level = LEVEL
    env._actor_scan_buf = torch.zeros(N_ENVS, lidar.num_actor_scan)
    env._actor_scan_prev = torch.zeros_like(env._actor_scan_buf)
    env._critic_scan_buf = torch.zeros(N_ENVS, lidar.num_critic_scan)
    env._get_terrain_height = lambda x, y: E._get_terrain_height(env, x, y)
    env._compute_lidar_scan = lambda lx, ly, n: E._compute_lidar_scan(env, lx, ly, n)
    fake = mod.torch = DrawTorch()
    pos, quat = LC.poses(N_ENVS, LC.STEPS, SEED)
    reset = LC.resets(N_ENVS, LC.STEPS)
    rec = {"actor": [], "critic": [], "z": [], "u": [], "z_b": [], "u_lat": [], "u_black": []}
    fired = {"dropout": 0, "stale_nonzero": 0, "blackout": 0, "clipped": 0, "reset": 0}
    noise = cfg["noise"]
    for t in range(LC.STEPS):
        d = R.draws(N_ENVS, lidar.num_actor_scan, SEED, t)
        fake.queue = [("randn_like", d["z"]), ("rand_like", d["u"]), ("randn", d["z_b"][:, None]), ("rand", d["u_lat"]), ("rand", d["u_black"])]
        env.base_pos, env.base_quat = torch.from_numpy(pos[t]), torch.from_numpy(quat[t])
        prev = env._actor_scan_buf.clone()
        E._update_actor_lidar_scan(env)
        E._update_critic_lidar_scan(env)
        assert not fake.queue, "the reference did not consume the step's five draws"
        idx = torch.from_numpy(np.flatnonzero(reset[t]))
        env._actor_scan_buf[idx] = 0.0                       # go2_env_stair_lidar.py:1779-1781, applied here (module docstring)
        env._actor_scan_prev[idx] = 0.0
        env._critic_scan_buf[idx] = 0.0
        live = reset[t] == 0
        lat = (d["u_lat"].astype(np.float32) < R.threshold(noise["latency_prob"], LEVEL)) & live
        black = (d["u_black"].astype(np.float32) < R.threshold(noise["full_blackout_prob"], LEVEL)) & live
        fired["dropout"] += int(((d["u"].astype(np.float32) < R.threshold(noise["dropout_prob"], LEVEL)) & live[:, None]).sum())
        fired["stale_nonzero"] += int(((prev.numpy() != 0).any(1) & lat & ~black).sum())
        fired["blackout"] += int(black.sum())
        fired["clipped"] += int((env._actor_scan_buf.abs().numpy() == np.float32(cfg["height_clip"] * scale)).sum())
        fired["reset"] += int(reset[t].sum())
        rec["actor"].append(env._actor_scan_buf.numpy().copy()); rec["critic"].append(env._critic_scan_buf.numpy().copy())
        for k in ("z", "u", "z_b", "u_lat", "u_black"):
            rec[k].append(d[k].astype(np.float32))
    assert all(v > 0 for v in fired.values()), f"a branch did not fire: {fired}"
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(pos=pos, quat=quat, reset=reset)
    return out, fired


def make():
    import lidar_cases as LC

    mod = load_reference_module()
    cfg = LC.lidar_cfg("5x3_9x5")
    data = {"hf": LC.heightfield(), "origin": np.asarray(LC.ORIGIN, np.float64), "h_scale": np.float64(LC.H_SCALE), "v_scale": np.float64(LC.V_SCALE),
            "level": np.float64(LEVEL), "seed": np.int64(SEED), "height_clip": np.float64(cfg["height_clip"]),
            "noise_names": np.array(sorted(cfg["noise"])), "noise_values": np.array([cfg["noise"][k] for k in sorted(cfg["noise"])], np.float64)}
    for name, scale in BLOCKS:
        block, fired = run_block(mod, scale)
        print(f"block {name} (height_scale {scale}): {fired}")
        data[name + "_height_scale"] = np.float64(scale)
        for k, v in block.items():
            data[f"{name}_{k}"] = v
    return data


def main():
    if not REF_ROOT:
        raise SystemExit("set GO2SIM_REFERENCE_DIR to a checkout of the reference project")
    data = make()
    np.savez(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
