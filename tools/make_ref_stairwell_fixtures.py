"""Golden fixtures of the stairwell env from the reference's OWN code (needs a checkout of the reference project; nothing of it is stored here).

    GO2SIM_REFERENCE_DIR=<reference checkout> python tools/make_ref_stairwell_fixtures.py
        -> tests/golden/ref_wells.npz, tests/golden/ref_cfgs_stairwell.json

examples/locomotion/go2_env_stair6_Omni.py is loaded where it lies (importlib, on the repository's `genesis` alias package, as the other fixture
tools load the env files).  No env is built -- the class needs a scene -- so `Go2Env._get_terrain_height`, `_compute_height_scan`, `_assign_wells`
and `_get_spawn_pos` are called as unbound methods on a plain namespace object that carries the attributes they read (`_use_terrain`, `_terrain_origin`,
`_h_scale`, `_hf_heights`, `_scan_n`, `_scan_local_x / _y`, `base_pos`, `base_quat`, `num_envs`, `device`, `_num_difficulty_levels`, `_env_well_level`,
`_well_spawns`, `base_init_pos`), and the module's global `gs` is a namespace with `device` and `tc_float`.  Every line that runs is the reference's.

Recorded, data only:
  * `build_stairwell_terrain` on the three configurations of tests/wells_cases.py: the int16 field, the well centres, origin, ground height, step heights;
  * `_compute_height_scan` with the 11 x 11 grid on the poses of wells_cases.poses over terrain (a);
  * `_assign_wells` and `_get_spawn_pos` for 20 envs at three curriculum levels with torch.randint / torch.randperm and random.uniform replaced by a
    constant schedule: a uniform in [0, 1) is the next value of wells_cases.U_CYCLE, randint(lo, hi) = lo + int(u (hi - lo)), uniform(a, b) = a + (b - a) u
    (python's own formula), randperm(n) a fixed permutation.  The schedule's values are recorded next to the results.
  * the dictionaries of go2_stair_train6_Omni.py's `get_cfgs()` / `get_train_cfg()` (the script is loaded with rsl_rl and its env file stubbed out)."""
import importlib.util
import io
import json
import os
import sys
import types
from contextlib import redirect_stdout
from importlib import metadata

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_ROOT = os.environ.get("GO2SIM_REFERENCE_DIR")
OUT = os.path.join(ROOT, "tests", "golden", "ref_wells.npz")
OUT_CFGS = os.path.join(ROOT, "tests", "golden", "ref_cfgs_stairwell.json")
N_SPAWN, LEVELS = 20, (0.0, 0.7, 1.0)
BASE_INIT_Z = 0.42


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    with redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


class Schedule:
    """The constant schedule of the module docstring; `log` keeps what was handed out."""

    def __init__(self, cycle):
        self.cycle, self.k, self.log = cycle, 0, []

    def u(self):
        v = float(self.cycle[self.k % len(self.cycle)])
        self.k += 1
        self.log.append(v)
        return v

    def uniform(self, a, b):
        return a + (b - a) * self.u()

    def randint(self, lo, hi, size=(), device=None):
        return torch.tensor([lo + int(self.u() * (hi - lo)) for _ in range(size[0])], dtype=torch.long)

    @staticmethod
    def randperm(n, device=None):
        return torch.from_numpy(np.roll(np.arange(n)[::-1], 3).copy())


class PatchedTorch:
    """Stands in for the global `torch` of the loaded module: randint and randperm come from the schedule, every other attribute is torch's."""

    def __init__(self, sched):
        self._s = sched

    def __getattr__(self, name):
        return getattr(torch, name)

    def randint(self, lo, hi, size=(), device=None):
        return self._s.randint(lo, hi, size)

    def randperm(self, n, device=None):
        return self._s.randperm(n)


def make_wells():
    import wells_cases as WC

    mod = load(os.path.join(REF_ROOT, "examples", "locomotion", "go2_env_stair6_Omni.py"), "ref_go2_env_stair6_omni")
    mod.gs = types.SimpleNamespace(device="cpu", tc_float=torch.float32)
    E = mod.Go2Env
    data = {"u_cycle": WC.U_CYCLE}
    built = {}
    for name, tcfg in WC.TERRAINS.items():
        with redirect_stdout(io.StringIO()):
            hf, info = mod.build_stairwell_terrain(dict(tcfg))
        built[name] = (hf, info)
        n = info["num_difficulty_levels"]
        data.update({f"{name}_hf": np.asarray(hf), f"{name}_centers": np.array([info["well_spawns"][k]["center"] for k in range(n)], np.float64),
                     f"{name}_origin": np.asarray(info["terrain_origin"], np.float64), f"{name}_ground_height_m": np.float64(info["ground_height_m"]),
                     f"{name}_step_heights_m": np.asarray(info["step_heights_m"], np.float64),
                     f"{name}_total_m": np.array([info["total_x_m"], info["total_y_m"]], np.float64)})
        assert np.asarray(hf).dtype == np.int16

    # ---- the scan on terrain (a) ----
    hf, info = built["a"]
    env = types.SimpleNamespace()
    env._use_terrain, env.device = True, "cpu"
    env._terrain_origin, env._h_scale = info["terrain_origin"], info["horizontal_scale"]
    env._hf_heights = torch.tensor(hf, dtype=torch.float32) * info["vertical_scale"]
    g = WC.SCAN_11
    gx, gy = torch.meshgrid(torch.linspace(float(g["x_range"][0]), float(g["x_range"][1]), g["num_x"]),
                            torch.linspace(float(g["y_range"][0]), float(g["y_range"][1]), g["num_y"]), indexing="ij")
    env._scan_local_x, env._scan_local_y, env._scan_n = gx.reshape(-1), gy.reshape(-1), g["num_x"] * g["num_y"]
    env._get_terrain_height = lambda x, y: E._get_terrain_height(env, x, y)
    pos, quat = WC.poses(24, info, seed=1)
    env.num_envs, env.base_pos, env.base_quat = len(pos), torch.from_numpy(pos), torch.from_numpy(quat)
    data.update(scan_pos=pos, scan_quat=quat, scan=E._compute_height_scan(env).numpy().astype(np.float32),
                scan_xs=torch.linspace(float(g["x_range"][0]), float(g["x_range"][1]), g["num_x"]).numpy(),
                scan_ys=torch.linspace(float(g["y_range"][0]), float(g["y_range"][1]), g["num_y"]).numpy())

    # ---- assignment and spawn on terrain (a) with the constant schedule ----
    env._num_difficulty_levels, env._well_spawns = info["num_difficulty_levels"], info["well_spawns"]
    env.base_init_pos = torch.tensor([0.0, 0.0, BASE_INIT_Z])
    idx = torch.arange(N_SPAWN)
    for k, level in enumerate(LEVELS):
        sched = Schedule(WC.U_CYCLE)
        mod.torch = PatchedTorch(sched)
        mod.random = types.SimpleNamespace(uniform=sched.uniform)
        env._env_well_level = torch.zeros(N_SPAWN, dtype=torch.long)
        E._assign_wells(env, idx, level)
        n_assign = sched.k
        spawn = E._get_spawn_pos(env, idx)
        data.update({f"spawn{k}_level": np.float64(level), f"spawn{k}_levels": env._env_well_level.numpy().copy(), f"spawn{k}_pos": spawn.numpy().astype(np.float32),
                     f"spawn{k}_u": np.asarray(sched.log, np.float64), f"spawn{k}_n_assign_draws": np.int64(n_assign),
                     f"spawn{k}_perm": Schedule.randperm(N_SPAWN).numpy()})
    data["spawn_base_init_z"] = np.float64(BASE_INIT_Z)
    np.savez_compressed(OUT, **data)
    print(f"-> {OUT} ({os.path.getsize(OUT)} bytes)")


def make_cfgs():
    script = os.path.join(REF_ROOT, "examples", "locomotion", "go2_stair_train6_Omni.py")
    stubs = {"rsl_rl": types.ModuleType("rsl_rl"), "rsl_rl.runners": types.ModuleType("rsl_rl.runners"), "go2_env_stair6_Omni": types.ModuleType("go2_env_stair6_Omni")}
    stubs["rsl_rl.runners"].OnPolicyRunner = stubs["go2_env_stair6_Omni"].Go2Env = None
    real_version = metadata.version

    def version(name):
        if name == "rsl-rl-lib":
            return "2.2.4"
        if name == "rsl-rl":
            raise metadata.PackageNotFoundError(name)
        return real_version(name)

    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    metadata.version = version
    try:
        mod = load(script, "ref_train_stairwell")
        with redirect_stdout(io.StringIO()):
            env_cfg, obs_cfg, reward_cfg, command_cfg = mod.get_cfgs()
        out = {"source": "examples/locomotion/go2_stair_train6_Omni.py get_cfgs()", "layout": ["env_cfg", "obs_cfg", "reward_cfg", "command_cfg", "train_cfg"],
               "env_cfg": env_cfg, "obs_cfg": obs_cfg, "reward_cfg": reward_cfg, "command_cfg": command_cfg,
               "train_cfg": mod.get_train_cfg("go2-stairwell-omni-v1", 10000)}                    # (the script's argument defaults)
        with open(OUT_CFGS, "w") as f:
            json.dump(out, f, indent=1)   # insertion order kept: the order of reward_scales is the evaluation order of the reward terms
            f.write("\n")
        print(f"{script} -> {OUT_CFGS} ({os.path.getsize(OUT_CFGS)} bytes)")
    finally:
        metadata.version = real_version
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


if __name__ == "__main__":
    if not REF_ROOT:
        raise SystemExit("set GO2SIM_REFERENCE_DIR to a checkout of the reference project")
    make_wells()
    make_cfgs()
