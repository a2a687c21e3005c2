#!/usr/bin/env python3
"""Build-container script: turn the reference-held config pickles into JSON fixtures.

    python tools/make_ref_cfg_fixtures.py        # reads /root/reference/logs/<exp>/cfgs.pkl, writes tests/golden/ref_cfgs_<task>.json

`logs/<exp>/cfgs.pkl` is what go2_train_*.py writes next to its checkpoints (go2_train_walk.py:462-465): the 5-element list
[env_cfg, obs_cfg, reward_cfg, command_cfg, train_cfg] of plain dicts / lists / strings / numbers.  They are the only reference-held data
on this path.  The files are read with an unpickler that refuses every global (`find_class` raises), i.e. nothing
from the file is executed or imported; a pickle that needs a global makes the script fail instead of loading it.  The JSON fixtures are
data (inputs of the env), not reference source text.  The rough-terrain run has no log directory: `rough_cfgs()` below takes its dictionaries from the
train script's own `get_cfgs()` (`--rough-only` makes those two fixtures alone).  /root/reference does not exist on the GPU box: tests read only the JSON."""
import io
import json
import os
import pickle
import sys

REF_LOGS = "/root/reference/logs"
OUT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
TASKS = {"walk": "go2-walk", "stairs": "go2-stairs", "jump": "go2-jump", "crouch": "go2-crouch"}


class NoGlobalsUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        raise pickle.UnpicklingError(f"refusing global {module}.{name}: config pickles hold plain containers only")


def load_plain_pickle(path):
    with open(path, "rb") as f:
        return NoGlobalsUnpickler(io.BytesIO(f.read())).load()


ROUGH_SCRIPT = os.path.join(os.path.dirname(REF_LOGS), "examples", "locomotion", "go2_train_Omni_kplearn_varied_terrain.py")
ROUGH_NUMPY_SEED = 3


def rough_cfgs():
    """The rough-terrain fine-tuning run has no log directory: its dictionaries come from the train script's own `get_cfgs()`, for both values of its
    TERRAIN_MODE.  The script is loaded where it lies with the modules it imports for training stubbed out (rsl_rl, its env file) and the version
    check of its first lines answered; only `get_cfgs` runs.  The heightmap (300 x 300 floats drawn from numpy's global generator, seeded here) is
    recorded as shape and SHA-256 of its float32 bytes: tests/golden/ref_cfgs_rough_<mode>.json."""
    import hashlib
    import importlib.util
    import types
    from contextlib import redirect_stdout
    from importlib import metadata

    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT_DIR)))                        # the repository root: the `genesis` alias package
    stubs = {"rsl_rl": types.ModuleType("rsl_rl"), "rsl_rl.runners": types.ModuleType("rsl_rl.runners"),
             "go2_env_Omni_kplearn_varied_terrain": types.ModuleType("go2_env_Omni_kplearn_varied_terrain")}
    stubs["rsl_rl.runners"].OnPolicyRunner = stubs["go2_env_Omni_kplearn_varied_terrain"].Go2Env = None
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
        spec = importlib.util.spec_from_file_location("ref_train_rough", ROUGH_SCRIPT)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        for mode in ("heightmap", "grid"):
            mod.TERRAIN_MODE = mode
            np.random.seed(ROUGH_NUMPY_SEED)
            with redirect_stdout(io.StringIO()):
                env_cfg, obs_cfg, reward_cfg, command_cfg = mod.get_cfgs()
            terrain = dict(env_cfg["terrain"])
            if "height_field" in terrain:
                hf = np.ascontiguousarray(terrain["height_field"])
                assert hf.dtype == np.float32
                terrain["height_field"] = {"shape": list(hf.shape), "sha256": hashlib.sha256(hf.tobytes()).hexdigest(), "min": float(hf.min()), "max": float(hf.max())}
            env_cfg = dict(env_cfg, terrain=terrain)
            out = {"source": "examples/locomotion/go2_train_Omni_kplearn_varied_terrain.py get_cfgs()", "terrain_mode": mode, "numpy_seed": ROUGH_NUMPY_SEED,
                   "layout": ["env_cfg", "obs_cfg", "reward_cfg", "command_cfg", "train_cfg"], "env_cfg": env_cfg, "obs_cfg": obs_cfg, "reward_cfg": reward_cfg,
                   "command_cfg": command_cfg, "train_cfg": mod.get_train_cfg("go2-terrain-v1", 220000)}     # (the script's default name, its usage line's count)
            dst = os.path.join(OUT_DIR, f"ref_cfgs_rough_{mode}.json")
            with open(dst, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
            print(f"{ROUGH_SCRIPT} [{mode}] -> {dst} ({os.path.getsize(dst)} bytes)")
    finally:
        metadata.version = real_version
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    if "--rough-only" in sys.argv:
        return rough_cfgs()
    for task, exp in TASKS.items():
        src = os.path.join(REF_LOGS, exp, "cfgs.pkl")
        cfgs = load_plain_pickle(src)
        assert isinstance(cfgs, (list, tuple)) and len(cfgs) == 5, f"{src}: expected [env, obs, reward, command, train]"
        out = {"source": f"logs/{exp}/cfgs.pkl", "layout": ["env_cfg", "obs_cfg", "reward_cfg", "command_cfg", "train_cfg"],
               "env_cfg": cfgs[0], "obs_cfg": cfgs[1], "reward_cfg": cfgs[2], "command_cfg": cfgs[3], "train_cfg": cfgs[4]}
        dst = os.path.join(OUT_DIR, f"ref_cfgs_{task}.json")
        with open(dst, "w") as f:
            json.dump(out, f, indent=1)   # insertion order kept: the order of reward_scales is the evaluation order of the reward terms
            f.write("\n")
        print(f"{src} -> {dst} ({os.path.getsize(dst)} bytes)")
    rough_cfgs()


if __name__ == "__main__":
    sys.exit(main())
