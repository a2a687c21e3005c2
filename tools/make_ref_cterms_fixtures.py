"""Golden fixtures of the two contact terms from the reference's OWN code (needs a checkout of the reference project; nothing of it is stored here).

    GO2SIM_REFERENCE_DIR=<reference checkout> python tools/make_ref_cterms_fixtures.py
        -> tests/golden/ref_cterms.npz, tests/golden/ref_cfgs_stair_info.json

examples/locomotion/go2_env_stair_lidar_2.py and examples/locomotion/go2_env_terrain.py are loaded where they lie (importlib, on the repository's
`genesis` alias package, as the other fixture tools load the env files; the terrain env's `terrain_manager` import is met by the reference's own file
next to it).  No env is built -- the classes need a scene -- so `Go2Env._init_body_contact_tracking`, `Go2Env._reward_body_contact` and
`Go2Env._reward_stumble` are called as unbound methods on a plain namespace object that carries the attributes they read (`env_cfg`, `reward_cfg`,
`num_envs`, `device`, `_has_body_contact_penalty`, `_body_contact_link_indices`, `_has_foot_contact_rewards`, `_foot_link_indices`) and a stand-in
`robot` whose `links` carry the model's names and whose `get_links_net_contact_force()` returns the table's force tensor; the modules' global `gs`
is a namespace with `device` and `tc_float`.  Every line of the two laws that runs is the reference's.  The foot link indices the terrain env finds
from `foot_names` in its constructor are set here to the four calf links.

Recorded, arrays only (tests/cterms_ref.py makes the tables):
  * `random`: 300 rows of [13][3] forces of 0 to 50 N at the scripts' thresholds (1 N, 5 N), with body_contact of the two front thighs and stumble;
  * `edge_body` / `edge_stumble`: single-component forces at the threshold and one float32 above it, both signs, x, y and z;
  * `zero`: the random rows' first 100 (and a row of no force at all) at thresholds 0;
  * `special`: NaN and infinite components;
and, as JSON, the dictionaries of go2_stair_train_lidar_2.py's `get_cfgs()` / `get_train_cfg()` (the script is loaded with rsl_rl and its env file
stubbed out): settings only."""
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
OUT = os.path.join(ROOT, "tests", "golden", "ref_cterms.npz")
OUT_CFGS = os.path.join(ROOT, "tests", "golden", "ref_cfgs_stair_info.json")


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    with redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


class Robot:
    def __init__(self, names):
        self.links = [types.SimpleNamespace(name=n) for n in names]
        self.cf = None

    def get_links_net_contact_force(self):
        return self.cf


def make_terms():
    import cterms_ref as R

    loco = os.path.join(REF_ROOT, "examples", "locomotion")
    sys.path.insert(0, loco)                                              # go2_env_terrain.py imports its sibling terrain_manager
    try:
        stair = load(os.path.join(loco, "go2_env_stair_lidar_2.py"), "ref_go2_env_stair_lidar_2")
        rough = load(os.path.join(loco, "go2_env_terrain.py"), "ref_go2_env_terrain")
    finally:
        sys.path.remove(loco)
    stair.gs = rough.gs = types.SimpleNamespace(device="cpu", tc_float=torch.float32)
    robot = Robot(R.ROBOT_LINKS)

    def run(F, body_thr, stumble_thr):
        F = np.ascontiguousarray(F, np.float32)
        robot.cf = torch.from_numpy(F)
        env = types.SimpleNamespace(robot=robot, num_envs=len(F), device="cpu", env_cfg={"body_contact_names": ["FR_thigh", "FL_thigh"], "body_contact_threshold": body_thr},
                                    reward_cfg={"stumble_threshold": stumble_thr}, _has_body_contact_penalty=True, _body_contact_link_indices=[],
                                    _has_foot_contact_rewards=True, _foot_link_indices=[R.ROBOT_LINKS.index(n) for n in R.ROBOT_LINKS if n.endswith("_calf")])
        with redirect_stdout(io.StringIO()):
            stair.Go2Env._init_body_contact_tracking(env)
            assert tuple(env._body_contact_link_indices) == R.THIGHS and env._has_body_contact_penalty
            count = stair.Go2Env._reward_body_contact(env)
            pen = rough.Go2Env._reward_stumble(env)
        assert count.dtype == torch.float32 and pen.dtype == torch.float32
        return count.numpy().copy(), pen.numpy().copy()

    rand = R.random_rows(300, seed=7)
    eb, eb_over = R.edge_rows(R.BODY_THRESHOLD, R.THIGHS)
    es, es_over = R.edge_rows(R.STUMBLE_THRESHOLD, (R.NON_FEET[0], R.NON_FEET[-1]))
    zero = np.concatenate([rand[:100], np.zeros((1,) + rand.shape[1:], np.float32)])
    blocks = {"random": (rand, R.BODY_THRESHOLD, R.STUMBLE_THRESHOLD), "edge_body": (eb, R.BODY_THRESHOLD, R.STUMBLE_THRESHOLD),
              "edge_stumble": (es, R.BODY_THRESHOLD, R.STUMBLE_THRESHOLD), "zero": (zero, 0.0, 0.0), "special": (R.special_rows(), R.BODY_THRESHOLD, R.STUMBLE_THRESHOLD)}
    data = {"robot_links": np.array(R.ROBOT_LINKS), "body_links": np.array(R.THIGHS, np.int64), "stumble_links": np.array(R.NON_FEET, np.int64),
            "edge_body_over": eb_over, "edge_stumble_over": es_over}
    for name, (F, tb, ts) in blocks.items():
        count, pen = run(F, tb, ts)
        data.update({f"{name}_forces": F, f"{name}_body_threshold": np.float64(tb), f"{name}_stumble_threshold": np.float64(ts),
                     f"{name}_body_contact": count, f"{name}_stumble": pen})
        if name != "special":
            R.check_ambiguity_cap(F, R.THIGHS, tb)
        print(f"{name}: {len(F)} rows, body_contact counts {np.unique(count[np.isfinite(count)]).tolist()}, stumble max {np.nanmax(np.where(np.isfinite(pen), pen, np.nan)):.3f}")
    assert np.array_equal(data["edge_body_body_contact"], eb_over.astype(np.float32)), "the reference's `>` at the threshold's edges"
    assert np.array_equal(data["edge_stumble_stumble"] > 0, es_over)
    np.savez_compressed(OUT, **data)
    print(f"-> {OUT} ({os.path.getsize(OUT)} bytes)")


def make_cfgs():
    script = os.path.join(REF_ROOT, "examples", "locomotion", "go2_stair_train_lidar_2.py")
    stubs = {"rsl_rl": types.ModuleType("rsl_rl"), "rsl_rl.runners": types.ModuleType("rsl_rl.runners"), "go2_env_stair_lidar_2": types.ModuleType("go2_env_stair_lidar_2")}
    stubs["rsl_rl.runners"].OnPolicyRunner = stubs["go2_env_stair_lidar_2"].Go2Env = None
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
        mod = load(script, "ref_train_stair_info")
        with redirect_stdout(io.StringIO()):
            env_cfg, obs_cfg, reward_cfg, command_cfg = mod.get_cfgs()
        out = {"source": "examples/locomotion/go2_stair_train_lidar_2.py get_cfgs()", "layout": ["env_cfg", "obs_cfg", "reward_cfg", "command_cfg", "train_cfg"],
               "env_cfg": env_cfg, "obs_cfg": obs_cfg, "reward_cfg": reward_cfg, "command_cfg": command_cfg,
               "train_cfg": mod.get_train_cfg("go2-stair-info", 10000)}
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
    make_terms()
    make_cfgs()
