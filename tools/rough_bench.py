#!/usr/bin/env python
"""Times the rough-terrain walk env (include/go2sim_tiles.h) on the GPU, at the training shape.

    python tools/rough_bench.py [--envs 4096] [--steps 24] [--rounds 10]

The closed collection loop (act, env.step, process_env_step for --steps env steps of an OnPolicyRunner at --envs), taken in one process with the
variants alternating round by round, so that other work on the machine hits all alike:

  collect_ms_walk              the walk env on the plane.urdf box
  collect_ms_stairs            the stair env (int16 stair heightfield, row curriculum, height scan)
  collect_ms_rough_heightmap   the rough env on the train script's 300 x 300 float heightmap
  collect_ms_rough_grid        the rough env on its 2 x 2 tile grid
  collect_ms_rough_grid_host_query
                               the rough grid env, plus what the reference does on top of it every env step: `_query_height_batch` as it
                               stands there -- the base positions copied to the host (one synchronisation), a numpy bilinear lookup, the result
                               copied back -- and its boundary test in torch.  The library has already done both inside its launches; this is the
                               cost the device-side form removes.

Device events bracket each round; every variant is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_runner(task, envs, steps, seed=3):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_rough_cfgs, get_stair_cfgs, get_walk_cfgs, init

    init(seed=seed)
    np.random.seed(seed)
    cfgs = {"walk": get_walk_cfgs, "stairs": get_stair_cfgs, "rough_heightmap": lambda: get_rough_cfgs("heightmap", seed=seed),
            "rough_grid": lambda: get_rough_cfgs("grid")}[task]()
    env = Go2Env(envs, *cfgs, seed=seed)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_cfgs_rough_heightmap.json" if task.startswith("rough") else "ref_cfgs_walk.json")))["train_cfg"]
    cfg["num_steps_per_env"] = steps
    return OnPolicyRunner(env, cfg)


class HostQuery:
    """terrain_manager.py:354-392 and :338-348 as the reference runs them after every env step"""

    def __init__(self, env):
        t = env.terrain
        self.env, self.hf, self.origin, self.hs, self.vs, self.mw = env, t._height_field, t._terrain_origin, t.horizontal_scale, t.vertical_scale, t.max_wander

    def __call__(self):
        env = self.env
        pos = env.base_pos
        hf = self.hf
        rows, cols = hf.shape
        lx = (pos[:, 0].cpu().numpy() - self.origin[0]) / self.hs
        ly = (pos[:, 1].cpu().numpy() - self.origin[1]) / self.hs
        lx, ly = np.clip(lx, 0, rows - 2).astype(np.float64), np.clip(ly, 0, cols - 2).astype(np.float64)
        ix, iy = lx.astype(np.int32), ly.astype(np.int32)
        fx, fy = lx - ix, ly - iy
        h = hf[ix, iy] * (1 - fx) * (1 - fy) + hf[ix + 1, iy] * fx * (1 - fy) + hf[ix, iy + 1] * (1 - fx) * fy + hf[ix + 1, iy + 1] * fx * fy
        ground = torch.tensor(h * self.vs, device=env.device, dtype=torch.float32)
        out = torch.norm(pos[:, :2] - env.terrain._env_spawn_pos[:, :2], dim=1) > self.mw
        return ground, out


def collect(runner, steps, after_step=None):
    """the collection part of OnPolicyRunner.learn: no returns, no update"""
    env, alg = runner.env, runner.alg
    obs, extras = env.get_observations()
    critic_obs = extras["observations"].get("critic", obs)
    for _ in range(steps):
        actions = alg.act(obs, critic_obs)
        obs, rewards, dones, infos = env.step(actions)
        if after_step is not None:
            after_step()
        critic_obs = infos["observations"].get("critic", obs)
        alg.process_env_step(rewards, dones, infos)
    alg.t = 0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=10, help="timed rollouts per variant")
    ap.add_argument("--only", default=None, help="comma-separated variants (e.g. rough_grid for a profiler run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rough_bench.py needs a ROCm GPU (nothing is measured without one)")
    B, T = args.envs, args.steps
    names = ["walk", "stairs", "rough_heightmap", "rough_grid", "rough_grid_host_query"]
    if args.only:
        names = [n for n in names if n in args.only.split(",")]
    runners = {n: make_runner("rough_grid" if n == "rough_grid_host_query" else n, B, T) for n in names}
    hooks = {n: (HostQuery(r.env) if n == "rough_grid_host_query" else None) for n, r in runners.items()}
    for n, r in runners.items():
        collect(r, T, hooks[n])
    torch.cuda.synchronize()
    ms = {n: [] for n in runners}
    for _ in range(args.rounds):
        for n, r in runners.items():
            ms[n].append(timed(lambda: collect(r, T, hooks[n])))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"tool": "rough_bench", "envs": B, "steps": T, "rounds": args.rounds}
    for n in runners:
        out[f"collect_ms_{n}"], out[f"collect_ms_{n}_min_max"] = round(med(ms[n]), 3), [round(min(ms[n]), 3), round(max(ms[n]), 3)]
        runners[n].env.check_errno()
    if "rough_grid" in ms and "rough_grid_host_query" in ms:
        out["host_query_us_per_env_step"] = round((med(ms["rough_grid_host_query"]) - med(ms["rough_grid"])) * 1e3 / T, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
