#!/usr/bin/env python
"""Times the stairwell env (include/go2sim_wells.h) on the GPU, at the training shape and on the training terrain.

    python tools/stairwell_bench.py [--envs 4096] [--steps 24] [--rounds 10]

The closed collection loop (act, env.step, process_env_step for --steps env steps of an OnPolicyRunner at --envs), taken in one process with the
variants alternating round by round, so that other work on the machine hits all alike:

  collect_ms_stairs              the corridor stair env (13 rows, 77-point scan inside the step kernels)
  collect_ms_stairs_lidar        the LIDAR stair env: the corridor env plus its scan launch, the yardstick for one more launch of this kind
  collect_ms_stairwell           the stairwell env on its 1583 x 1583 field: well spawn in the chain, the wells launch after the step
  collect_ms_stairwell_no_spawn  the same handle reconfigured with GO2SIM_IC_WELL_SPAWN off (envs spawn on the well centres, yaw 0): the difference
                                 is the spawn launch's share

and, launched back to back on the envs' own pose buffers, the scan launches alone: wells_step_us (226-wide rows, 121 points, alive term) and
lidar_step_us (165-wide rows, 15 + 45 points, noise) per launch.

Then the terrain itself: the time of go2sim_set_terrain for the training field on a fresh handle, and the contact counts of robots standing, after
--settle zero-action steps, on the bottom of their wells and on the landings between the two flights.

Device events bracket each round; every variant is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_runner(task, envs, steps, seed=3):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_stair_cfgs, get_stair_lidar_cfgs, get_stairwell_cfgs, init

    init(seed=seed)
    cfgs = {"stairs": get_stair_cfgs, "stairs_lidar": get_stair_lidar_cfgs, "stairwell": get_stairwell_cfgs, "stairwell_no_spawn": get_stairwell_cfgs}[task]()
    env = Go2Env(envs, *cfgs, seed=seed)
    if task == "stairwell_no_spawn":
        from go2_sim2real_locomotion_rl_amd.capi import C
        from go2_sim2real_locomotion_rl_amd.configs import flatten_walk_cfg

        inner = dict(cfgs[1], num_privileged_obs=cfgs[1]["num_obs"] + C["GO2SIM_WELLS_PRIV_EXTRA"])
        f, i, _ = flatten_walk_cfg(envs, cfgs[0], inner, cfgs[2], cfgs[3])
        i[C["GO2SIM_IC_WELL_SPAWN"]] = 0
        env._sim.env_configure(f, i)
        env.reset()
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_cfgs_stairwell.json" if task.startswith("stairwell") else "ref_cfgs_stairs.json")))["train_cfg"]
    cfg["num_steps_per_env"] = steps
    return OnPolicyRunner(env, cfg)


def collect(runner, steps):
    """the collection part of OnPolicyRunner.learn: no returns, no update"""
    env, alg = runner.env, runner.alg
    obs, extras = env.get_observations()
    critic_obs = extras["observations"].get("critic", obs)
    for _ in range(steps):
        actions = alg.act(obs, critic_obs)
        obs, rewards, dones, infos = env.step(actions)
        critic_obs = infos["observations"].get("critic", obs)
        alg.process_env_step(rewards, dones, infos)
    alg.t = 0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def scan_launch_us(env, reps=200):
    """one scan launch of `env` on its own pose buffers, back to back: microseconds per launch"""
    pos, quat, cs = env._base_pose
    if env._wells is not None:
        rew = torch.zeros(env.num_envs, device=env.device)
        one = lambda: env._wells.step(pos, (cs, 1), quat, (cs, 1), env.reset_buf, env._inner_priv, env.num_obs, env.privileged_obs_buf, rew)
    else:
        n_in = env._inner_obs.shape[1]
        one = lambda: env._lidar.step(pos, (cs, 1), quat, (cs, 1), env.reset_buf, env._level_ptr, env._inner_obs, env._inner_priv, n_in,
                                      env.obs_buf, env.privileged_obs_buf)
    many = lambda: [one() for _ in range(reps)]
    many()
    torch.cuda.synchronize()
    return sorted(timed(many) for _ in range(5))[2] * 1e3 / reps


def terrain_report(envs, settle):
    """set_terrain time of the training field, and contact counts at the bottoms and on the landings"""
    from go2_sim2real_locomotion_rl_amd import Go2Env, get_stairwell_cfgs, init
    from go2_sim2real_locomotion_rl_amd.capi import C, Go2Sim, load_hip_lib
    from go2_sim2real_locomotion_rl_amd.model_blob import pack_model
    from go2_sim2real_locomotion_rl_amd.terrain_wells import build_stairwell_terrain, well_centers

    cfgs = get_stairwell_cfgs()
    t0 = time.perf_counter()
    hf, info = build_stairwell_terrain(cfgs[0]["terrain"])
    t_build = time.perf_counter() - t0
    sim = Go2Sim(load_hip_lib(), pack_model(), 8, 0, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.set_terrain(hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"])
    torch.cuda.synchronize()
    t_set = time.perf_counter() - t0
    del sim
    init(seed=5)
    cfgs[0]["curriculum"]["level_init"] = 1.0
    cfgs[0].pop("push_force_range", None)
    env = Go2Env(envs, *cfgs, seed=5)
    zero = torch.zeros(envs, env.num_actions, device=env.device)

    def contacts():
        n_reset = 0
        for _ in range(settle):
            n_reset += int(env.step(zero)[2].sum())
        n = torch.zeros(1, envs, dtype=torch.int32, device=env.device)
        env._sim.get_field(C["GO2SIM_I_N_CONTACTS"], n, torch.cuda.current_stream(env.device).cuda_stream)
        torch.cuda.synchronize()
        n = n.cpu().numpy()[0]
        return {"mean": round(float(n.mean()), 3), "min": int(n.min()), "max": int(n.max()), "resets_while_settling": n_reset}

    out = {"field_cells": list(hf.shape), "build_terrain_s": round(t_build, 3), "set_terrain_s": round(t_set, 3), "contacts_bottom": contacts()}
    # the landing between the two flights, along +x of every env's well: half the bottom, one flight, half the landing
    t = cfgs[0]["terrain"]
    hs = info["horizontal_scale"]
    cells = lambda m: max(1, int(round(m / hs)))
    dist = (cells(t["flat_bottom_m"]) // 2 + t["steps_per_flight"] * cells(t["step_depth_m"]) + cells(t["flat_landing_m"]) // 2) * hs
    levels = env._env_view("TERRAIN_ROW", 1, torch.int32).long()
    centres = torch.tensor(well_centers(info), device=env.device, dtype=torch.float32)[levels]
    rise = torch.tensor(info["step_heights_m"], device=env.device, dtype=torch.float32)[levels]
    rise = torch.round(rise / info["vertical_scale"]) * info["vertical_scale"] * t["steps_per_flight"]
    pos = torch.stack([centres[:, 0] + dist, centres[:, 1], centres[:, 2] + rise + 0.36], 1)
    env.respawn(torch.arange(envs), pos, None, True)
    out["contacts_landing"] = contacts()
    out["errno"] = int(env.check_errno())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=10, help="timed rollouts per variant")
    ap.add_argument("--settle", type=int, default=40, help="zero-action steps before the contacts are counted")
    ap.add_argument("--only", default=None, help="comma-separated variants (e.g. stairwell for a profiler run)")
    ap.add_argument("--no-terrain-report", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/stairwell_bench.py needs a ROCm GPU (nothing is measured without one)")
    B, T = args.envs, args.steps
    names = ["stairs", "stairs_lidar", "stairwell", "stairwell_no_spawn"]
    if args.only:
        names = [n for n in names if n in args.only.split(",")]
    runners = {n: make_runner(n, B, T) for n in names}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    ms = {n: [] for n in runners}
    for _ in range(args.rounds):
        for n, r in runners.items():
            ms[n].append(timed(lambda: collect(r, T)))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"tool": "stairwell_bench", "envs": B, "steps": T, "rounds": args.rounds}
    for n in runners:
        out[f"collect_ms_{n}"], out[f"collect_ms_{n}_min_max"] = round(med(ms[n]), 3), [round(min(ms[n]), 3), round(max(ms[n]), 3)]
        runners[n].env.check_errno()
    if "stairwell" in ms and "stairwell_no_spawn" in ms:
        out["spawn_us_per_env_step"] = round((med(ms["stairwell"]) - med(ms["stairwell_no_spawn"])) * 1e3 / T, 2)
    if "stairwell" in runners:
        out["wells_step_us"] = round(scan_launch_us(runners["stairwell"].env), 2)
    if "stairs_lidar" in runners:
        out["lidar_step_us"] = round(scan_launch_us(runners["stairs_lidar"].env), 2)
    runners.clear()
    if not args.no_terrain_report:
        out["terrain"] = terrain_report(min(B, 256), args.settle)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
