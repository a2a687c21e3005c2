#!/usr/bin/env python3
"""Env-steps/s of the walk env with per-leg stiffness off (pls_enable=False), next to the PLS-on walk env measured the same way.

    python tools/pls_off_bench.py [--envs 4096] [--steps 300] [--warmup 100] [--modes on,A,B,C]

Modes ("Per-leg stiffness off"): on = the shipped PLS walk cfg; A = PLS off, manual PD on per-env base x factor gains; B = PLS off, engine PD
with the batch-mean gain of each reset call; C = PLS off, engine PD on env_cfg kp / kd.  Go2Env through the step graph, a ring of eight fixed random
action batches (scale 0.6, so that envs fall and reset throughout), hipEvent timing of the timed steps.  Prints one JSON line per mode.  Not bench.py:
the driver's workload stays the PLS-on walk env."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cfgs_for(mode):
    from go2_sim2real_locomotion_rl_amd.configs import get_walk_cfgs

    cfgs = copy.deepcopy(get_walk_cfgs(pls_enable=(mode == "on")))
    if mode in ("B", "C"):
        cfgs[0].pop("kp_factor_range"); cfgs[0].pop("kd_factor_range")
    if mode == "C":
        cfgs[0].pop("kp_range"); cfgs[0].pop("kd_range")
    return cfgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--modes", default="on,A,B,C")
    args = ap.parse_args()
    from go2_sim2real_locomotion_rl_amd import Go2Env, init

    init(precision="32", seed=1)
    modes = args.modes.split(",")
    for k, mode in enumerate([modes[0]] + modes):                          # pass 0 warms the device up (the first env of a process runs slower); not reported
        env = Go2Env(args.envs, *cfgs_for(mode), seed=1, log_extras=False)
        gen = torch.Generator(device="cuda").manual_seed(0)
        ring = [0.6 * torch.randn(args.envs, env.num_actions, device="cuda", generator=gen) for _ in range(8)]
        for s in range(args.warmup):
            env.step(ring[s % 8])
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        resets = torch.zeros((), device="cuda")
        torch.cuda.synchronize()
        t0.record()
        for s in range(args.steps):
            _, _, rst, _ = env.step(ring[s % 8])
            resets += rst.sum()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        assert env.check_errno() == 0
        if k == 0:
            del env
            continue
        print(json.dumps({"mode": mode, "pls_enable": mode == "on", "num_actions": env.num_actions, "envs": args.envs, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": ms / args.steps, "env_steps_per_s": args.envs * args.steps / (ms / 1e3),
                          "resets_per_step": float(resets) / args.steps}), flush=True)
        del env


if __name__ == "__main__":
    main()
