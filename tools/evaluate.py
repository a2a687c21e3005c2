#!/usr/bin/env python
"""Evaluates a trained policy over a grid of commands (and terrain rows) on the GPU and prints one JSON document.

    python tools/evaluate.py --log-dir logs/go2-walk --ckpt 3000 --envs 4096 --vx 0 0.5 1.0 --vy 0 --yaw -0.5 0 0.5 [--rows 0 4 8 12] [--level 1.0]
                             [--episodes 4] [--settle-steps 25] [--max-steps 6000] [--json out.json]

Reads <log-dir>/cfgs.pkl and <log-dir>/model_<ckpt>.pt through eval_io (plain containers and tensors only: nothing from the files is imported or
executed), builds the env with the curriculum frozen (at --level if given) and the command resampling pushed past the episode, and the runner of the
run's train_cfg, so that the checkpoint's normaliser is applied when it has one and a recurrent policy keeps its memory, reset with the env's dones.
Every env evaluates one cell of the grid; the per-step bookkeeping is one launch behind the env step (include/go2sim_evalstats.h), the derived values
are float64 on the host (evaluation.bin_metrics)."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--log-dir", required=True)
    ap.add_argument("--ckpt", type=int, required=True, help="the iteration N of model_N.pt")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--vx", type=float, nargs="+", default=[0.0, 0.5, 1.0])
    ap.add_argument("--vy", type=float, nargs="+", default=[0.0])
    ap.add_argument("--yaw", type=float, nargs="+", default=[0.0])
    ap.add_argument("--rows", type=int, nargs="+", default=None, help="difficulty rows of a stair terrain to evaluate on")
    ap.add_argument("--level", type=float, default=None, help="the curriculum level to evaluate at (default: the cfg's level_init)")
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--settle-steps", type=int, default=25)
    ap.add_argument("--max-steps", type=int, default=None, help="default: episodes + 1 whole episodes")
    ap.add_argument("--torque-limit", type=float, default=23.7)
    ap.add_argument("--dof-vel-limit", type=float, default=30.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None, help="also write the document to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/evaluate.py needs a ROCm GPU (the product path has no CPU fallback)")
    from go2_sim2real_locomotion_rl_amd import Evaluator, Go2Env, OnPolicyRunner, command_grid, init, load_cfgs

    env_cfg, obs_cfg, reward_cfg, command_cfg, train_cfg = (copy.deepcopy(c) for c in load_cfgs(os.path.join(args.log_dir, "cfgs.pkl")))
    env_cfg["resampling_time_s"] = 2.0 * float(env_cfg["episode_length_s"])          # the scripted command holds for the whole episode
    init(seed=args.seed)
    env = Go2Env(args.envs, env_cfg, obs_cfg, reward_cfg, command_cfg, seed=args.seed, freeze_curriculum=True)
    if args.level is not None:
        env._sim.env_set_level(float(args.level), torch.cuda.current_stream(env.device).cuda_stream)
    runner = OnPolicyRunner(env, train_cfg)
    path = os.path.join(args.log_dir, f"model_{args.ckpt}.pt")
    runner.load(path, load_optimizer=False)
    grid = command_grid(args.envs, vx=args.vx, vy=args.vy, yaw=args.yaw)
    ev = Evaluator(env, runner.get_inference_policy(), commands=grid, terrain_rows=args.rows, settle_steps=args.settle_steps, max_episodes=args.episodes,
                   torque_limit=args.torque_limit, dof_vel_limit=args.dof_vel_limit, memory=runner.policy)
    max_steps = args.max_steps if args.max_steps is not None else (args.episodes + 1) * (env.max_episode_length + 1)
    report = ev.run(max_steps)
    report.update({"tool": "evaluate", "checkpoint": path, "level": float(env.curriculum_level), "torque_limit": args.torque_limit,
                   "dof_vel_limit": args.dof_vel_limit, "errno": int(env.check_errno())})
    text = json.dumps(report, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
