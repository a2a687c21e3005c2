#!/usr/bin/env python
"""Times the empirical observation normaliser (include/go2sim_norm.h) on the GPU, at the walk task's training shape.

    python tools/norm_bench.py [--envs 4096] [--steps 24] [--rounds 10] [--calls 2000] [--trace-steps N]

Two timings, both taken in one process with the two variants alternating round by round, so that other work on the machine hits both alike:

  (a) the closed collection loop (Go2Env walk task at --envs: act, env.step, normalise, process_env_step for --steps env steps) of an OnPolicyRunner with
      ``empirical_normalization`` on against one with it off: `collect_ms_norm_on`, `collect_ms_norm_off` per rollout and their difference per env step;
  (b) `norm_step` on [envs x 49] + [envs x 104] (both normalisers in one call, update on) against a literal eager-torch restatement of rsl_rl 2.2.4's module
      called on the two tensors: `norm_step_us`, `torch_eager_us` per env step's normalisation.

Device events bracket each round; every shape is warmed up first.  Prints one JSON line.  --trace-steps N instead runs N normalised env steps after a warm-up
and exits: the body of a `rocprofv3 --kernel-trace` run of its own, which counts the launches per env step (the k_norm_* rows of the trace)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class TorchNorm:
    """rsl_rl 2.2.4 EmpiricalNormalization in eager torch on the device"""

    def __init__(self, d, device, eps=1e-2, until=1e8):
        self.eps, self.until = eps, until
        self._mean, self._var, self._std = torch.zeros(1, d, device=device), torch.ones(1, d, device=device), torch.ones(1, d, device=device)
        self.count = torch.tensor(0, dtype=torch.long, device=device)

    def __call__(self, x):
        self.update(x)
        return (x - self._mean) / (self._std + self.eps)

    def update(self, x):
        if self.until is not None and self.count >= self.until:          # the module's host read of its count
            return
        count_x = x.shape[0]
        self.count += count_x
        rate = count_x / self.count
        var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(x, dim=0, keepdim=True)
        delta_mean = mean_x - self._mean
        self._mean += rate * delta_mean
        self._var += rate * (var_x - self._var + delta_mean * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)


def make_runner(envs, steps, normalise, seed=3):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_walk_cfgs, init

    init(seed=seed)
    env = Go2Env(envs, *get_walk_cfgs(), seed=seed)
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref_cfgs_walk.json")))["train_cfg"]
    cfg["num_steps_per_env"], cfg["empirical_normalization"] = steps, bool(normalise)
    return OnPolicyRunner(env, cfg)


def collect(runner, steps):
    """the collection part of OnPolicyRunner.learn: no returns, no update"""
    env, alg = runner.env, runner.alg
    obs, extras = env.get_observations()
    critic_obs = extras["observations"].get("critic", obs)
    if runner.empirical_normalization:
        obs, critic_obs = runner._normalize(obs, extras["observations"].get("critic"), update=False)
    for _ in range(steps):
        actions = alg.act(obs, critic_obs)
        obs, rewards, dones, infos = env.step(actions)
        critic_obs = infos["observations"].get("critic", obs)
        if runner.empirical_normalization:
            obs, critic_obs = runner._normalize(obs, infos["observations"].get("critic"), update=True)
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
    ap.add_argument("--rounds", type=int, default=10, help="timed rollouts per variant of (a) and timed rounds of (b)")
    ap.add_argument("--calls", type=int, default=2000, help="normalisation calls per round of (b)")
    ap.add_argument("--trace-steps", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/norm_bench.py needs a ROCm GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    B, T = args.envs, args.steps

    if args.trace_steps:
        runner = make_runner(B, args.trace_steps, True)
        collect(runner, args.trace_steps)                                  # warm-up: code objects, buffers
        torch.cuda.synchronize()
        print(json.dumps({"tool": "norm_bench", "trace_steps": args.trace_steps, "note": "the second block of env steps is the one to count"}), flush=True)
        collect(runner, args.trace_steps)
        torch.cuda.synchronize()
        return

    from go2_sim2real_locomotion_rl_amd import EmpiricalNormalization
    from go2_sim2real_locomotion_rl_amd.normalization import norm_step

    # (a) the closed collection loop
    runners = {"on": make_runner(B, T, True), "off": make_runner(B, T, False)}
    ms = {k: [] for k in runners}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, r in runners.items():
            ms[k].append(timed(lambda: collect(r, T)))
    med = lambda v: sorted(v)[len(v) // 2]

    # (b) the normalisation of one env step: both observation sets
    g = torch.Generator(device=dev).manual_seed(5)
    xa, xb = torch.randn(B, 49, device=dev, generator=g) * 2 + 1, torch.randn(B, 104, device=dev, generator=g) * 3 - 1
    na, nb = EmpiricalNormalization(49, until=1e8), EmpiricalNormalization(104, until=1e8)
    ta, tb = TorchNorm(49, dev), TorchNorm(104, dev)
    sides = {"hip": lambda: norm_step(na, xa, nb, xb, update=True), "torch": lambda: (ta(xa), tb(xb))}
    us = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in sides.items():
            us[k].append(timed(lambda: [fn() for _ in range(args.calls)]) * 1e3 / args.calls)
    print(json.dumps({"tool": "norm_bench", "envs": B, "steps": T, "rounds": args.rounds, "calls_per_round": args.calls,
                      "collect_ms_norm_on": round(med(ms["on"]), 3), "collect_ms_norm_off": round(med(ms["off"]), 3),
                      "collect_ms_norm_on_min_max": [round(min(ms["on"]), 3), round(max(ms["on"]), 3)],
                      "collect_ms_norm_off_min_max": [round(min(ms["off"]), 3), round(max(ms["off"]), 3)],
                      "norm_us_per_env_step_in_loop": round((med(ms["on"]) - med(ms["off"])) * 1e3 / T, 2),
                      "norm_step_us": round(med(us["hip"]), 2), "torch_eager_us": round(med(us["torch"]), 2),
                      "norm_step_us_min_max": [round(min(us["hip"]), 2), round(max(us["hip"]), 2)],
                      "torch_eager_us_min_max": [round(min(us["torch"]), 2), round(max(us["torch"]), 2)],
                      "torch_over_hip": round(med(us["torch"]) / med(us["hip"]), 2), "bytes_read_per_call": B * (49 + 104) * 4}))


if __name__ == "__main__":
    main()
