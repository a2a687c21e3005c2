#!/usr/bin/env python
"""Times the LIDAR terrain scan (include/go2sim_lidar.h) on the GPU, at the stair task's training shape.

    python tools/lidar_bench.py [--envs 4096] [--steps 24] [--rounds 10] [--calls 2000]
    python tools/lidar_bench.py --count-ops            # no GPU needed: the aten operators one eager scan step dispatches

Two timings, both taken in one process with the variants alternating round by round, so that other work on the machine hits all alike:

  (a) the closed collection loop (act, env.step, process_env_step for --steps env steps of an OnPolicyRunner at --envs) on the stair env
      (`collect_ms_stairs`), on the LIDAR env (`collect_ms_lidar`: the scan is one launch of k_lidar_step per env step) and on the LIDAR env whose
      scan call is replaced by an eager-torch restatement of the reference's lines on the same device tensors (`collect_ms_lidar_eager`);
  (b) the scan call alone on the LIDAR env's buffers: `lidar_step_us` against `torch_eager_us` per env step.

The eager form reads the DR level as a device scalar and applies every randomisation step unconditionally (at L = 0 they are neutral), so it has no
host read either; its random numbers are torch's.  Device events bracket each round; every shape is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import sys

import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class EagerScan:
    """go2_env_stair_lidar.py:883-1015 and the row assembly :1615-1692 in eager torch; `step` has LidarScan.step's signature."""

    def __init__(self, layout, hf, h_scale, v_scale, origin, n_envs, pos, quat, level, dr_schedule, device):
        t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=device)
        self.ax, self.ay, self.cx, self.cy = t(layout["actor_xy"][0]), t(layout["actor_xy"][1]), t(layout["critic_xy"][0]), t(layout["critic_xy"][1])
        self.hf = torch.as_tensor(hf, device=device).to(torch.float32) * v_scale
        self.h_scale, self.ox, self.oy = h_scale, origin[0], origin[1]
        self.lay, self.pos, self.quat, self.level, self.sched = layout, pos, quat, level, dr_schedule      # pos [3][n], quat [4][n], level: 0-dim float64
        self.stored = torch.zeros(n_envs, self.ax.numel(), device=device)
        self.n, self.device = n_envs, device

    def _scan(self, lx, ly):
        qw, qx, qy, qz = self.quat[0], self.quat[1], self.quat[2], self.quat[3]
        yaw = torch.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))
        c, s = torch.cos(yaw).unsqueeze(1), torch.sin(yaw).unsqueeze(1)
        wx = self.pos[0].unsqueeze(1) + c * lx.unsqueeze(0) - s * ly.unsqueeze(0)
        wy = self.pos[1].unsqueeze(1) + s * lx.unsqueeze(0) + c * ly.unsqueeze(0)
        col = ((wx - self.ox) / self.h_scale).long().clamp(0, self.hf.shape[0] - 1)
        row = ((wy - self.oy) / self.h_scale).long().clamp(0, self.hf.shape[1] - 1)
        return self.hf[col, row] - self.pos[2].unsqueeze(1)

    def _level(self):
        t = self.level
        if self.sched is None:
            return t
        p1, gate = self.sched["phase1_level"], self.sched["terrain_gate"]
        return torch.where(t < gate, torch.full_like(t, p1), p1 + (1.0 - p1) * ((t - gate) / max(1e-6, 1.0 - gate)).clamp(0.0, 1.0))

    def step(self, pos, pos_strides, quat, quat_strides, reset, level, obs, priv, n_in, obs_out, priv_out):
        lay, L = self.lay, self._level()
        Lf = L.float()
        raw = self._scan(self.ax, self.ay)
        raw = raw + torch.randn_like(raw) * lay["height_noise_std"] * Lf
        raw = torch.where(torch.rand_like(raw) < (lay["dropout_prob"] * L).float(), torch.zeros_like(raw), raw)
        raw = raw + torch.randn(self.n, 1, device=self.device) * lay["vertical_offset_std"] * Lf
        raw = torch.where((torch.rand(self.n, device=self.device) < (lay["latency_prob"] * L).float()).unsqueeze(1), self.stored, raw)
        raw = torch.where((torch.rand(self.n, device=self.device) < (lay["full_blackout_prob"] * L).float()).unsqueeze(1), torch.zeros_like(raw), raw)
        actor = torch.clamp(raw, -lay["height_clip"], lay["height_clip"]) * lay["height_scale"]
        critic = torch.clamp(self._scan(self.cx, self.cy), -lay["height_clip"], lay["height_clip"]) * lay["height_scale"]
        if reset is not None:
            live = (reset == 0).unsqueeze(1)
            actor, critic = actor * live, critic * live
        self.stored = actor
        torch.cat([obs, actor], dim=1, out=obs_out)
        torch.cat([priv[:, :n_in], actor, priv[:, n_in:], critic], dim=1, out=priv_out)


def swap_in(env, hip, eager):
    """Run `eager` (a `step` with the handle's signature) in the env's launch list in the place of the handle `hip`; nothing is cleared or logged."""
    eager.launch = types.MethodType(type(hip).launch, eager)
    eager.clear = eager.log = lambda *a: None
    eager.episode_entries, eager.curriculum_entries = hip.episode_entries, hip.curriculum_entries
    env._launches[env._launches.index(hip)] = eager


def eager_for(env):
    """The eager scan on an LIDAR Go2Env's own buffers: the pose fields, the level word of the globals, the heightfield the env was built with."""
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain
    from go2_sim2real_locomotion_rl_amd.capi import _as_device_tensor

    hf, info = build_stair_terrain(env.env_cfg["terrain"])
    pos_ptr, quat_ptr, cs = env._base_pose
    pos = _as_device_tensor(pos_ptr, (3, cs), torch.float32, env.device)
    quat = _as_device_tensor(quat_ptr, (4, cs), torch.float32, env.device)
    return EagerScan(env._lidar.layout, hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"], env.num_envs, pos, quat,
                     env._glob_f64[env._level_off], env.env_cfg.get("dr_schedule"), env.device)


def count_ops():
    """aten operators of one eager step on CPU tensors (each is at least one kernel launch on the device)"""
    from torch.utils._python_dispatch import TorchDispatchMode

    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain, get_stair_lidar_cfgs
    from go2_sim2real_locomotion_rl_amd.lidar import lidar_layout

    env_cfg = get_stair_lidar_cfgs()[0]
    hf, info = build_stair_terrain(env_cfg["terrain"])
    n = 64
    quat = torch.zeros(4, n); quat[0] = 1.0
    e = EagerScan(lidar_layout(env_cfg["lidar"]), hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"], n, torch.rand(3, n), quat,
                  torch.tensor(0.65, dtype=torch.float64), env_cfg["dr_schedule"], "cpu")
    ops = []

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            ops.append(str(func))
            return func(*args, **(kwargs or {}))

    with Count():
        e.step(None, None, None, None, torch.zeros(n, dtype=torch.uint8), None, torch.zeros(n, 49), torch.zeros(n, 105), 49, torch.empty(n, 64), torch.empty(n, 165))
    views = ("unsqueeze", "select", "slice", "expand", "view", "alias", "detach")
    launches = [o for o in ops if not any(v in o for v in views)]
    print(json.dumps({"tool": "lidar_bench", "eager_aten_ops_per_step": len(ops), "of_which_not_views": len(launches)}))


def make_runner(task, envs, steps, seed=3):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_stair_cfgs, get_stair_lidar_cfgs, init

    init(seed=seed)
    env = Go2Env(envs, *(get_stair_lidar_cfgs() if task == "lidar" else get_stair_cfgs()), seed=seed)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_cfgs_stairs.json")))["train_cfg"]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=10, help="timed rollouts per variant of (a) and timed rounds of (b)")
    ap.add_argument("--calls", type=int, default=2000, help="scan calls per round of (b)")
    ap.add_argument("--count-ops", action="store_true")
    args = ap.parse_args()
    if args.count_ops:
        return count_ops()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lidar_bench.py needs a ROCm GPU (nothing is measured without one)")
    B, T = args.envs, args.steps

    # (a) the closed collection loop
    runners = {"stairs": make_runner("stairs", B, T), "lidar": make_runner("lidar", B, T), "lidar_eager": make_runner("lidar", B, T)}
    swap_in(runners["lidar_eager"].env, runners["lidar_eager"].env._lidar, eager_for(runners["lidar_eager"].env))
    ms = {k: [] for k in runners}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, r in runners.items():
            ms[k].append(timed(lambda: collect(r, T)))
    med = lambda v: sorted(v)[len(v) // 2]

    # (b) the scan call of one env step, on the LIDAR env's own buffers
    env = runners["lidar"].env
    hip, eager = env._lidar, eager_for(env)
    pos, quat, cs = env._base_pose
    obs_out, priv_out = torch.empty_like(env.obs_buf), torch.empty_like(env.privileged_obs_buf)
    a = (pos, (cs, 1), quat, (cs, 1), env.reset_buf, env._level_ptr, env._inner_obs, env._inner_priv, env._inner_obs.shape[1], obs_out, priv_out)
    sides = {"hip": lambda: hip.step(*a), "torch": lambda: eager.step(*a)}
    us = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in sides.items():
            us[k].append(timed(lambda: [fn() for _ in range(args.calls)]) * 1e3 / args.calls)
    mm = lambda v, nd: [round(min(v), nd), round(max(v), nd)]
    print(json.dumps({"tool": "lidar_bench", "envs": B, "steps": T, "rounds": args.rounds, "calls_per_round": args.calls,
                      "collect_ms_stairs": round(med(ms["stairs"]), 3), "collect_ms_lidar": round(med(ms["lidar"]), 3),
                      "collect_ms_lidar_eager": round(med(ms["lidar_eager"]), 3),
                      "collect_ms_stairs_min_max": mm(ms["stairs"], 3), "collect_ms_lidar_min_max": mm(ms["lidar"], 3),
                      "collect_ms_lidar_eager_min_max": mm(ms["lidar_eager"], 3),
                      "lidar_minus_stairs_us_per_env_step": round((med(ms["lidar"]) - med(ms["stairs"])) * 1e3 / T, 2),
                      "eager_minus_lidar_us_per_env_step": round((med(ms["lidar_eager"]) - med(ms["lidar"])) * 1e3 / T, 2),
                      "lidar_step_us": round(med(us["hip"]), 2), "torch_eager_us": round(med(us["torch"]), 2),
                      "lidar_step_us_min_max": mm(us["hip"], 2), "torch_eager_us_min_max": mm(us["torch"], 2),
                      "torch_over_hip": round(med(us["torch"]) / med(us["hip"]), 2)}))


if __name__ == "__main__":
    main()
