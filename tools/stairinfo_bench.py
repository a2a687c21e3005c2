#!/usr/bin/env python
"""Times the four-value stair info (include/go2sim_stairinfo.h) on the GPU, at the stair task's training shape.

    python tools/stairinfo_bench.py [--envs 4096] [--steps 24] [--rounds 10] [--calls 2000]
    python tools/stairinfo_bench.py --count-ops            # no GPU needed: the aten operators one eager step dispatches

Two timings, both taken in one process with the variants alternating round by round, so that other work on the machine hits all alike:

  (a) the closed collection loop (act, env.step, process_env_step for --steps env steps of an OnPolicyRunner at --envs) on the stair env
      (`collect_ms_stairs`), on the LIDAR env (`collect_ms_lidar`), on the stair-info env (`collect_ms_stair_info`: one launch of k_stairinfo_step
      per env step) and on the stair-info env whose call is replaced by an eager-torch restatement of the reference's lines on the same device
      tensors (`collect_ms_stair_info_eager`);
  (b) the call alone on the stair-info env's buffers: `stairinfo_step_us` against `torch_eager_us` per env step.

The eager form reads the DR level as a device scalar and applies every degradation step unconditionally (at L = 0 they are neutral), so it has no
host read either; its random numbers are torch's.  Device events bracket each round; every shape is warmed up first.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidar_bench import swap_in  # noqa: E402


class EagerStairInfo:
    """go2_env_stair_lidar_2.py:836-975, the reset lines and the row assembly in eager torch; `step` has StairInfo.step's signature."""

    def __init__(self, layout, hf, h_scale, v_scale, origin, heights, depths, n_envs, pos, quat, rows, level, dr_schedule, device):
        t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=device)
        self.xs = t(layout["sample_x"])
        self.mid = (self.xs[:-1] + self.xs[1:]) / 2
        self.hf = torch.as_tensor(hf, device=device).to(torch.float32) * v_scale
        self.heights, self.depths = t(heights), t(depths)
        self.h_scale, self.ox, self.oy = h_scale, origin[0], origin[1]
        self.lay, self.pos, self.quat, self.rows, self.level, self.sched = layout, pos, quat, rows, level, dr_schedule   # pos [3][n], quat [4][n], rows int32 [n]
        self.stored = torch.zeros(n_envs, 4, device=device)
        self.n, self.device = n_envs, device
        self.batch = torch.arange(n_envs, device=device)

    def _level(self):
        t = self.level
        if self.sched is None:
            return t
        p1, gate = self.sched["phase1_level"], self.sched["terrain_gate"]
        return torch.where(t < gate, torch.full_like(t, p1), p1 + (1.0 - p1) * ((t - gate) / max(1e-6, 1.0 - gate)).clamp(0.0, 1.0))

    def _edge(self):
        lay = self.lay
        qw, qx, qy, qz = self.quat[0], self.quat[1], self.quat[2], self.quat[3]
        yaw = torch.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))
        c, s = torch.cos(yaw).unsqueeze(1), torch.sin(yaw).unsqueeze(1)
        lx = self.xs.unsqueeze(0)
        wx, wy = self.pos[0].unsqueeze(1) + c * lx, self.pos[1].unsqueeze(1) + s * lx
        col = ((wx - self.ox) / self.h_scale).long().clamp(0, self.hf.shape[0] - 1)
        row = ((wy - self.oy) / self.h_scale).long().clamp(0, self.hf.shape[1] - 1)
        h = self.hf[col, row]
        dh = h[:, 1:] - h[:, :-1]
        sig = torch.abs(dh) > lay["threshold"]
        has = sig.any(dim=1)
        first = sig.to(torch.int32).argmax(dim=1)
        edge = torch.where(has, self.mid[first], torch.full_like(self.mid[first], lay["max_range"]))
        e_dh = dh[self.batch, first]
        return edge, torch.where(has, torch.sign(e_dh), torch.zeros_like(e_dh))

    def step(self, pos, pos_strides, quat, quat_strides, rows, reset, level, obs, priv, n_in, obs_out, priv_out):
        lay, L = self.lay, self._level()
        Lf = L.float()
        edge, direction = self._edge()
        r = self.rows.long().clamp(0, self.heights.numel() - 1)
        height, depth = self.heights[r], self.depths[r]
        scales = (lay["edge_dist_scale"], lay["height_scale"], lay["depth_scale"], lay["direction_scale"])
        clean = torch.stack([edge * scales[0], height * scales[1], depth * scales[2], direction * scales[3]], dim=1)
        edge = (edge + torch.randn_like(edge) * lay["edge_noise_std"] * Lf).clamp(0.0, lay["max_range"])
        height = height + torch.randn_like(height) * lay["height_noise_std"] * Lf
        depth = depth + torch.randn_like(depth) * lay["depth_noise_std"] * Lf
        direction = torch.where(torch.rand(self.n, device=self.device) < (lay["direction_flip_prob"] * L).float(), -direction, direction)
        lat = torch.rand(self.n, device=self.device) < (lay["latency_prob"] * L).float()
        edge = torch.where(lat, self.stored[:, 0] / scales[0], edge)
        direction = torch.where(lat, self.stored[:, 3] / scales[3], direction)
        black = torch.rand(self.n, device=self.device) < (lay["full_blackout_prob"] * L).float()
        edge = torch.where(black, torch.full_like(edge, lay["max_range"]), edge)
        direction = torch.where(black, torch.zeros_like(direction), direction)
        actor = torch.stack([edge * scales[0], height * scales[1], depth * scales[2], direction * scales[3]], dim=1)
        if reset is not None:
            live = (reset == 0).unsqueeze(1)
            actor, clean = actor * live, clean * live
        self.stored = actor
        torch.cat([obs, actor], dim=1, out=obs_out)
        torch.cat([priv[:, :n_in], actor, priv[:, n_in:], clean], dim=1, out=priv_out)


def eager_for(env):
    """The eager form on a stair-info Go2Env's own buffers: the pose fields, the terrain rows, the level word, the heightfield the env was built with."""
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain
    from go2_sim2real_locomotion_rl_amd.capi import _as_device_tensor

    hf, info = build_stair_terrain(env.env_cfg["terrain"])
    pos_ptr, quat_ptr, cs = env._base_pose
    pos = _as_device_tensor(pos_ptr, (3, cs), torch.float32, env.device)
    quat = _as_device_tensor(quat_ptr, (4, cs), torch.float32, env.device)
    rows = _as_device_tensor(env._terrain_rows_ptr, (cs,), torch.int32, env.device)
    return EagerStairInfo(env._stairinfo.layout, hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"], info["step_heights_m"],
                          info["step_depths_m"], env.num_envs, pos, quat, rows, env._glob_f64[env._level_off], env.env_cfg.get("dr_schedule"), env.device)


def count_ops():
    """aten operators of one eager step on CPU tensors (each is at least one kernel launch on the device)"""
    from torch.utils._python_dispatch import TorchDispatchMode

    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain, get_stair_info_cfgs
    from go2_sim2real_locomotion_rl_amd.stairinfo import stair_info_layout

    env_cfg = get_stair_info_cfgs()[0]
    hf, info = build_stair_terrain(env_cfg["terrain"])
    n = 64
    quat = torch.zeros(4, n); quat[0] = 1.0
    e = EagerStairInfo(stair_info_layout(env_cfg["stair_info"]), hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"],
                       info["step_heights_m"], info["step_depths_m"], n, torch.rand(3, n), quat, torch.zeros(n, dtype=torch.int32),
                       torch.tensor(0.65, dtype=torch.float64), env_cfg["dr_schedule"], "cpu")
    ops = []

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            ops.append(str(func))
            return func(*args, **(kwargs or {}))

    with Count():
        e.step(None, None, None, None, None, torch.zeros(n, dtype=torch.uint8), None, torch.zeros(n, 49), torch.zeros(n, 105), 49, torch.empty(n, 53),
               torch.empty(n, 113))
    views = ("unsqueeze", "select", "slice", "expand", "view", "alias", "detach")
    launches = [o for o in ops if not any(v in o for v in views)]
    print(json.dumps({"tool": "stairinfo_bench", "eager_aten_ops_per_step": len(ops), "of_which_not_views": len(launches)}))


def make_runner(task, envs, steps, seed=3):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_stair_cfgs, get_stair_info_cfgs, get_stair_lidar_cfgs, init

    init(seed=seed)
    cfgs = {"stairs": get_stair_cfgs, "lidar": get_stair_lidar_cfgs, "stair_info": get_stair_info_cfgs}[task]()
    env = Go2Env(envs, *cfgs, seed=seed)
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
    ap.add_argument("--calls", type=int, default=2000, help="calls per round of (b)")
    ap.add_argument("--count-ops", action="store_true")
    args = ap.parse_args()
    if args.count_ops:
        return count_ops()
    if not torch.cuda.is_available():
        raise SystemExit("tools/stairinfo_bench.py needs a ROCm GPU (nothing is measured without one)")
    B, T = args.envs, args.steps

    # (a) the closed collection loop
    runners = {"stairs": make_runner("stairs", B, T), "lidar": make_runner("lidar", B, T), "stair_info": make_runner("stair_info", B, T),
               "stair_info_eager": make_runner("stair_info", B, T)}
    eenv = runners["stair_info_eager"].env
    swap_in(eenv, eenv._stairinfo, eager_for(eenv))
    ms = {k: [] for k in runners}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, r in runners.items():
            ms[k].append(timed(lambda: collect(r, T)))
    med = lambda v: sorted(v)[len(v) // 2]

    # (b) the call of one env step, on the stair-info env's own buffers
    env = runners["stair_info"].env
    hip, eager = env._stairinfo, eager_for(env)
    pos, quat, cs = env._base_pose
    obs_out, priv_out = torch.empty_like(env.obs_buf), torch.empty_like(env.privileged_obs_buf)
    a = (pos, (cs, 1), quat, (cs, 1), env._terrain_rows_ptr, env.reset_buf, env._level_ptr, env._inner_obs, env._inner_priv, env._inner_obs.shape[1], obs_out, priv_out)
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
    out = {"tool": "stairinfo_bench", "envs": B, "steps": T, "rounds": args.rounds, "calls_per_round": args.calls}
    for k in runners:
        out[f"collect_ms_{k}"], out[f"collect_ms_{k}_min_max"] = round(med(ms[k]), 3), mm(ms[k], 3)
    out.update({"stair_info_minus_stairs_us_per_env_step": round((med(ms["stair_info"]) - med(ms["stairs"])) * 1e3 / T, 2),
                "stair_info_minus_lidar_us_per_env_step": round((med(ms["stair_info"]) - med(ms["lidar"])) * 1e3 / T, 2),
                "eager_minus_stair_info_us_per_env_step": round((med(ms["stair_info_eager"]) - med(ms["stair_info"])) * 1e3 / T, 2),
                "stairinfo_step_us": round(med(us["hip"]), 2), "torch_eager_us": round(med(us["torch"]), 2),
                "stairinfo_step_us_min_max": mm(us["hip"], 2), "torch_eager_us_min_max": mm(us["torch"], 2),
                "torch_over_hip": round(med(us["torch"]) / med(us["hip"]), 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
