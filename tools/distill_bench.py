#!/usr/bin/env python
"""Times teacher-student distillation (include/go2sim_distill.h) on the GPU, at the walk task's training shape.

    python tools/distill_bench.py [--envs 4096] [--steps 24] [--gradient-length 15] [--rounds 10]
    python tools/distill_bench.py --recurrent [--rnn-hidden 256] [--sub-envs 1024] ...      # the recurrent student (include/go2sim_rdistill.h), see below

Two timings, both taken in one process with the two variants alternating round by round, so that other work on the machine hits both alike:

  (a) ``Distillation.update()`` (one epoch, the windows of --gradient-length steps, the loss-only tail, the read of the statistics) against an eager-torch
      float32 restatement on the same tensors (nn.Sequential on the device, autograd, torch.optim.Adam, one ``.item()`` at the end): `update_ms_hip`,
      `update_ms_torch`;
  (b) the closed collection loop (Go2Env walk task at --envs: act, env.step, process_env_step for --steps env steps) of a distillation runner (student and
      teacher in one launch per step) against the PPO runner's (actor and critic in one launch): `collect_ms_distill`, `collect_ms_ppo` per rollout.

Device events bracket each round; every shape is warmed up first.  Prints one JSON line.  Launches, counted from the code (csrc/go2sim_distill.hip): 2 per env
step for act (forward of both networks, sampling); per sub-batch of 8192 rows 3 L + 2 (forward, head, dW and db per layer, dA per hidden layer, the chunk
reduction: 14 for a student of L = 4 layers), per window one finalize and 2 for the optimizer.

--recurrent times Distillation + StudentTeacherRecurrent (an LSTM of --rnn-hidden units in front of a 256-256-256 student) the same way: (a) its ``update()``
against an eager-torch float32 restatement (nn.LSTM + autograd with the law's detaches) on the same tensors, dones and saved state: `update_ms_hip`,
`update_ms_torch`; (b) its collection loop (3 launches per env step) against the MLP student's (2): `collect_ms_recurrent`, `collect_ms_distill`.  Launches of
one window of P pairs, counted from csrc/go2sim_rdistill.hip, per env block: 1 row list + P cell steps + forward + head + finalize + (2 L + L) backward + P
steps back through time + 4 for the memory's dW / db + 1 reduction + 1 state carry, and 2 for the optimizer per window."""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_runner(envs, steps, distill, gradient_length, seed=3, rnn_hidden=0, sub_envs=None):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_walk_cfgs, init

    init(seed=seed)
    env = Go2Env(envs, *get_walk_cfgs(), seed=seed)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_cfgs_walk.json")))["train_cfg"]
    cfg["num_steps_per_env"], cfg["empirical_normalization"] = steps, False
    if distill:
        cfg["algorithm"] = {"class_name": "Distillation", "num_learning_epochs": 1, "gradient_length": gradient_length, "learning_rate": 1e-3, "max_grad_norm": None,
                            "loss_type": "mse"}
        cfg["policy"] = {"class_name": "StudentTeacher", "activation": "elu", "student_hidden_dims": [256, 256, 256],
                         "teacher_hidden_dims": list(cfg["policy"]["actor_hidden_dims"]), "init_noise_std": 0.1}
        if rnn_hidden:
            cfg["policy"].update(class_name="StudentTeacherRecurrent", rnn_type="lstm", rnn_hidden_dim=rnn_hidden, rnn_num_layers=1)
            cfg["algorithm"]["sub_envs"] = sub_envs
    return OnPolicyRunner(env, cfg)


def collect(runner, steps):
    """the collection part of OnPolicyRunner.learn: no returns, no update"""
    env, alg = runner.env, runner.alg
    obs, extras = env.get_observations()
    a, b = (obs, obs) if runner.distill else (obs, extras["observations"].get("critic", obs))
    for _ in range(steps):
        actions = alg.act(a, b)
        obs, rewards, dones, infos = env.step(actions)
        a, b = (obs, obs) if runner.distill else (obs, infos["observations"].get("critic", obs))
        alg.process_env_step(rewards, dones, infos)
    alg.t = 0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class TorchDistillation:
    """rsl_rl's Distillation.update in eager torch float32 on the device"""

    def __init__(self, dims, device, gradient_length, lr=1e-3):
        layers = []
        for l in range(len(dims) - 1):
            layers.append(torch.nn.Linear(dims[l], dims[l + 1]))
            if l < len(dims) - 2:
                layers.append(torch.nn.ELU())
        self.student = torch.nn.Sequential(*layers).to(device)
        self.opt = torch.optim.Adam(self.student.parameters(), lr=lr)
        self.G = gradient_length

    def update(self, obs, teacher_actions, n_epochs=1):
        mean_loss, loss, cnt = 0, 0, 0
        for _ in range(n_epochs):
            for t in range(obs.shape[0]):
                behavior_loss = torch.nn.functional.mse_loss(self.student(obs[t]), teacher_actions[t])
                loss = loss + behavior_loss
                mean_loss = mean_loss + behavior_loss.detach()
                cnt += 1
                if cnt % self.G == 0:
                    self.opt.zero_grad()
                    loss.backward()
                    self.opt.step()
                    loss = 0
        return (mean_loss / cnt).item()


class TorchRecurrentDistillation:
    """the recurrent branch of rsl_rl's Distillation.update in eager torch float32 on the device, as include/go2sim_rdistill.h states it"""

    def __init__(self, n_in, dims, device, gradient_length, lr=1e-3):
        self.rnn = torch.nn.LSTM(n_in, dims[0], 1).to(device)
        self.student = TorchDistillation(dims, device, gradient_length).student
        self.opt = torch.optim.Adam(list(self.student.parameters()) + list(self.rnn.parameters()), lr=lr)
        self.G = gradient_length

    def update(self, obs, teacher_actions, dones, S, n_epochs=1):
        mean_loss, loss, cnt = 0, 0, 0
        keep = (dones == 0).to(obs.dtype).unsqueeze(-1)
        for _ in range(n_epochs):
            h, c = S[0].unsqueeze(0), S[1].unsqueeze(0)
            for t in range(obs.shape[0]):
                out, (h, c) = self.rnn(obs[t].unsqueeze(0), (h, c))
                behavior_loss = torch.nn.functional.mse_loss(self.student(out[0]), teacher_actions[t])
                loss = loss + behavior_loss
                mean_loss = mean_loss + behavior_loss.detach()
                cnt += 1
                if cnt % self.G == 0:
                    self.opt.zero_grad()
                    loss.backward()
                    self.opt.step()
                    loss = 0
                    h, c = h.detach(), c.detach()
                h, c = h * keep[t], c * keep[t]
        return (mean_loss / cnt).item()


def main_recurrent(args):
    B, T, G, H = args.envs, args.steps, args.gradient_length, args.rnn_hidden
    med = lambda v: sorted(v)[len(v) // 2]
    ppo, dis, rec = make_runner(B, T, False, G), make_runner(B, T, True, G), make_runner(B, T, True, G, rnn_hidden=H, sub_envs=args.sub_envs)
    with tempfile.TemporaryDirectory() as d:                              # the PPO runner's actor is the teacher of both
        ppo.save(os.path.join(d, "teacher.pt"))
        dis.load(os.path.join(d, "teacher.pt")); rec.load(os.path.join(d, "teacher.pt"))
    dev = rec.device

    # (a) the update on one recorded rollout
    collect(rec, T)
    alg = rec.alg
    obs, ta, dones, S = alg.obs.clone(), alg.teacher_actions.clone(), alg.dones.clone(), (alg.saved_h.clone(), alg.saved_c.clone())
    ref = TorchRecurrentDistillation(rec.policy._smem[0], rec.policy._sdims, dev, G)
    sides = {"hip": alg.update, "torch": lambda: ref.update(obs, ta, dones, S)}
    ms_u = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in sides.items():
            ms_u[k].append(timed(fn))

    # (b) the closed collection loop
    runners = {"recurrent": rec, "distill": dis}
    ms_c = {k: [] for k in runners}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, r in runners.items():
            ms_c[k].append(timed(lambda: collect(r, T)))
    rng = lambda v: [round(min(v), 3), round(max(v), 3)]
    from go2_sim2real_locomotion_rl_amd.capi import C

    L, sub = len(rec.policy._sdims) - 1, args.sub_envs or C["GO2SIM_RDISTILL_SUB_ENVS"]
    blocks = (B + sub - 1) // sub
    print(json.dumps({"tool": "distill_bench", "mode": "recurrent", "envs": B, "steps": T, "gradient_length": G, "rounds": args.rounds, "rnn_hidden": H, "sub_envs": sub,
                      "student": rec.policy._sdims, "update_ms_hip": round(med(ms_u["hip"]), 3), "update_ms_torch": round(med(ms_u["torch"]), 3),
                      "update_ms_hip_min_max": rng(ms_u["hip"]), "update_ms_torch_min_max": rng(ms_u["torch"]),
                      "torch_over_hip": round(med(ms_u["torch"]) / med(ms_u["hip"]), 2),
                      "collect_ms_recurrent": round(med(ms_c["recurrent"]), 3), "collect_ms_distill": round(med(ms_c["distill"]), 3),
                      "collect_ms_recurrent_min_max": rng(ms_c["recurrent"]), "collect_ms_distill_min_max": rng(ms_c["distill"]),
                      "launches_per_env_step_act": 3, "env_blocks_per_window": blocks, "launches_per_block_of_a_full_window": 2 * G + 3 * L + 10,
                      "launches_per_window_close": 2}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--recurrent", action="store_true", help="time the recurrent student (Distillation + StudentTeacherRecurrent) instead")
    ap.add_argument("--rnn-hidden", type=int, default=256, help="rnn_hidden_dim of --recurrent")
    ap.add_argument("--sub-envs", type=int, default=None, help="envs of a block of the recurrent update's window walk (default: GO2SIM_RDISTILL_SUB_ENVS)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--gradient-length", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/distill_bench.py needs a ROCm GPU (nothing is measured without one)")
    if args.recurrent:
        return main_recurrent(args)
    B, T, G = args.envs, args.steps, args.gradient_length
    med = lambda v: sorted(v)[len(v) // 2]

    ppo, dis = make_runner(B, T, False, G), make_runner(B, T, True, G)
    with tempfile.TemporaryDirectory() as d:                              # the PPO runner's actor is the teacher
        ppo.save(os.path.join(d, "teacher.pt"))
        dis.load(os.path.join(d, "teacher.pt"))
    dev = dis.device

    # (a) the update on one recorded rollout
    collect(dis, T)
    obs, ta = dis.alg.obs.clone(), dis.alg.teacher_actions.clone()
    ref = TorchDistillation(dis.policy._sdims, dev, G)
    sides = {"hip": dis.alg.update, "torch": lambda: ref.update(obs, ta)}
    ms_u = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in sides.items():
            ms_u[k].append(timed(fn))

    # (b) the closed collection loop
    runners = {"distill": dis, "ppo": ppo}
    ms_c = {k: [] for k in runners}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, r in runners.items():
            ms_c[k].append(timed(lambda: collect(r, T)))
    rng = lambda v: [round(min(v), 3), round(max(v), 3)]
    n_layers = len(dis.policy._sdims) - 1
    print(json.dumps({"tool": "distill_bench", "envs": B, "steps": T, "gradient_length": G, "rounds": args.rounds, "student": dis.policy._sdims,
                      "update_ms_hip": round(med(ms_u["hip"]), 3), "update_ms_torch": round(med(ms_u["torch"]), 3),
                      "update_ms_hip_min_max": rng(ms_u["hip"]), "update_ms_torch_min_max": rng(ms_u["torch"]),
                      "torch_over_hip": round(med(ms_u["torch"]) / med(ms_u["hip"]), 2),
                      "collect_ms_distill": round(med(ms_c["distill"]), 3), "collect_ms_ppo": round(med(ms_c["ppo"]), 3),
                      "collect_ms_distill_min_max": rng(ms_c["distill"]), "collect_ms_ppo_min_max": rng(ms_c["ppo"]),
                      "launches_per_env_step_act": 2, "launches_per_sub_batch": 3 * n_layers + 2, "launches_per_window_close": 3}))


if __name__ == "__main__":
    main()
