#!/usr/bin/env python
"""Times PPO.update() of the library against an eager-torch fp32 restatement of the same update on the same GPU, at the training shape of the
walk task: T = 24 steps x B = 4096 envs, 49 / 104 observations, 16 actions, two 512-256-128 MLPs, 5 epochs x 4 mini-batches of 24 576 rows.

    python tools/ppo_update_bench.py [--updates 5] [--warmup 2] [--envs 4096] [--steps 24] [--shards N] [--symmetry {off,augment,mirror,both}] [--activation NAME]
    python tools/ppo_update_bench.py --recurrent [--rnn-hidden 256] [--collection]

Both sides update from the same rollout (collected once with the library's ActorCritic on random observations and rewards) and the same initial
parameters.  Every shape is warmed up first; device events bracket `--updates` whole updates per side, the two sides alternating update by update so
that other work on the machine hits both alike.  The HIP update ends in its one read of the statistics; the torch restatement reads kl_mean once per
mini-batch, as rsl_rl's adaptive schedule does.  Prints one JSON line: both times per update, their ratio, the matrix work of an update computed
from the shapes (forward, dW and dA of every layer, 2 x rows x in x out each; unpadded) and the fraction of the 157.3 TFLOPS fp32 matrix peak
that the HIP update as a whole achieves (an end-to-end rate over peak, not a kernel's).

--shards N adds the sharded form of the update as a rank of an N-rank job runs it, in this one process: per mini-batch go2sim_ppo_shard_grad, go2sim_ppo_shard_reduce
of N copies of the record (what the all-gather would deliver; the collective itself is NOT in the time), go2sim_ppo_apply, alternating with the plain update.
It reports `sharded_ms_per_update` and the difference to `hip_ms_per_update`.

--symmetry sets the walk env's mirror on the HIP side (symmetry_cfg with Go2Env's tables; mirror_loss_coeff 0.5): the update then handles twice the rows.  The
torch side stays the plain update, so `hip_over_torch` compares unlike work; the time to hold `hip_ms_per_update` against is a plain run at --envs 8192.

--recurrent times the recurrent update (include/go2sim_rnn.h: an LSTM memory of --rnn-hidden units in front of each MLP, env-block mini-batches walked through
time) against eager torch on the same GPU: nn.LSTM stepped over the [T][block] grid with the done mask between steps, plus the MLPs and the same losses.  --collection adds the closed collection loop (Go2Env walk task at --envs, `--steps` env steps of act / step / process_env_step, compute_returns)
timed with the MLP policy and with the recurrent one: `collect_ms_mlp`, `collect_ms_recurrent`."""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MATRIX = 157.3e12
HP = dict(clip_param=0.2, desired_kl=0.01, entropy_coef=0.003, learning_rate=1e-3, max_grad_norm=1.0, value_loss_coef=1.0)
EPOCHS, MINI_BATCHES = 5, 4


TORCH_ACT = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "identity": nn.Identity}
ACTIVATION = "elu"                                             # --activation: both sides' hidden layers (include/go2sim_activation.h)


def mlp(dims):
    layers = []
    for l in range(len(dims) - 1):
        layers.append(nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            layers.append(TORCH_ACT[ACTIVATION]())
    return nn.Sequential(*layers)


class TorchPPO:
    """rsl_rl 2.2.4 PPO.update in eager torch (autograd, Normal, clip_grad_norm_, Adam)"""

    def __init__(self, adims, cdims, state, device):
        self.actor, self.critic = mlp(adims).to(device), mlp(cdims).to(device)
        self.std = nn.Parameter(state["std"].to(device).clone())
        with torch.no_grad():
            for prefix, net in (("actor", self.actor), ("critic", self.critic)):
                for k, p in net.named_parameters():
                    p.copy_(state[f"{prefix}.{k}"])
        self.params = [*self.actor.parameters(), *self.critic.parameters(), self.std]
        self.lr = HP["learning_rate"]
        self.opt = torch.optim.Adam(self.params, lr=self.lr)

    def update(self, ro, perm):
        mbs = perm.numel() // MINI_BATCHES
        clip = HP["clip_param"]
        for _ in range(EPOCHS):
            for i in range(MINI_BATCHES):
                idx = perm[i * mbs:(i + 1) * mbs].long()
                mu = self.actor(ro["obs"][idx])
                v = self.critic(ro["critic_obs"][idx]).squeeze(-1)
                sigma = mu * 0.0 + self.std
                dist = torch.distributions.Normal(mu, sigma)
                logp = dist.log_prob(ro["actions"][idx]).sum(-1)
                entropy = dist.entropy().sum(-1)
                old_mu, old_sigma = ro["old_mu"][idx], ro["old_sigma"][idx]
                with torch.inference_mode():
                    kl = torch.sum(torch.log(sigma / old_sigma + 1.0e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5, dim=-1)
                    kl_mean = float(kl.mean())                                      # the schedule's host read
                if kl_mean > HP["desired_kl"] * 2.0:
                    self.lr = max(1e-5, self.lr / 1.5)
                elif 0.0 < kl_mean < HP["desired_kl"] / 2.0:
                    self.lr = min(1e-2, self.lr * 1.5)
                for g in self.opt.param_groups:
                    g["lr"] = self.lr
                adv, tv, ret = ro["advantages"][idx], ro["target_values"][idx], ro["returns"][idx]
                ratio = torch.exp(logp - ro["old_log_prob"][idx])
                surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
                v_clipped = tv + (v - tv).clamp(-clip, clip)
                value_loss = torch.max((v - ret).pow(2), (v_clipped - ret).pow(2)).mean()
                loss = surrogate + HP["value_loss_coef"] * value_loss - HP["entropy_coef"] * entropy.mean()
                self.opt.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(self.params, HP["max_grad_norm"])
                self.opt.step()


class TorchRecurrentPPO(TorchPPO):
    """The recurrent update in eager torch: two nn.LSTM stepped over the [T][block] grid with the done mask between steps, env-block mini-batches"""

    def __init__(self, n_obs, n_cobs, H, adims, cdims, state, device):
        super().__init__(adims, cdims, state, device)
        self.mem = [nn.LSTM(n_obs, H).to(device), nn.LSTM(n_cobs, H).to(device)]
        with torch.no_grad():
            for prefix, m in zip(("memory_a", "memory_c"), self.mem):
                for k, p in m.named_parameters():
                    p.copy_(state[f"{prefix}.rnn.{k}"])
        self.params = [*self.actor.parameters(), *self.critic.parameters(), *self.mem[0].parameters(), *self.mem[1].parameters(), self.std]
        self.opt = torch.optim.Adam(self.params, lr=self.lr)

    @staticmethod
    def unroll(lstm, x, h, c, keep):
        hs = []
        for t in range(x.shape[0]):
            if t > 0:
                h, c = h * keep[t - 1], c * keep[t - 1]
            out, (hn, cn) = lstm(x[t:t + 1], (h.unsqueeze(0), c.unsqueeze(0)))
            h, c = hn[0], cn[0]
            hs.append(out[0])
        return torch.cat(hs)

    def update(self, ro, saved, T, B):
        clip, nb = HP["clip_param"], B // MINI_BATCHES
        r3 = lambda k, sl: ro[k].reshape(T, B, *ro[k].shape[1:])[:, sl]
        for _ in range(EPOCHS):
            for i in range(MINI_BATCHES):
                sl = slice(i * nb, (i + 1) * nb)
                keep = (r3("dones", sl) == 0).float().unsqueeze(-1)
                mu = self.actor(self.unroll(self.mem[0], r3("obs", sl), saved[0][sl], saved[1][sl], keep))
                v = self.critic(self.unroll(self.mem[1], r3("critic_obs", sl), saved[2][sl], saved[3][sl], keep)).squeeze(-1)
                row = lambda k: r3(k, sl).reshape(T * nb, *ro[k].shape[1:])
                sigma = mu * 0.0 + self.std
                dist = torch.distributions.Normal(mu, sigma)
                logp = dist.log_prob(row("actions")).sum(-1)
                entropy = dist.entropy().sum(-1)
                old_mu, old_sigma = row("old_mu"), row("old_sigma")
                with torch.inference_mode():
                    kl = torch.sum(torch.log(sigma / old_sigma + 1.0e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5, dim=-1)
                    kl_mean = float(kl.mean())
                if kl_mean > HP["desired_kl"] * 2.0:
                    self.lr = max(1e-5, self.lr / 1.5)
                elif 0.0 < kl_mean < HP["desired_kl"] / 2.0:
                    self.lr = min(1e-2, self.lr * 1.5)
                for g in self.opt.param_groups:
                    g["lr"] = self.lr
                adv, tv, ret = row("advantages"), row("target_values"), row("returns")
                ratio = torch.exp(logp - row("old_log_prob"))
                surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
                v_clipped = tv + (v - tv).clamp(-clip, clip)
                value_loss = torch.max((v - ret).pow(2), (v_clipped - ret).pow(2)).mean()
                loss = surrogate + HP["value_loss_coef"] * value_loss - HP["entropy_coef"] * entropy.mean()
                self.opt.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(self.params, HP["max_grad_norm"])
                self.opt.step()


def time_collection(dev, B, T, recurrent, H, reps=3):
    """ms per rollout of the closed loop Go2Env -> policy -> storage (walk task), after one warm-up rollout"""
    from go2_sim2real_locomotion_rl_amd import PPO, ActorCritic, ActorCriticRecurrent, Go2Env, get_walk_cfgs, init

    init(seed=1)
    env = Go2Env(B, *get_walk_cfgs(), seed=1, device=dev)
    obs, extras = env.get_observations()
    cobs = extras["observations"]["critic"]
    hidden = [512, 256, 128]
    pol = (ActorCriticRecurrent(obs.shape[1], cobs.shape[1], env.num_actions, hidden, hidden, rnn_hidden_size=H, device=dev) if recurrent
           else ActorCritic(obs.shape[1], cobs.shape[1], env.num_actions, hidden, hidden, device=dev))
    alg = PPO(pol, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, schedule="adaptive", gamma=0.99, lam=0.95, **HP)
    alg.init_storage(B, T, [obs.shape[1]], [cobs.shape[1]], [env.num_actions])
    total = 0.0
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(T):
            actions = alg.act(obs, cobs)
            obs, rew, dones, infos = env.step(actions)
            cobs = infos["observations"]["critic"]
            alg.process_env_step(rew, dones, infos)
        alg.compute_returns(cobs)
        e1.record()
        torch.cuda.synchronize()
        alg.t = 0
        if rep > 0:
            total += e0.elapsed_time(e1)
    return total / reps


def matrix_flop(adims, cdims, rows):
    f = 0
    for dims in (adims, cdims):
        for l in range(len(dims) - 1):
            f += 2 * rows * dims[l] * dims[l + 1] * (3 if l > 0 else 2)                  # forward, dW, and dA except for the first layer
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--shards", type=int, default=0, help="also time shard_grad + shard_reduce of N copies of the record + apply per mini-batch")
    ap.add_argument("--symmetry", choices=("off", "augment", "mirror", "both"), default="off", help="mirror symmetry on the HIP side (twice the rows)")
    ap.add_argument("--recurrent", action="store_true", help="time the recurrent (LSTM) update against eager torch")
    ap.add_argument("--rnn-hidden", type=int, default=256)
    ap.add_argument("--collection", action="store_true", help="with --recurrent: also time the closed collection loop with the MLP and the recurrent policy")
    ap.add_argument("--activation", choices=sorted(TORCH_ACT), default="elu", help="the hidden layers' activation on both sides")
    args = ap.parse_args()
    global ACTIVATION
    ACTIVATION = args.activation
    if not torch.cuda.is_available():
        raise SystemExit("ppo_update_bench needs a ROCm GPU: a time taken anywhere else says nothing")
    from go2_sim2real_locomotion_rl_amd import PPO, ActorCritic

    dev = torch.device("cuda", 0)
    if args.recurrent:
        return main_recurrent(args, dev)
    T, B, nobs, npriv, nact = args.steps, args.envs, 49, 104, 16
    hidden = [512, 256, 128]
    adims, cdims = [nobs, *hidden, nact], [npriv, *hidden, 1]
    policy = ActorCritic(nobs, npriv, nact, hidden, hidden, activation=args.activation, device=dev, seed=1)
    state = {k: v.clone() for k, v in policy.state_dict().items()}
    sym = None
    if args.symmetry != "off":
        from go2_sim2real_locomotion_rl_amd import get_walk_cfgs
        from go2_sim2real_locomotion_rl_amd.go2_env import mirror_tables

        sym = {"use_data_augmentation": args.symmetry in ("augment", "both"), "use_mirror_loss": args.symmetry in ("mirror", "both"), "mirror_loss_coeff": 0.5,
               "mirror_tables": mirror_tables(*get_walk_cfgs()[:2])}
    alg = PPO(policy, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, schedule="adaptive", gamma=0.99, lam=0.95, seed=1, symmetry_cfg=sym, **HP)
    alg.init_storage(B, T, [nobs], [npriv], [nact])
    g = torch.Generator(device=dev).manual_seed(0)

    def collect():
        for _ in range(T):
            obs, cobs = torch.randn(B, nobs, device=dev, generator=g), torch.randn(B, npriv, device=dev, generator=g)
            alg.act(obs, cobs)
            alg.process_env_step(torch.randn(B, device=dev, generator=g), (torch.rand(B, device=dev, generator=g) < 0.01).to(torch.uint8), {})
        alg.compute_returns(torch.randn(B, npriv, device=dev, generator=g))

    collect()
    flat = lambda t: t.reshape(T * B, *t.shape[2:]).clone()
    ro = dict(obs=flat(alg.obs), critic_obs=flat(alg.critic_obs), actions=flat(alg.actions), old_mu=flat(alg.old_mu), old_sigma=flat(alg.old_sigma),
              old_log_prob=flat(alg.old_log_prob), target_values=flat(alg.storage.values), returns=flat(alg.storage.returns),
              advantages=flat(alg.storage.advantages))
    ref = TorchPPO(adims, cdims, state, dev)
    perm_gen = torch.Generator(device=dev).manual_seed(1)
    torch_update = lambda: ref.update(ro, torch.randperm(T * B // MINI_BATCHES * MINI_BATCHES, device=dev, generator=perm_gen))
    sides = [("hip", alg.update), ("torch", torch_update)]
    if args.shards > 0:
        h, mbs, n_sh = alg._h, alg._mbs, args.shards
        records = torch.empty(n_sh, h.shard_len, dtype=torch.float64, device=dev)
        shard_perm_gen = torch.Generator(device=dev).manual_seed(2)

        def sharded_update():                                                              # PPO._update_sharded with copies in the collective's place
            perm = torch.randperm(MINI_BATCHES * mbs, device=dev, generator=shard_perm_gen).to(torch.int32)
            h.reset_stats()
            for _ in range(EPOCHS):
                for i in range(MINI_BATCHES):
                    h.shard_grad(alg._batch, policy.std, perm[i * mbs:(i + 1) * mbs], n_sh * mbs, records[0])
                    records[1:] = records[0]
                    h.shard_reduce(records, policy.std)
                    h.apply(policy.std)
            h.stats().cpu()                                                                # the update's one read

        sides.append(("sharded", sharded_update))
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    ms = {name: 0.0 for name, _ in sides}
    for _ in range(args.updates):                                                          # alternate the sides update by update
        for name, fn in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms[name] += e0.elapsed_time(e1)
    hip_ms, torch_ms = ms["hip"] / args.updates, ms["torch"] / args.updates
    flop = matrix_flop(adims, cdims, T * B // MINI_BATCHES) * EPOCHS * MINI_BATCHES
    extra = {}
    if args.shards > 0:
        sh_ms = ms["sharded"] / args.updates
        extra = {"shards": args.shards, "sharded_ms_per_update": round(sh_ms, 3), "sharded_minus_hip_ms": round(sh_ms - hip_ms, 3)}
    if sym is not None:
        extra["symmetry"] = args.symmetry
        extra["symmetry_loss"] = alg.symmetry_loss
    print(json.dumps({"tool": "ppo_update_bench", "activation": args.activation, "envs": B, "steps": T, "epochs": EPOCHS, "mini_batches": MINI_BATCHES, "updates_timed": args.updates,
                      "hip_ms_per_update": round(hip_ms, 3), "torch_eager_ms_per_update": round(torch_ms, 3), "hip_over_torch": round(hip_ms / torch_ms, 3),
                      "matrix_flop_per_update": flop, "hip_fraction_of_157.3_tflops": round(flop / (hip_ms * 1e-3) / PEAK_FP32_MATRIX, 4), **extra}))


def main_recurrent(args, dev):
    from go2_sim2real_locomotion_rl_amd import PPO, ActorCriticRecurrent

    T, B, nobs, npriv, nact, H = args.steps, args.envs, 49, 104, 16, args.rnn_hidden
    hidden = [512, 256, 128]
    adims, cdims = [H, *hidden, nact], [H, *hidden, 1]
    policy = ActorCriticRecurrent(nobs, npriv, nact, hidden, hidden, activation=args.activation, rnn_hidden_size=H, device=dev, seed=1)
    state = {k: v.clone() for k, v in policy.state_dict().items()}
    alg = PPO(policy, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, schedule="adaptive", gamma=0.99, lam=0.95, seed=1, **HP)
    alg.init_storage(B, T, [nobs], [npriv], [nact])
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(2):                                                                     # the second rollout starts from a non-zero saved state
        for _ in range(T):
            obs, cobs = torch.randn(B, nobs, device=dev, generator=g), torch.randn(B, npriv, device=dev, generator=g)
            alg.act(obs, cobs)
            alg.process_env_step(torch.randn(B, device=dev, generator=g), (torch.rand(B, device=dev, generator=g) < 0.01).to(torch.uint8), {})
        alg.compute_returns(torch.randn(B, npriv, device=dev, generator=g))
        alg.t = 0
    flat = lambda t: t.reshape(T * B, *t.shape[2:]).clone()
    ro = dict(obs=flat(alg.obs), critic_obs=flat(alg.critic_obs), actions=flat(alg.actions), old_mu=flat(alg.old_mu), old_sigma=flat(alg.old_sigma),
              old_log_prob=flat(alg.old_log_prob), target_values=flat(alg.storage.values), returns=flat(alg.storage.returns),
              advantages=flat(alg.storage.advantages), dones=flat(alg.storage.dones))
    saved = [t.clone() for t in alg._saved]
    ref = TorchRecurrentPPO(nobs, npriv, H, adims, cdims, state, dev)
    sides = [("hip", alg.update), ("torch", lambda: ref.update(ro, saved, T, B))]
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    ms = {name: 0.0 for name, _ in sides}
    for _ in range(args.updates):
        for name, fn in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms[name] += e0.elapsed_time(e1)
    hip_ms, torch_ms = ms["hip"] / args.updates, ms["torch"] / args.updates
    rows = T * B // MINI_BATCHES
    flop = (matrix_flop(adims, cdims, rows) + 2 * rows * H * (adims[1] + cdims[1])                     # the MLPs, with the first layers' dA
            + sum(2 * rows * 4 * H * (n_in + H) * 2 + 2 * rows * 4 * H * H for n_in in (nobs, npriv))) * EPOCHS * MINI_BATCHES   # gates forward + dW, dh through W_hh
    extra = {}
    if args.collection:
        del alg, policy, ref
        extra = {"collect_ms_mlp": round(time_collection(dev, B, T, False, H), 3), "collect_ms_recurrent": round(time_collection(dev, B, T, True, H), 3)}
    print(json.dumps({"tool": "ppo_update_bench", "activation": args.activation, "recurrent": True, "rnn_hidden": H, "envs": B, "steps": T, "epochs": EPOCHS, "mini_batches": MINI_BATCHES,
                      "updates_timed": args.updates, "hip_ms_per_update": round(hip_ms, 3), "torch_eager_ms_per_update": round(torch_ms, 3),
                      "hip_over_torch": round(hip_ms / torch_ms, 3), "matrix_flop_per_update": flop,
                      "hip_fraction_of_157.3_tflops": round(flop / (hip_ms * 1e-3) / PEAK_FP32_MATRIX, 4), **extra}))


if __name__ == "__main__":
    main()
