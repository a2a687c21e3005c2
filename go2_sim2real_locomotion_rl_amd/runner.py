"""OnPolicyRunner -- the part of ``rsl_rl.runners.OnPolicyRunner`` (rsl-rl-lib==2.2.4) the train scripts use
(examples/locomotion/final/go2_train_walk.py:475-476): it takes the reference's ``train_cfg`` dictionary unchanged and closes
``Go2Env -> ActorCritic -> RolloutStorage -> PPO.update()`` into a training loop that stays on the device.

    runner = OnPolicyRunner(env, get_train_cfg("go2-walk", 1000), log_dir="logs/go2-walk")
    log = runner.learn(num_learning_iterations=1000, init_at_random_ep_len=True)
    policy = runner.get_inference_policy()

No TensorBoard: ``learn`` returns one dictionary per iteration.  The reward / episode-length means are taken over the episodes that ended
during the iteration (the reference averages its last 100 finished episodes); they are counted on the device and read once per iteration,
after the update's own read of its statistics.

Under ``torchrun`` every rank builds its shard of the envs (``Go2Env(n_local, ..., shared_globals=True)``) and a runner; the runners train one policy
(ppo.PPO with the process group): rank 0's initial weights, per-rank noise and permutation streams, one curriculum, gradients summed in rank order,
global means in every rank's log, checkpoints written by rank 0 (tools/train.py).

``train_cfg["empirical_normalization"]`` (off in the reference's train scripts) puts ``normalization.EmpiricalNormalization`` in front of the policy, as rsl_rl
does: ``obs_normalizer`` and ``critic_obs_normalizer`` (``until = 1e8``) step together after every ``env.step``, the policy sees and stores the normalised rows,
the checkpoint gains ``obs_norm_state_dict`` / ``critic_obs_norm_state_dict`` and ``get_inference_policy()`` normalises before it acts.  The observations
``learn()`` starts from are normalised with the statistics as they are and are not counted (DESIGN.md "Empirical normalisation").
"""
import os

import torch

from .capi import Go2SimError
from .distributed import is_multi, shard_seed, sum_in_rank_order
from .eval_io import read_checkpoint, save_checkpoint
from .normalization import EmpiricalNormalization, norm_step
from .policy import ActorCritic, ActorCriticRecurrent
from .ppo import PPO


class OnPolicyRunner:
    def __init__(self, env, train_cfg, log_dir=None, device=None, group=None):
        self.cfg, self.env, self.log_dir = train_cfg, env, log_dir
        self.device = torch.device(device) if device is not None else env.device
        self.empirical_normalization = bool(train_cfg.get("empirical_normalization"))
        alg_cfg, pol_cfg = dict(train_cfg["algorithm"]), dict(train_cfg["policy"])
        pol_class = pol_cfg.pop("class_name", "ActorCritic")
        if alg_cfg.pop("class_name", "PPO") != "PPO" or pol_class not in ("ActorCritic", "ActorCriticRecurrent"):
            raise Go2SimError("go2sim implements class_name PPO / ActorCritic / ActorCriticRecurrent")
        pol_class = ActorCriticRecurrent if pol_class == "ActorCriticRecurrent" else ActorCritic
        sym = alg_cfg.get("symmetry_cfg")
        if sym and sym.get("mirror_tables") is None and sym.get("data_augmentation_func") is None:
            alg_cfg["symmetry_cfg"] = dict(sym, mirror_tables=env.mirror_tables())     # the env knows its own observation layout
        obs, extras = env.get_observations()
        critic_obs = extras["observations"].get("critic", obs)
        seed = int(train_cfg.get("seed", 1) or 1)
        if group is None and is_multi():
            group = torch.distributed.group.WORLD
        self.group = group if group is not None and is_multi(group) else None
        self.rank = torch.distributed.get_rank(self.group) if self.group is not None else 0
        # the noise stream is the rank's own; the initial weights drawn from the same seed are replaced by rank 0's at the end of init_storage
        self.policy = pol_class(obs.shape[1], critic_obs.shape[1], env.num_actions, device=self.device, seed=shard_seed(seed, self.rank), **pol_cfg)
        self.alg = PPO(self.policy, device=self.device, seed=seed, group=self.group, **alg_cfg)
        self.num_steps_per_env = int(train_cfg["num_steps_per_env"])
        self.save_interval = int(train_cfg.get("save_interval", 0) or 0)
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [obs.shape[1]], [critic_obs.shape[1]], [env.num_actions])
        self.obs_normalizer = self.critic_obs_normalizer = None
        if self.empirical_normalization:
            # both exist even when the env gives no critic observations (the second then stays unused: the critic reads the normalised actor rows)
            self.obs_normalizer = EmpiricalNormalization([obs.shape[1]], until=1.0e8, device=self.device)
            self.critic_obs_normalizer = EmpiricalNormalization([critic_obs.shape[1]], until=1.0e8, device=self.device)
        self.current_learning_iteration = 0
        self._last_means = (0.0, 0.0)
        self._cur_rew, self._cur_len = torch.zeros(env.num_envs, device=self.device), torch.zeros(env.num_envs, device=self.device)

    def _normalize(self, obs, critic, update):
        """Both observation sets through one norm_step call (`critic` is None when the env has no critic observations: the critic then reads the normalised
        actor rows).  The results are the normalisers' own buffers: the env's tensors, which get_observations() hands out again, are not written."""
        if critic is None:
            y, _ = norm_step(self.obs_normalizer, obs, update=update, group=self.group)
            return y, y
        return norm_step(self.obs_normalizer, obs, self.critic_obs_normalizer, critic, update=update, group=self.group)

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        env, alg, dev = self.env, self.alg, self.device
        if init_at_random_ep_len:
            env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
        obs, extras = env.get_observations()
        critic_obs = extras["observations"].get("critic", obs)
        norm = self.empirical_normalization
        if norm:                                                              # the starting observations: current statistics, not counted
            obs, critic_obs = self._normalize(obs, extras["observations"].get("critic"), update=False)
        cur_rew, cur_len = self._cur_rew, self._cur_len                       # running episodes carry over from one learn() to the next
        log = []
        start = self.current_learning_iteration
        for it in range(start, start + num_learning_iterations):
            acc = torch.zeros(3, device=dev, dtype=torch.float64)            # finished episodes: count, sum of rewards, sum of lengths
            for _ in range(self.num_steps_per_env):
                actions = alg.act(obs, critic_obs)
                obs, rewards, dones, infos = env.step(actions)
                critic_obs = infos["observations"].get("critic", obs)
                if norm:
                    obs, critic_obs = self._normalize(obs, infos["observations"].get("critic"), update=True)
                alg.process_env_step(rewards, dones, infos)
                cur_rew += rewards; cur_len += 1
                d = (dones > 0).to(torch.float64)
                acc += torch.stack([d.sum(), (d * cur_rew).sum(), (d * cur_len).sum()])
                keep = (dones == 0).to(cur_rew.dtype)
                cur_rew *= keep; cur_len *= keep
            if getattr(env, "_shared_globals", False):
                env.sync_globals(self.group)                                   # one curriculum and one set of global DR draws for all shards
            alg.compute_returns(critic_obs)
            value_loss, surrogate_loss, entropy = alg.update()
            n, rs, ls = sum_in_rank_order(acc, self.group).tolist()            # every rank logs the global means
            if n > 0:
                self._last_means = (rs / n, ls / n)
            self.current_learning_iteration = it + 1
            log.append({"iteration": it, "mean_reward": self._last_means[0], "mean_episode_length": self._last_means[1], "value_loss": value_loss,
                        "surrogate_loss": surrogate_loss, "entropy": entropy, "learning_rate": alg.learning_rate})
            if alg.symmetry is not None:
                log[-1]["symmetry_loss"] = alg.symmetry_loss
            if self.log_dir is not None and self.save_interval > 0 and (it + 1) % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it + 1}.pt"))
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
        return log

    def save(self, path, infos=None):
        """rsl_rl 2.2.4 checkpoint layout (eval_io.read_checkpoint): model_state_dict, optimizer_state_dict (Adam's m, v, step, learning rate), iter, infos."""
        if self.rank != 0:                                                     # the ranks hold the same bits: rank 0 writes them
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        opt = self.alg.optimizer_state_dict()
        opt["policy_noise_step"] = int(self.policy._step)
        if self.empirical_normalization:
            save_checkpoint(path, self.policy.state_dict(), opt, self.current_learning_iteration, infos, obs_norm_state_dict=self.obs_normalizer.state_dict(),
                            critic_obs_norm_state_dict=self.critic_obs_normalizer.state_dict())
        else:
            save_checkpoint(path, self.policy.state_dict(), opt, self.current_learning_iteration, infos)

    def load(self, path, load_optimizer=True):
        ckpt = read_checkpoint(path)
        has_norm = [k for k in ("obs_norm_state_dict", "critic_obs_norm_state_dict") if ckpt.get(k) is not None]
        if self.empirical_normalization and len(has_norm) != 2:
            raise Go2SimError(f"{path}: empirical_normalization is on, but the checkpoint has no obs_norm_state_dict / critic_obs_norm_state_dict")
        if not self.empirical_normalization and has_norm:
            raise Go2SimError(f"{path}: the checkpoint carries {has_norm} (its policy was trained on normalised observations), but empirical_normalization "
                              "is off in this runner's train_cfg")
        self.policy.load_state_dict(ckpt["model_state_dict"])
        opt = ckpt.get("optimizer_state_dict") or {}
        if load_optimizer and "exp_avg" in opt:
            self.alg.load_optimizer_state_dict(opt)
            self.policy._step = int(opt.get("policy_noise_step", self.policy._step))
        self.alg.broadcast_parameters()                                        # every rank read the file; rank 0's parameters are the ones in force
        if self.empirical_normalization:                                      # every rank read the same file: nothing to broadcast
            self.obs_normalizer.load_state_dict(ckpt["obs_norm_state_dict"])
            self.critic_obs_normalizer.load_state_dict(ckpt["critic_obs_norm_state_dict"])
        self.current_learning_iteration = int(ckpt.get("iter", 0) or 0)
        return ckpt.get("infos")

    def get_inference_policy(self, device=None):
        """The deterministic policy as a callable.  A recurrent policy keeps its memory between calls: the caller resets it through
        ``runner.policy.reset(dones)`` after every env step, as the collection loop does.  With empirical normalisation the callable first applies the actor
        normaliser without moving its statistics (rsl_rl puts it in eval mode here); the raw observations are not written."""
        if not self.empirical_normalization:
            return self.policy.act_inference
        normalizer, act = self.obs_normalizer, self.policy.act_inference
        return lambda observations: act(norm_step(normalizer, observations, update=False)[0])
