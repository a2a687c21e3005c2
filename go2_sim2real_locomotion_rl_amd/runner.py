"""OnPolicyRunner -- the part of ``rsl_rl.runners.OnPolicyRunner`` (rsl-rl-lib==2.2.4) the train scripts use
(examples/locomotion/final/go2_train_walk.py:475-476): it takes the reference's ``train_cfg`` dictionary unchanged and closes
``Go2Env -> ActorCritic -> RolloutStorage -> PPO.update()`` into a training loop that stays on the device.

    runner = OnPolicyRunner(env, get_train_cfg("go2-walk", 1000), log_dir="logs/go2-walk")
    log = runner.learn(num_learning_iterations=1000, init_at_random_ep_len=True)
    policy = runner.get_inference_policy()

No TensorBoard: ``learn`` returns one dictionary per iteration.  The reward / episode-length means are taken over the episodes that ended
during the iteration (the reference averages its last 100 finished episodes); they are counted on the device and read once per iteration,
after the update's own read of its statistics.  The env's ``extras["episode"]`` means of the iteration's last step (``rew_<term>``, rsl_rl's
"Episode/rew_<term>") ride in the same entry, read in one stacked copy.

Under ``torchrun`` every rank builds its shard of the envs (``Go2Env(n_local, ..., shared_globals=True)``) and a runner; the runners train one policy
(ppo.PPO with the process group): rank 0's initial weights, per-rank noise and permutation streams, one curriculum, gradients summed in rank order,
global means in every rank's log, checkpoints written by rank 0 (tools/train.py).

``train_cfg["empirical_normalization"]`` (off in the reference's train scripts) puts ``normalization.EmpiricalNormalization`` in front of the policy, as rsl_rl
does: ``obs_normalizer`` and ``critic_obs_normalizer`` (``until = 1e8``) step together after every ``env.step``, the policy sees and stores the normalised rows,
the checkpoint gains ``obs_norm_state_dict`` / ``critic_obs_norm_state_dict`` and ``get_inference_policy()`` normalises before it acts.  The observations
``learn()`` starts from are normalised with the statistics as they are and are not counted (DESIGN.md "Empirical normalisation").

``train_cfg["obs_groups"]`` (optional) maps the roles ``policy``, ``critic`` and ``teacher`` to the env's observation groups ``"policy"`` (what
``get_observations()`` returns) or ``"critic"`` (``extras["observations"]["critic"]``).  ``{"policy": "critic"}`` on a PPO run trains an actor on the
privileged rows -- a teacher.  ``algorithm.class_name == "Distillation"`` with ``policy.class_name == "StudentTeacher"`` or ``"StudentTeacherRecurrent"``
(distillation.py; the second puts an LSTM memory in front of the student and needs ``rnn_hidden_dim``) distils such a teacher into a student: ``load(teacher_checkpoint)`` fills the teacher, ``learn()`` collects with the student and regresses it onto the teacher's actions,
the log carries ``behavior_loss``.  A teacher checkpoint's ``obs_norm_state_dict`` becomes a frozen teacher normaliser that is always applied (it is part of
the teacher's function) and is saved as ``privileged_obs_norm_state_dict`` (DESIGN.md "Distillation").

``train_cfg["algorithm"]["rnd_cfg"]`` (rsl_rl's random network distillation; rnd.py, DESIGN.md "RND") adds a curiosity bonus to the reward: the role ``rnd_state`` of
``obs_groups`` (default ``"policy"``) names the rows the two networks embed and sizes them (``num_states``), ``weight`` is multiplied by ``env.dt`` on a copy of
the cfg, the log gains ``rnd_loss``, ``mean_intrinsic_reward``, ``mean_extrinsic_reward`` and ``rnd_weight``, and a checkpoint ``rnd_state_dict`` /
``rnd_optimizer_state_dict``.  One rank only.
"""
import os
import sys

import torch

from .capi import Go2SimError
from .distillation import Distillation, StudentTeacher, StudentTeacherRecurrent
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
        alg_class = alg_cfg.pop("class_name", "PPO")
        pairings = {"PPO": ("ActorCritic", "ActorCriticRecurrent"), "Distillation": ("StudentTeacher", "StudentTeacherRecurrent")}
        if alg_class not in pairings or pol_class not in pairings[alg_class]:
            raise Go2SimError(f"go2sim implements class_name PPO with ActorCritic / ActorCriticRecurrent and Distillation with StudentTeacher / "
                              f"StudentTeacherRecurrent; algorithm {alg_class!r} with policy {pol_class!r} is not one of these pairings")
        self.distill = alg_class == "Distillation"
        self.obs_groups = self._check_obs_groups(train_cfg.get("obs_groups"))
        obs, extras = env.get_observations()
        self._roles(obs, extras["observations"])                              # an env without the group a role names is refused here
        sym = alg_cfg.get("symmetry_cfg")
        if sym and sym.get("mirror_tables") is None and sym.get("data_augmentation_func") is None:
            tables = dict(env.mirror_tables())                                 # the env knows its own observation layout
            if self.obs_groups:                                                # a role that reads the other group mirrors with that group's table
                env_tables = dict(tables)
                for role in ("policy", "critic"):
                    if role in self.obs_groups:
                        tables[role] = env_tables[self.obs_groups[role]]
            alg_cfg["symmetry_cfg"] = dict(sym, mirror_tables=tables)
        seed = int(train_cfg.get("seed", 1) or 1)
        if group is None and is_multi():
            group = torch.distributed.group.WORLD
        self.group = group if group is not None and is_multi(group) else None
        self.rank = torch.distributed.get_rank(self.group) if self.group is not None else 0
        self.num_steps_per_env = int(train_cfg["num_steps_per_env"])
        self.save_interval = int(train_cfg.get("save_interval", 0) or 0)
        self.current_learning_iteration = 0
        self._last_means = (0.0, 0.0)
        self._kind = f"{alg_class}/{pol_class}"                                # what a checkpoint's runner_state_dict must come from
        self.save_env_state = False                                            # learn()'s own checkpoints: with the env's and the loop's state (save(env_state=True))
        self._resumed = False                                                  # load() put an env state back: the next learn() re-randomises nothing
        self._last_rows = self._resume_rows = None                             # the rows the next act reads: as learn() left them / as load() restored them
        self._cur_rew, self._cur_len = torch.zeros(env.num_envs, device=self.device), torch.zeros(env.num_envs, device=self.device)
        self.obs_normalizer = self.critic_obs_normalizer = self.privileged_obs_normalizer = None
        self.rnd = None
        if self.distill:
            if self.group is not None:
                raise Go2SimError("Distillation over a multi-rank group is not implemented (the sharded distillation update is a follow-up)")
            s_obs, _, t_obs = self._roles(obs, extras["observations"])
            st_class = StudentTeacherRecurrent if pol_class == "StudentTeacherRecurrent" else StudentTeacher   # the recurrent class refuses a config without rnn_hidden_dim
            self.policy = st_class(s_obs.shape[1], t_obs.shape[1], env.num_actions, device=self.device, seed=seed, **pol_cfg)
            self.alg = Distillation(self.policy, device=self.device, **alg_cfg)
            self.alg.init_storage(env.num_envs, self.num_steps_per_env, [s_obs.shape[1]], [t_obs.shape[1]], [env.num_actions])
            if self.empirical_normalization:                                  # the student's normaliser learns as the actor's does in a PPO run
                self.obs_normalizer = EmpiricalNormalization([s_obs.shape[1]], until=1.0e8, device=self.device)
            return
        obs, critic_raw, _ = self._roles(obs, extras["observations"])
        critic_obs = obs if critic_raw is None else critic_raw
        pol_class = ActorCriticRecurrent if pol_class == "ActorCriticRecurrent" else ActorCritic
        # the noise stream is the rank's own; the initial weights drawn from the same seed are replaced by rank 0's at the end of init_storage
        self.policy = pol_class(obs.shape[1], critic_obs.shape[1], env.num_actions, device=self.device, seed=shard_seed(seed, self.rank), **pol_cfg)
        if alg_cfg.get("rnd_cfg"):
            if self.group is not None:
                raise Go2SimError("rnd_cfg over a multi-rank group is not implemented (the sharded predictor update is a follow-up)")
            # on a copy: the width of the rows the role reads, and the weight per env step scaled by the step's length as rsl_rl's runner does
            rnd_cfg = dict(alg_cfg["rnd_cfg"], num_states=int(self._rnd_rows(*env.get_observations()).shape[1]))
            rnd_cfg["weight"] = float(rnd_cfg.get("weight", 0.0)) * float(env.dt)
            alg_cfg["rnd_cfg"] = rnd_cfg
        self.alg = PPO(self.policy, device=self.device, seed=seed, group=self.group, **alg_cfg)
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [obs.shape[1]], [critic_obs.shape[1]], [env.num_actions])
        self.rnd = self.alg.rnd
        if self.rnd is not None:                                              # running episodes' two reward parts, counted as _count_episodes counts the sum
            self._cur_int, self._cur_ext = torch.zeros(env.num_envs, device=self.device), torch.zeros(env.num_envs, device=self.device)
            self._last_rnd_means = (0.0, 0.0)
        if self.empirical_normalization:
            # both exist even when the env gives no critic observations (the second then stays unused: the critic reads the normalised actor rows)
            self.obs_normalizer = EmpiricalNormalization([obs.shape[1]], until=1.0e8, device=self.device)
            self.critic_obs_normalizer = EmpiricalNormalization([critic_obs.shape[1]], until=1.0e8, device=self.device)

    ROLES, GROUPS = ("policy", "critic", "teacher", "rnd_state"), ("policy", "critic")

    @classmethod
    def _check_obs_groups(cls, cfg):
        """train_cfg["obs_groups"]: {role: env group}; -> dict (empty when absent: everything as without it)"""
        if not cfg:
            return {}
        bad_roles = sorted(set(cfg) - set(cls.ROLES))
        if bad_roles:
            raise Go2SimError(f"obs_groups: unknown role(s) {bad_roles}; the roles are {list(cls.ROLES)}")
        bad = {r: g for r, g in cfg.items() if g not in cls.GROUPS}
        if bad:
            raise Go2SimError(f"obs_groups: unknown observation group(s) {bad}; the env's groups are {list(cls.GROUPS)}")
        return dict(cfg)

    def _roles(self, obs, observations):
        """The env's rows by role: -> (policy rows, critic rows or None, teacher rows).  Without obs_groups: the env's policy group, its critic group (None
        when it has none: the critic then reads what the policy reads), and the policy group for the teacher."""
        def group(name):
            if name == "policy":
                return obs
            if "critic" not in observations:
                raise Go2SimError("obs_groups names the group 'critic', but the env gives no critic observations")
            return observations["critic"]
        g = self.obs_groups
        critic = group(g["critic"]) if "critic" in g else observations.get("critic")
        return group(g.get("policy", "policy")), critic, group(g.get("teacher", "policy"))

    def _rnd_rows(self, obs, extras):
        """the env's raw rows of the role rnd_state (default: the policy group); `extras` is what the env returned next to obs"""
        if self.obs_groups.get("rnd_state", "policy") == "policy":
            return obs
        if "critic" not in extras["observations"]:
            raise Go2SimError("obs_groups names the group 'critic', but the env gives no critic observations")
        return extras["observations"]["critic"]

    def _normalize(self, obs, critic, update):
        """Both observation sets through one norm_step call (`critic` is None when the env has no critic observations: the critic then reads the normalised
        actor rows).  The results are the normalisers' own buffers: the env's tensors, which get_observations() hands out again, are not written."""
        if critic is None:
            y, _ = norm_step(self.obs_normalizer, obs, update=update, group=self.group)
            return y, y
        return norm_step(self.obs_normalizer, obs, self.critic_obs_normalizer, critic, update=update, group=self.group)

    def _rows(self, obs, observations, update):
        """The env's rows of one step as the pair ``alg.act`` takes, normalised where a normaliser exists (`update`: the learning ones count the rows):
        (actor rows, critic rows) for PPO, (student rows, teacher rows) for distillation."""
        if self.distill:
            return self._distill_rows(obs, observations, update)
        obs, critic_raw, _ = self._roles(obs, observations)
        if self.empirical_normalization:
            return self._normalize(obs, critic_raw, update=update)
        return obs, (obs if critic_raw is None else critic_raw)

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        env, alg, dev = self.env, self.alg, self.device
        if self.distill and not self.policy.loaded_teacher:
            raise Go2SimError("learn(): no teacher has been loaded; load a PPO checkpoint (the teacher) or a distillation checkpoint with runner.load(path) first")
        resumed, self._resumed = self._resumed, False
        if self._resume_rows is not None:
            # a checkpoint with the env's state was loaded: the episode lengths, the observations and the rows the interrupted loop was about to act on
            # are the saved ones; nothing the state carries is read again or drawn again
            rows, self._resume_rows = self._resume_rows, None
        else:
            if init_at_random_ep_len and not resumed:
                env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
            obs, extras = env.get_observations()
            rows = self._rows(obs, extras["observations"], update=False)      # the starting observations: current statistics, not counted
        log = []
        start = self.current_learning_iteration
        for it in range(start, start + num_learning_iterations):
            acc = torch.zeros(3, device=dev, dtype=torch.float64)            # finished episodes: count, sum of rewards, sum of lengths
            acc_rnd = torch.zeros(2, device=dev, dtype=torch.float64) if self.rnd is not None else None      # their intrinsic and extrinsic reward sums
            for _ in range(self.num_steps_per_env):
                actions = alg.act(*rows)
                obs, rewards, dones, infos = env.step(actions)
                rows = self._rows(obs, infos["observations"], update=True)
                if self.rnd is not None:
                    alg.process_env_step(rewards, dones, infos, self._rnd_rows(obs, infos))
                    self._count_rnd(acc_rnd, alg.intrinsic_rewards, rewards, dones)
                else:
                    alg.process_env_step(rewards, dones, infos)
                self._count_episodes(acc, rewards, dones)
            if not self.distill and getattr(env, "_shared_globals", False):
                env.sync_globals(self.group)                                   # one curriculum and one set of global DR draws for all shards
            alg.compute_returns(rows[1])                                       # nothing for distillation: the targets are the stored teacher actions
            results = alg.update()
            if self.rnd is not None:                                           # one rank: the two extra sums ride in the same read
                n, rs, ls, ri, re = torch.cat([acc, acc_rnd]).tolist()
                if n > 0:
                    self._last_rnd_means = (ri / n, re / n)
            else:
                n, rs, ls = (acc if self.distill else sum_in_rank_order(acc, self.group)).tolist()      # every rank logs the global means; distillation is one rank
            if n > 0:
                self._last_means = (rs / n, ls / n)
            self.current_learning_iteration = it + 1
            self._last_rows = rows
            log.append({"iteration": it, "mean_reward": self._last_means[0], "mean_episode_length": self._last_means[1],
                        **dict(zip(alg.result_names, results if isinstance(results, tuple) else (results,))), "learning_rate": alg.learning_rate})
            episode = infos.get("episode") if isinstance(infos, dict) else None
            if episode:                                                        # the env's per-term episode means (rsl_rl's "Episode/rew_*"), one read
                keys = [k for k in episode if k not in log[-1]]
                log[-1].update(zip(keys, torch.stack([torch.as_tensor(episode[k], device=dev).detach().to(torch.float32).reshape(()) for k in keys]).tolist()))
            if alg.symmetry is not None:
                log[-1]["symmetry_loss"] = alg.symmetry_loss
            if self.rnd is not None:
                log[-1].update(mean_intrinsic_reward=self._last_rnd_means[0], mean_extrinsic_reward=self._last_rnd_means[1], rnd_weight=self.rnd.weight)
            if self.log_dir is not None and self.save_interval > 0 and (it + 1) % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it + 1}.pt"), env_state=self.save_env_state)
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"), env_state=self.save_env_state)
        return log

    def _count_episodes(self, acc, rewards, dones):
        """acc += (finished episodes, their reward sum, their length sum); running episodes carry over from one learn() to the next"""
        cur_rew, cur_len = self._cur_rew, self._cur_len
        cur_rew += rewards; cur_len += 1
        d = (dones > 0).to(torch.float64)
        acc += torch.stack([d.sum(), (d * cur_rew).sum(), (d * cur_len).sum()])
        keep = (dones == 0).to(cur_rew.dtype)
        cur_rew *= keep; cur_len *= keep

    def _count_rnd(self, acc_rnd, intrinsic, rewards, dones):
        """acc_rnd += (intrinsic, extrinsic) reward sums of the episodes that ended in this step, with _count_episodes's accounting"""
        self._cur_int += intrinsic; self._cur_ext += rewards
        d = (dones > 0).to(torch.float64)
        acc_rnd += torch.stack([(d * self._cur_int).sum(), (d * self._cur_ext).sum()])
        keep = (dones == 0).to(self._cur_int.dtype)
        self._cur_int *= keep; self._cur_ext *= keep

    # ---- distillation ----------------------------------------------------------------------------------------
    def _distill_rows(self, obs, observations, update):
        """The student's and the teacher's rows of one env step, each through its normaliser where it has one: the student's learns (`update`), the
        teacher's is frozen and always applied.  The results are the normalisers' own buffers or the env's tensors, which are not written."""
        s_obs, _, t_obs = self._roles(obs, observations)
        if self.obs_normalizer is not None:
            s_obs = norm_step(self.obs_normalizer, s_obs, update=update)[0]
        if self.privileged_obs_normalizer is not None:
            t_obs = norm_step(self.privileged_obs_normalizer, t_obs, update=False)[0]
        return s_obs, t_obs

    def _load_distill(self, ckpt, path):
        """A PPO checkpoint is the teacher: teacher.* <- actor.* (for a StudentTeacherRecurrent with a recurrent teacher also memory_t.* <- memory_a.*), its
        actor normaliser becomes the frozen teacher normaliser; the student, the iteration and the optimizer are untouched.  A distillation checkpoint
        resumes: student, teacher, (the memories,) std and both normalisers.  -> resume"""
        resume = self.policy.load_state_dict(ckpt["model_state_dict"])
        t_norm = ckpt.get("privileged_obs_norm_state_dict" if resume else "obs_norm_state_dict")
        if t_norm is not None:
            if self.privileged_obs_normalizer is None:
                self.privileged_obs_normalizer = EmpiricalNormalization([self.policy.num_teacher_obs], until=1.0e8, device=self.device).eval()
            self.privileged_obs_normalizer.load_state_dict(t_norm)
        elif resume:
            self.privileged_obs_normalizer = None
        if resume and self.empirical_normalization:
            if ckpt.get("obs_norm_state_dict") is None:
                raise Go2SimError(f"{path}: empirical_normalization is on, but the distillation checkpoint has no obs_norm_state_dict")
            self.obs_normalizer.load_state_dict(ckpt["obs_norm_state_dict"])
        elif resume and ckpt.get("obs_norm_state_dict") is not None:
            raise Go2SimError(f"{path}: the checkpoint's student was trained on normalised observations (obs_norm_state_dict), but empirical_normalization "
                              "is off in this runner's train_cfg")
        return resume

    def _load_ppo(self, ckpt, path):
        has_norm = [k for k in ("obs_norm_state_dict", "critic_obs_norm_state_dict") if ckpt.get(k) is not None]
        if self.empirical_normalization and len(has_norm) != 2:
            raise Go2SimError(f"{path}: empirical_normalization is on, but the checkpoint has no obs_norm_state_dict / critic_obs_norm_state_dict")
        if not self.empirical_normalization and has_norm:
            raise Go2SimError(f"{path}: the checkpoint carries {has_norm} (its policy was trained on normalised observations), but empirical_normalization "
                              "is off in this runner's train_cfg")
        has_rnd = [k for k in ("rnd_state_dict", "rnd_optimizer_state_dict") if ckpt.get(k) is not None]
        if self.rnd is not None and len(has_rnd) != 2:
            raise Go2SimError(f"{path}: rnd_cfg is set, but the checkpoint has no rnd_state_dict / rnd_optimizer_state_dict")
        if self.rnd is None and has_rnd:
            raise Go2SimError(f"{path}: the checkpoint carries {has_rnd} (it was trained with random network distillation), but this runner's train_cfg has no rnd_cfg")
        self.policy.load_state_dict(ckpt["model_state_dict"])
        self.alg.broadcast_parameters()                                        # every rank read the file; rank 0's parameters are the ones in force
        if self.empirical_normalization:                                      # every rank read the same file: nothing to broadcast
            self.obs_normalizer.load_state_dict(ckpt["obs_norm_state_dict"])
            self.critic_obs_normalizer.load_state_dict(ckpt["critic_obs_norm_state_dict"])
        if self.rnd is not None:
            self.rnd.load_state_dict(ckpt["rnd_state_dict"])
        return True

    # ---- the collection loop's own state (checkpoints with env_state) ---------------------------------------------
    def _memories(self):
        """the policy's memory states that exist and have stepped (module_core.MemoryState)"""
        return [(k, st) for k, st in enumerate(getattr(self.policy, "_hid", ())) if st is not None and st.B > 0]

    def runner_state_dict(self):
        """What the collection loop carries from one iteration to the next, as CPU tensors and plain numbers: the rows the next act reads, the running
        episodes' sums behind mean_reward / mean_episode_length (and RND's pair), the last means, and every memory's (h, c) as the next step enters it."""
        cpu = lambda t: t.detach().cpu().clone()
        sd = {"kind": self._kind, "num_envs": int(self.env.num_envs), "cur_rew": cpu(self._cur_rew), "cur_len": cpu(self._cur_len),
              "last_means": [float(v) for v in self._last_means]}
        if self._last_rows is not None:
            sd["rows"] = [cpu(r) for r in self._last_rows]
        if self.rnd is not None:
            sd.update(cur_int=cpu(self._cur_int), cur_ext=cpu(self._cur_ext), last_rnd_means=[float(v) for v in self._last_rnd_means])
        for k, st in self._memories():
            h, c = torch.empty_like(st.h), torch.empty_like(st.c)
            st.copy_entering(h, c)
            sd[f"memory_{k}_h"], sd[f"memory_{k}_c"] = h.cpu(), c.cpu()
        return sd

    def load_runner_state_dict(self, sd):
        """puts back a runner_state_dict() of a runner of this kind and size (runner_state_matches)"""
        if not self.runner_state_matches(sd):
            raise Go2SimError(f"the runner state was saved by a {sd.get('kind')!r} runner with {sd.get('num_envs')} envs, this one is {self._kind!r} with {self.env.num_envs}")
        dev = self.device
        self._cur_rew.copy_(sd["cur_rew"]); self._cur_len.copy_(sd["cur_len"])
        self._last_means = tuple(float(v) for v in sd["last_means"])
        if self.rnd is not None:
            self._cur_int.copy_(sd["cur_int"]); self._cur_ext.copy_(sd["cur_ext"])
            self._last_rnd_means = tuple(float(v) for v in sd["last_rnd_means"])
        for k, st in enumerate(getattr(self.policy, "_hid", ())):
            if st is not None and f"memory_{k}_h" in sd:
                h = sd[f"memory_{k}_h"].to(dev)
                st.rows(h.shape[0])
                st.zero()                                                      # (drops a pending mask: the saved state is the entering one)
                st.h.copy_(h); st.c.copy_(sd[f"memory_{k}_c"].to(dev))
        self._resume_rows = self._last_rows = tuple(r.to(dev) for r in sd["rows"]) if "rows" in sd else None
        self._resumed = True

    def runner_state_matches(self, sd):
        return sd.get("kind") == self._kind and int(sd.get("num_envs", -1)) == int(self.env.num_envs)

    def save(self, path, infos=None, env_state=False):
        """rsl_rl 2.2.4 checkpoint layout (eval_io.read_checkpoint): model_state_dict, optimizer_state_dict (Adam's m, v, step, learning rate), iter, infos,
        and the state of the normalisers that exist.  With `env_state` two more keys make the file an exact resume point: ``env_state_dict``
        (Go2Env.state_dict()) and ``runner_state_dict`` (runner_state_dict()).  One rank only: each rank of a group owns its shard of the envs."""
        if env_state and self.group is not None:
            raise Go2SimError("save(env_state=True) over a multi-rank group is not implemented: each rank owns its shard of the envs "
                              "(per-rank env-state sidecar files are a follow-up)")
        if self.rank != 0:                                                     # the ranks hold the same bits: rank 0 writes them
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        opt = self.alg.optimizer_state_dict()
        opt["policy_noise_step"] = int(self.policy.noise_step)
        norm_state = lambda normalizer: None if normalizer is None else normalizer.state_dict()
        save_checkpoint(path, self.policy.state_dict(), opt, self.current_learning_iteration, infos, obs_norm_state_dict=norm_state(self.obs_normalizer),
                        critic_obs_norm_state_dict=norm_state(self.critic_obs_normalizer), privileged_obs_norm_state_dict=norm_state(self.privileged_obs_normalizer),
                        rnd_state_dict=norm_state(self.rnd), rnd_optimizer_state_dict=None if self.rnd is None else self.rnd.optimizer_state_dict(),
                        env_state_dict=self.env.state_dict() if env_state else None, runner_state_dict=self.runner_state_dict() if env_state else None)

    def load(self, path, load_optimizer=True):
        """A checkpoint of this runner's own kind resumes the run: model, normalisers, optimizer, the policy's noise step, iteration.  A distillation runner
        also takes a PPO checkpoint, as its teacher (_load_distill); that is no resume and leaves the rest alone."""
        ckpt = read_checkpoint(path)
        if (self._load_distill if self.distill else self._load_ppo)(ckpt, path):
            opt = ckpt.get("optimizer_state_dict") or {}
            if load_optimizer and "exp_avg" in opt:
                self.alg.load_optimizer_state_dict(opt)
                self.policy.noise_step = int(opt.get("policy_noise_step", self.policy.noise_step))
                if self.rnd is not None:
                    self.rnd.load_optimizer_state_dict(ckpt["rnd_optimizer_state_dict"])
            self.current_learning_iteration = int(ckpt.get("iter", 0) or 0)
            ignored = None
            # an exact resume point, taken when it comes from a runner of this kind: the env's state first (it validates before it writes), then the loop's
            if ckpt.get("env_state_dict") is not None and ckpt.get("runner_state_dict") is not None and self.group is None:
                if self.runner_state_matches(ckpt["runner_state_dict"]):
                    self.env.load_state_dict(ckpt["env_state_dict"])
                    self.load_runner_state_dict(ckpt["runner_state_dict"])
                else:
                    ignored = (f"it was saved by a {ckpt['runner_state_dict'].get('kind')!r} runner with {ckpt['runner_state_dict'].get('num_envs')} envs, "
                               f"this one is {self._kind!r} with {self.env.num_envs}")
            elif ckpt.get("env_state_dict") is not None and self.group is not None:
                ignored = "this runner is one rank of a group, and each rank owns its shard of the envs"
            if ignored:
                print(f"OnPolicyRunner.load: {path} carries an env state that is NOT restored ({ignored}); training continues in front of this env as it is, "
                      "curriculum and episode counters included", file=sys.stderr, flush=True)
        return ckpt.get("infos")

    def get_inference_policy(self, device=None):
        """The deterministic policy as a callable.  A recurrent policy keeps its memory between calls: the caller resets it through
        ``runner.policy.reset(dones)`` after every env step, as the collection loop does.  With empirical normalisation the callable first applies the actor
        normaliser without moving its statistics (rsl_rl puts it in eval mode here); the raw observations are not written."""
        if self.obs_normalizer is None:
            return self.policy.act_inference
        normalizer, act = self.obs_normalizer, self.policy.act_inference
        return lambda observations: act(norm_step(normalizer, observations, update=False)[0])
