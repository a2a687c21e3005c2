"""PPO -- host-side mirror of ``rsl_rl.algorithms.PPO`` (rsl-rl-lib==2.2.4) on top of the update entry points of the C ABI
(include/go2sim_train.h): the fused MLP backward, the clipped losses, the adaptive learning rate, the gradient clip and Adam run as HIP
kernels on the arrays ``ActorCritic.act`` reads; nothing of an update goes through the host.

    policy = ActorCritic(49, 104, 16)
    alg = PPO(policy, num_learning_epochs=5, num_mini_batches=4, schedule="adaptive", entropy_coef=0.003, gamma=0.99)
    alg.init_storage(env.num_envs, 24, [49], [104], [16])
    for t in range(24):
        actions = alg.act(obs, critic_obs)
        obs, rew, dones, infos = env.step(actions)
        critic_obs = infos["observations"]["critic"]
        alg.process_env_step(rew, dones, infos)
    alg.compute_returns(critic_obs)
    value_loss, surrogate_loss, entropy = alg.update()      # one host synchronisation, after the last mini-batch

Under ``torchrun`` (``PPO(..., group=torch.distributed.group.WORLD)``) every rank holds a shard of the envs and all of them train ONE policy: per
mini-batch each rank writes its shard's contribution as a float64 record (go2sim_ppo_shard_grad), the records are all-gathered
(distributed.allgather_records) and every rank adds them in rank order (go2sim_ppo_shard_reduce) before the usual go2sim_ppo_apply, so the ranks'
parameters stay bit-identical without ever being re-broadcast.

Left-right symmetry (rsl_rl's ``symmetry_cfg``): ``PPO(..., symmetry_cfg={"use_data_augmentation": True, "use_mirror_loss": True,
"mirror_loss_coeff": 0.5, "mirror_tables": env.mirror_tables()})``.  The mirror is three signed permutations given as tables (Go2Env.mirror_tables);
the kernels read every mini-batch row a second time through them, no mirrored copy is made (include/go2sim_train.h).

A recurrent policy (policy.ActorCriticRecurrent, include/go2sim_rnn.h): ``act`` saves the memories' state at the rollout's first step, ``process_env_step``
zeroes the state of the done envs, and ``update`` runs rsl_rl's recurrent mini-batches -- env blocks with all their steps, no permutation -- through the
cell kernel forwards and backwards in time.  It needs ``num_envs`` divisible by ``num_mini_batches`` and refuses ``symmetry_cfg`` and a multi-rank group.

Random network distillation (rsl_rl's ``rnd_cfg``; rnd.py, include/go2sim_rnd.h): ``PPO(..., rnd_cfg={"num_states": 49, "weight": 0.1 * env.dt, ...})`` builds a
``RandomNetworkDistillation``; ``process_env_step(rewards, dones, infos, rnd_state)`` adds the curiosity bonus to the reward the storage takes (the env's tensor is
not written) and keeps the state rows, and ``update`` trains the predictor on the policy's own mini-batch row lists and returns ``rnd_loss`` as a fourth value.
One rank only.
"""
import ctypes

import torch

from .capi import C, Go2SimError, PpoBatch, PpoCfg, PpoMirror, PpoRnnState, _ptr, load_hip_lib
from .distributed import allgather_records, broadcast_from_rank0, is_multi, shard_seed
from .module_core import memory_keys, mlp_keys, unflatten_keys
from .rnd import RandomNetworkDistillation, check_rnd_cfg
from .rollout import RolloutStorage
from .trainer import OptimizerState, TrainerHandle

VECS = ("PARAMS", "GRADS", "ADAM_M", "ADAM_V")


def make_batch(**tensors):
    """go2sim_ppo_batch_t of contiguous float32 device tensors (kept alive by the caller)."""
    b = PpoBatch()
    for name in PpoBatch.FIELDS:
        t = tensors[name]
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise Go2SimError(f"{name} must be a contiguous float32 tensor")
        setattr(b, name, t.data_ptr())
    return b


class PpoHandle(TrainerHandle):
    """One go2sim_ppo handle: pointers only.  `actor` / `critic` are policy.Mlp objects of the product library."""

    def __init__(self, lib, actor, critic, n_actions, max_rows, *, clip_param=0.2, desired_kl=0.01, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
                 value_loss_coef=1.0, use_clipped_value_loss=True, adaptive=False, betas=(0.9, 0.999), eps=1e-8, lr_min=1e-5, lr_max=1e-2, device=None,
                 memories=None, n_steps=None):
        """memories = (policy.Lstm of the actor, of the critic) and n_steps: the recurrent handle (include/go2sim_rnn.h), max_rows = n_steps x envs of a mini-batch"""
        TrainerHandle.__init__(self, lib, "ppo", device)
        self.actor, self.critic, self.memories = actor, critic, memories
        cfg = PpoCfg(clip_param, desired_kl, entropy_coef, learning_rate, max_grad_norm, value_loss_coef, betas[0], betas[1], eps, lr_min, lr_max,
                     int(bool(use_clipped_value_loss)), int(bool(adaptive)))
        h = ctypes.c_void_p()
        if memories is None:
            lib.check(lib.fn("ppo_create")(actor.h, critic.h, ctypes.c_int(n_actions), ctypes.byref(cfg), ctypes.c_int(max_rows), ctypes.byref(h)), "ppo_create")
        else:
            if not n_steps or max_rows % int(n_steps):
                raise Go2SimError("a recurrent handle is sized as n_steps x envs per mini-batch rows")
            lib.check(lib.fn("ppo_create_recurrent")(actor.h, critic.h, memories[0].h, memories[1].h, ctypes.c_int(n_actions), ctypes.byref(cfg), ctypes.c_int(int(n_steps)),
                                                     ctypes.c_int(max_rows // int(n_steps)), ctypes.byref(h)), "ppo_create_recurrent")
        self._created(h)
        n = ctypes.c_size_t()
        lib.check(lib.fn("ppo_shard_len")(self.h, ctypes.byref(n)), "ppo_shard_len")
        self.shard_len = n.value
        self._sym = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.mirror = None

    def minibatch_grad(self, batch, std, idx, n_rows=None):
        n = idx.numel() if n_rows is None else n_rows
        self._call("minibatch_grad", ctypes.byref(batch), _ptr(std), _ptr(idx), ctypes.c_int(n))

    def shard_grad(self, batch, std, idx, n_rows_global, record=None, n_rows=None):
        """This shard's contribution to a mini-batch of n_rows_global rows: a float64 device record of shard_len entries (include/go2sim_train.h)"""
        n = idx.numel() if n_rows is None else n_rows
        if record is None:
            record = torch.empty(self.shard_len, dtype=torch.float64, device=self.device)
        elif record.dtype != torch.float64 or record.numel() != self.shard_len or not record.is_contiguous():
            raise Go2SimError(f"a record is a contiguous float64 tensor of {self.shard_len} entries")
        self._call("shard_grad", ctypes.byref(batch), _ptr(std), _ptr(idx), ctypes.c_int(n), ctypes.c_longlong(int(n_rows_global)), _ptr(record))
        return record

    def shard_reduce(self, records, std):
        """records [n][shard_len] float64 on the device, added in the order given: gradients, learning-rate rule and running sums of the whole mini-batch"""
        if records.dtype != torch.float64 or not records.is_contiguous() or records.numel() % self.shard_len or not records.is_cuda:
            raise Go2SimError(f"records must be a contiguous float64 device tensor [n][{self.shard_len}]")
        self._call("shard_reduce", _ptr(records), ctypes.c_int(records.numel() // self.shard_len), _ptr(std))

    def set_mirror(self, tables, use_data_augmentation=False, use_mirror_loss=False, mirror_loss_coeff=0.0):
        """tables: {"policy": (src, sign), "critic": (src, sign), "actions": (src, sign)}, each a signed permutation (M x)[j] = sign[j] x[src[j]], or None
        to return to the plain update.  Waits for the device (the library validates the tables on the host); shard_len changes with it."""
        if tables is None:
            self._call("set_mirror", ctypes.c_void_p(0))
            self.mirror = None
        else:
            m, keep = PpoMirror(), []
            for key, name in (("policy", "obs"), ("critic", "critic"), ("actions", "action")):
                if key not in tables:
                    raise Go2SimError(f"mirror_tables needs the entries 'policy', 'critic' and 'actions'; {key!r} is missing")
                src, sign = tables[key]
                src = torch.as_tensor(src).to(device=self.device, dtype=torch.int32).contiguous()
                sign = torch.as_tensor(sign).to(device=self.device, dtype=torch.float32).contiguous()
                width = {"policy": self.actor.dims[0], "critic": self.critic.dims[0], "actions": self.actor.dims[-1]}[key]
                if src.numel() != width or sign.numel() != width:
                    raise Go2SimError(f"mirror table {key!r} has {src.numel()} / {sign.numel()} entries, the network's width is {width}")
                setattr(m, name + "_src", src.data_ptr()); setattr(m, name + "_sign", sign.data_ptr())
                keep += [src, sign]
            m.use_data_augmentation, m.use_mirror_loss, m.mirror_loss_coeff = int(bool(use_data_augmentation)), int(bool(use_mirror_loss)), float(mirror_loss_coeff)
            self._call("set_mirror", ctypes.byref(m))      # the library has its own copy on return
            self.mirror = dict(use_data_augmentation=bool(use_data_augmentation), use_mirror_loss=bool(use_mirror_loss), mirror_loss_coeff=float(mirror_loss_coeff))
        n = ctypes.c_size_t()
        self.L.check(self.L.fn("ppo_shard_len")(self.h, ctypes.byref(n)), "ppo_shard_len")
        self.shard_len = n.value

    def symmetry_loss(self):
        """float64 device tensor [1]: mean of the mirror loss L_sym over the mini-batches since the last reset; no synchronisation"""
        self._call("symmetry_loss", _ptr(self._sym))
        return self._sym

    def apply(self, std):
        self._call("apply", _ptr(std))

    def update(self, batch, std, perm, n_rows_total, n_epochs, n_mini_batches):
        self._call("update", ctypes.byref(batch), _ptr(std), _ptr(perm), ctypes.c_int(n_rows_total), ctypes.c_int(n_epochs), ctypes.c_int(n_mini_batches))

    def rnn_minibatch_grad(self, batch, state, std, n_envs, env0, n_block):
        """forward, head and backward through time of the env block [env0, env0 + n_block) of a rollout of n_steps x n_envs rows (recurrent handle)"""
        self._call("rnn_minibatch_grad", ctypes.byref(batch), ctypes.byref(state), _ptr(std), ctypes.c_int(n_envs), ctypes.c_int(env0), ctypes.c_int(n_block))

    def rnn_update(self, batch, state, std, n_envs, n_epochs, n_mini_batches):
        self._call("rnn_update", ctypes.byref(batch), ctypes.byref(state), _ptr(std), ctypes.c_int(n_envs), ctypes.c_int(n_epochs), ctypes.c_int(n_mini_batches))

    def export(self, which, std=None):
        """flat float32 device vector in state-dict order: actor W0, b0, ..., critic W0, b0, ..., (memory_a, memory_c: weight_ih, weight_hh, bias_ih, bias_hh,) std"""
        return TrainerHandle.export(self, which, std)

    def import_(self, which, flat, std=None):
        TrainerHandle.import_(self, which, flat, std)

    def stats(self):
        """float64 device tensor [value loss, surrogate loss, entropy, kl_mean, learning rate, grad norm, step, mini-batches]; no synchronisation"""
        return TrainerHandle.stats(self)


def make_rnn_state(h_a, c_a, h_c, c_c, dones):
    """go2sim_ppo_rnn_state_t of contiguous device tensors (kept alive by the caller): four float32 [B][H] arrays and the uint8 dones [T][B]"""
    s = PpoRnnState()
    for name, t in zip(PpoRnnState.FIELDS, (h_a, c_a, h_c, c_c, dones)):
        if t.dtype != (torch.uint8 if name == "dones" else torch.float32) or not t.is_contiguous():
            raise Go2SimError(f"{name} must be a contiguous {'uint8' if name == 'dones' else 'float32'} tensor")
        setattr(s, name, t.data_ptr())
    return s


def state_dict_keys(adims, cdims, mdims=None):
    """[(key, shape)] in the flat order of go2sim_ppo_export; mdims = ((n_in, H) of memory_a, of memory_c) for a recurrent policy"""
    keys = mlp_keys("actor", adims) + mlp_keys("critic", cdims)
    if mdims is not None:
        keys += memory_keys("memory_a", *mdims[0]) + memory_keys("memory_c", *mdims[1])
    keys.append(("std", (adims[-1],)))
    return keys


def unflatten(flat, adims, cdims, mdims=None):
    return unflatten_keys(flat, state_dict_keys(adims, cdims, mdims))


def flatten(sd, adims, cdims, mdims=None):
    return torch.cat([sd[k].detach().reshape(-1).to(torch.float32).cpu() for k, _ in state_dict_keys(adims, cdims, mdims)])


class PPO(OptimizerState):
    result_names = ("value_loss", "surrogate_loss", "entropy")                # of what update() returns, as the runner logs them

    def __init__(self, policy, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95, value_loss_coef=1.0, entropy_coef=0.0,
                 learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device=None, *, seed=1, group=None, symmetry_cfg=None,
                 rnd_cfg=None, **kwargs):
        if schedule not in ("adaptive", "fixed"):
            raise Go2SimError(f"schedule must be 'adaptive' or 'fixed', got {schedule!r}")
        unknown = {k: v for k, v in kwargs.items() if k not in ("class_name", "normalize_advantage_per_mini_batch") and v is not None}
        if unknown or kwargs.get("normalize_advantage_per_mini_batch"):
            raise Go2SimError(f"go2sim's PPO does not implement {sorted(unknown) or ['normalize_advantage_per_mini_batch']} (beyond rnd_cfg and symmetry_cfg with mirror_tables, RND and symmetry are out of scope)")
        self.symmetry = self._check_symmetry_cfg(symmetry_cfg)
        self.rnd_cfg = check_rnd_cfg(rnd_cfg)                                   # None for None / {}: everything as without it
        if self.rnd_cfg is not None:
            if group is not None and is_multi(group):
                raise Go2SimError("rnd_cfg over a multi-rank group is not implemented (the sharded predictor update is a follow-up)")
            if "num_states" not in self.rnd_cfg:
                raise Go2SimError("rnd_cfg needs 'num_states', the width of the rnd_state rows (the runner fills it from obs_groups['rnd_state'])")
        self.recurrent = bool(getattr(policy, "is_recurrent", False))
        if self.recurrent and self.symmetry is not None:
            raise Go2SimError("symmetry_cfg with a recurrent policy is not implemented (rsl_rl refuses it too)")
        if self.recurrent and group is not None and is_multi(group):
            raise Go2SimError("the sharded (multi-rank) update of a recurrent policy is not implemented")
        self.policy = self.actor_critic = policy
        self.device = policy.device if device is None else torch.device(device)
        self.num_learning_epochs, self.num_mini_batches = int(num_learning_epochs), int(num_mini_batches)
        self.gamma, self.lam = gamma, lam
        self._hyper = dict(clip_param=clip_param, desired_kl=desired_kl, entropy_coef=entropy_coef, learning_rate=learning_rate, max_grad_norm=max_grad_norm,
                           value_loss_coef=value_loss_coef, use_clipped_value_loss=use_clipped_value_loss, adaptive=schedule == "adaptive")
        self.schedule, self.desired_kl = schedule, desired_kl
        self.learning_rate = float(learning_rate)
        # a process group of more than one rank: the envs are sharded over the ranks and the update sums the shards' gradients in rank order
        self.group = group if group is not None and is_multi(group) else None
        self.rank = torch.distributed.get_rank(self.group) if self.group is not None else 0
        self._gen = torch.Generator(device=self.device).manual_seed(shard_seed(seed, self.rank))
        self.storage = self._h = None
        self.last_stats = None
        self.symmetry_loss = None
        self.rnd = None
        if self.rnd_cfg is not None:
            self.rnd = RandomNetworkDistillation(device=self.device, seed=seed, **self.rnd_cfg)
            self.result_names = PPO.result_names + ("rnd_loss",)
            self.rnd_loss = None

    @staticmethod
    def _check_symmetry_cfg(cfg):
        """rsl_rl's symmetry_cfg with the mirror as tables: -> dict(tables, use_data_augmentation, use_mirror_loss, mirror_loss_coeff) or None"""
        if not cfg:
            return None
        known = {"use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff", "data_augmentation_func", "mirror_tables"}
        if set(cfg) - known:
            raise Go2SimError(f"symmetry_cfg: unknown entries {sorted(set(cfg) - known)}")
        if cfg.get("data_augmentation_func") is not None:
            raise Go2SimError("symmetry_cfg['data_augmentation_func']: a Python callable cannot run inside the update's kernels; give the mirror as "
                              "symmetry_cfg['mirror_tables'] = {'policy': (src, sign), 'critic': (src, sign), 'actions': (src, sign)} (Go2Env.mirror_tables())")
        if cfg.get("mirror_tables") is None:
            raise Go2SimError("symmetry_cfg needs 'mirror_tables' (Go2Env.mirror_tables())")
        return dict(tables=cfg["mirror_tables"], use_data_augmentation=bool(cfg.get("use_data_augmentation", False)),
                    use_mirror_loss=bool(cfg.get("use_mirror_loss", False)), mirror_loss_coeff=float(cfg.get("mirror_loss_coeff", 0.0)))

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape, rnd_state_shape=None):
        T, B, dev = int(num_transitions_per_env), int(num_envs), self.device
        self.T, self.B, self.t = T, B, 0
        self.storage = RolloutStorage(T, B, dev)
        z = lambda *s: torch.zeros(T, B, *s, device=dev)
        self.obs, self.critic_obs, self.actions = z(*actor_obs_shape), z(*critic_obs_shape), z(*action_shape)
        self.old_log_prob, self.old_mu, self.old_sigma = z(), z(*action_shape), z(*action_shape)
        self._mbs = T * B // self.num_mini_batches
        if self._mbs < 1:
            raise Go2SimError("fewer rows than mini-batches")
        if self.recurrent:
            # rsl_rl's recurrent generator: mini-batch m is the env block [m B / nmb, (m + 1) B / nmb) with all T steps
            if B % self.num_mini_batches:
                raise Go2SimError(f"a recurrent policy needs num_envs ({B}) divisible by num_mini_batches ({self.num_mini_batches})")
            self._h = self.policy.attach_trainer(T, B // self.num_mini_batches, **self._hyper)
            self._saved = [torch.zeros(B, self.policy.rnn_hidden_size, device=dev) for _ in range(4)]      # h_a, c_a, h_c, c_c at the rollout's first act
            self._rnn_state = make_rnn_state(*self._saved, self.storage.dones)
        else:
            self._h = self.policy.attach_trainer(self._mbs, **self._hyper)
        if self.symmetry is not None:                                   # before the record below is sized: a record grows by the mirror-loss sum
            self._h.set_mirror(**self.symmetry)
        self._batch = make_batch(obs=self.obs, critic_obs=self.critic_obs, actions=self.actions, target_values=self.storage.values, returns=self.storage.returns,
                                 advantages=self.storage.advantages, old_log_prob=self.old_log_prob, old_mu=self.old_mu, old_sigma=self.old_sigma)
        if self.rnd is not None:
            if rnd_state_shape is not None and list(rnd_state_shape) != [self.rnd.num_states]:
                raise Go2SimError(f"rnd_state_shape {list(rnd_state_shape)} is not rnd_cfg's num_states [{self.rnd.num_states}]")
            self.rnd_states = z(self.rnd.num_states)                      # the rows the predictor's update reads, as the step's networks saw them
            self.rnd.attach(max(B, self._mbs))
            if self.recurrent:                                            # the env blocks with all their steps, t-major: mini-batch m is entries [m mbs, (m + 1) mbs)
                blk = B // self.num_mini_batches
                rows = torch.arange(T, device=dev).view(1, T, 1) * B + torch.arange(B, device=dev).view(self.num_mini_batches, 1, blk)
                self._rnd_idx = rows.reshape(-1).to(torch.int32).contiguous()
        if self.group is not None:
            # the ranks' mini-batch sizes, gathered once: a row weighs 1 / (their sum), so unequal shards are weighted by rows
            sizes = allgather_records(torch.tensor([float(self._mbs)], dtype=torch.float64, device=dev), self.group)
            self._mbs_global = int(sizes.sum().item())
            self._record = torch.empty(self._h.shard_len, dtype=torch.float64, device=dev)
            self.broadcast_parameters()

    def broadcast_parameters(self):
        """Every rank takes rank 0's parameters (network weights and std): the ranks start from the same bits, and keep them because they apply the
        same gradients.  Nothing to do for a single process."""
        if self.group is None:
            return
        flat = broadcast_from_rank0(self._h.export("PARAMS", self.policy.std), self.group)
        self._h.import_("PARAMS", flat, self.policy.std)

    def act(self, obs, critic_obs):
        t = self.t
        if self.recurrent and t == 0:                                      # the state the update's walk through time starts from
            self.policy.save_memory_state(*self._saved)
        actions = self.policy.act(obs, critic_obs)
        self.obs[t].copy_(obs); self.critic_obs[t].copy_(critic_obs); self.actions[t].copy_(actions)
        self.old_log_prob[t].copy_(self.policy.actions_log_prob); self.old_mu[t].copy_(self.policy.action_mean); self.old_sigma[t].copy_(self.policy.action_std)
        return actions

    def process_env_step(self, rewards, dones, infos, rnd_state=None):
        if self.rnd is not None:
            if rnd_state is None:
                raise Go2SimError("process_env_step: a PPO with rnd_cfg needs the rnd_state rows of this step")
            self.intrinsic_rewards, rewards = self.rnd.get_intrinsic_reward(rnd_state, rewards)      # the env's reward tensor is not written
            self.rnd_states[self.t].copy_(self.rnd.last_state)
        self.storage.add_transitions(self.t, rewards, dones, self.policy.values, infos.get("time_outs") if infos else None, gamma=self.gamma)
        self.t += 1
        if self.recurrent:
            self.policy.reset(dones)

    def compute_returns(self, last_critic_obs):
        self.storage.compute_returns(self.policy.evaluate(last_critic_obs), self.gamma, self.lam, group=self.group)

    def update(self):
        n = self.num_mini_batches * self._mbs
        perm = None if self.recurrent else torch.randperm(n, device=self.device, generator=self._gen).to(torch.int32)
        if self.recurrent:
            self._h.rnn_update(self._batch, self._rnn_state, self.policy.std, self.B, self.num_learning_epochs, self.num_mini_batches)
        elif self.group is None:
            self._h.update(self._batch, self.policy.std, perm, self.T * self.B, self.num_learning_epochs, self.num_mini_batches)
        else:
            self._update_sharded(perm)
        extra = []
        if self.rnd is not None:                                           # the predictor's loop on the same row lists, after the policy's
            idx, n_rnd = (self._rnd_idx, self.T * self.B) if self.recurrent else (perm, n)
            extra.append(self.rnd.update(self.rnd_states, idx, n_rnd, self.num_learning_epochs, self.num_mini_batches)[:1])
        if self.symmetry is not None:
            extra.append(self._h.symmetry_loss())
        s = (torch.cat([self._h.stats(), *extra]) if extra else self._h.stats()).cpu()      # the update's only host synchronisation; the extras ride along
        if self.symmetry is not None:
            self.symmetry_loss = float(s[-1])
        if self.rnd is not None:
            self.rnd_loss = float(s[C["GO2SIM_PPO_N_STATS"]])
        s = s[:C["GO2SIM_PPO_N_STATS"]]
        self.last_stats = s
        self.learning_rate = float(s[C["GO2SIM_PPO_ST_LR"]])
        self.t = 0
        out = float(s[C["GO2SIM_PPO_ST_VALUE_LOSS"]]), float(s[C["GO2SIM_PPO_ST_SURROGATE"]]), float(s[C["GO2SIM_PPO_ST_ENTROPY"]])
        return out + (self.rnd_loss,) if self.rnd is not None else out

    def _update_sharded(self, perm):
        """go2sim_ppo_update's loop on the host with the collective in it: per mini-batch this shard's record, one all-gather, the ordered reduction, Adam."""
        h, std, mbs = self._h, self.policy.std, self._mbs
        h.reset_stats()
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                rec = h.shard_grad(self._batch, std, perm[i * mbs:(i + 1) * mbs], self._mbs_global, self._record)
                h.shard_reduce(allgather_records(rec, self.group), std)
                h.apply(std)

    # ---- optimizer state (runner checkpoints) ----------------------------------------------------------
    def optimizer_state_dict(self):
        return dict(OptimizerState.optimizer_state_dict(self), perm_generator_state=self._gen.get_state().cpu())

    def load_optimizer_state_dict(self, sd):
        OptimizerState.load_optimizer_state_dict(self, sd)
        if sd.get("perm_generator_state") is not None and self.rank == 0:     # the file holds rank 0's stream; the other ranks keep their own
            self._gen.set_state(sd["perm_generator_state"].cpu())
