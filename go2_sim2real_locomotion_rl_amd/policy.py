"""ActorCritic -- host-side mirror of ``rsl_rl.modules.ActorCritic`` (rsl-rl-lib==2.2.4, the version
``examples/locomotion/final/go2_train_walk.py:12-15`` pins) on top of the policy entry points of the C ABI
(include/go2sim_policy.h).  It covers the inference side that ``OnPolicyRunner`` / ``PPO.act`` call once per
environment step -- ``act``, ``evaluate``, ``get_actions_log_prob``, ``act_inference``, ``action_mean``,
``action_std`` -- with the reference's argument meaning.  The PPO update runs either in the library (ppo.PPO, include/go2sim_train.h: the
optimizer writes the arrays ``act`` reads, :meth:`state_dict` exports them from the device) or with the caller in torch, who pushes new
parameters with :meth:`load_state_dict`.

    policy = ActorCritic(49, 104, 16, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu")
    policy.load_state_dict(torch.load("model_1000.pt", weights_only=True)["model_state_dict"])
    actions = policy.act(obs, critic_obs)        # one fused MLP kernel per network + one sampling kernel
    values, log_prob = policy.values, policy.actions_log_prob

State-dict keys are those of the reference class: ``actor.{0,2,4,6}.{weight,bias}``, ``critic.{0,2,4,6}.{weight,bias}``, ``std``.
Random numbers come from the library's counter-based Philox stream (seed, row, step), not from torch's global generator.
``activation`` is one of rsl_rl's ``elu``, ``selu``, ``relu``, ``lrelu``, ``tanh``, ``sigmoid``, ``identity`` (include/go2sim_activation.h); as in rsl_rl it is part of the
config, not of the checkpoint.

``ActorCriticRecurrent`` (below) is ``rsl_rl.modules.ActorCriticRecurrent`` with one LSTM layer per network (include/go2sim_rnn.h): the same surface plus
``reset(dones)`` / ``get_hidden_states()``, and the four ``nn.LSTM`` keys of ``memory_{a,c}.rnn.`` (module_core.lstm_shapes).

What the two classes share with distillation's modules -- the initial draws, the key lists, the memories' state, the device set-up and the create-or-set of a
network -- is module_core.py; this file keeps the handles (``Mlp``, ``Lstm``), the launches and what is particular to the two classes.
"""
import ctypes

import numpy as np
import torch

from .capi import ACTIVATIONS, Go2SimError, Handle, _ptr
from .module_core import (LSTM_KEYS, MemoryState, PolicyModule, actor_critic_init, actor_critic_recurrent_init, check_lstm_config, hidden_state_views,  # noqa: F401
                          lstm_shapes)
from .ppo import PpoHandle, unflatten


def resolve_activation(name):
    """train_cfg["policy"]["activation"] -> one of the seven names of include/go2sim_activation.h (rsl_rl's resolve_nn_activation, each meaning the same torch
    module).  Touches no device: a refusal is a Go2SimError before anything is allocated."""
    key = str(name).lower()
    if key == "crelu":
        raise Go2SimError("activation 'crelu' is not implemented: it doubles the layer's width and is not a function of one value; "
                          f"go2sim implements {sorted(ACTIVATIONS)}")
    if key not in ACTIVATIONS:
        raise Go2SimError(f"unknown activation {name!r}: go2sim implements {sorted(ACTIVATIONS)}")
    return key


class Mlp(Handle):
    """One go2sim_mlp handle (works with either library: product or CPU oracle; the oracle's is ELU only)."""

    def __init__(self, lib, dims, params, device=0, activation="elu"):
        Handle.__init__(self, lib, "mlp_destroy")
        self.L, self.dims = lib, [int(d) for d in dims]
        activation = resolve_activation(activation)
        if activation != "elu" and not lib.is_device:                              # before the handle exists: nothing to release on the refusal
            raise Go2SimError("the CPU oracle's MLP is ELU only (include/go2sim_activation.h has no CPU twin)")
        params = np.ascontiguousarray(params, dtype=np.float32)
        self.n_params = params.size
        h = ctypes.c_void_p()
        d = (ctypes.c_int * len(self.dims))(*self.dims)
        rc = lib.fn("mlp_create")(ctypes.c_int(device), d, ctypes.c_int(len(self.dims) - 1), params.ctypes.data_as(ctypes.c_void_p),
                                  ctypes.c_size_t(params.size), ctypes.byref(h))
        lib.check(rc, "mlp_create")
        self.h = h
        self.activation = "elu"
        if activation != "elu":
            self.set_activation(activation)

    def set_activation(self, name):
        """go2sim_act_set (include/go2sim_activation.h): to be called before the handle's first launch.  Product library only."""
        name = resolve_activation(name)
        if not self.L.is_device:
            raise Go2SimError("the CPU oracle's MLP is ELU only (include/go2sim_activation.h has no CPU twin)")
        self.L.check(self.L.lib.go2sim_act_set(self.h, ctypes.c_int(ACTIVATIONS[name])), "act_set")
        self.activation = name

    def get_activation(self):
        """the name behind go2sim_act_get"""
        out = ctypes.c_int(-1)
        self.L.check(self.L.lib.go2sim_act_get(self.h, ctypes.byref(out)), "act_get")
        return {v: k for k, v in ACTIVATIONS.items()}[out.value]

    def set_params(self, params, stream=0):
        params = np.ascontiguousarray(params, dtype=np.float32)
        self.L.check(self.L.fn("mlp_set_params")(self.h, params.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(params.size), ctypes.c_void_p(stream)),
                     "mlp_set_params")

    def forward(self, x, y, n_rows, stream=0):
        self.L.check(self.L.fn("mlp_forward")(self.h, _ptr(x), _ptr(y), ctypes.c_int(n_rows), ctypes.c_void_p(stream)), "mlp_forward")

def flatten_sequential(state_dict, prefix, n_layers):
    """[W0, b0, W1, b1, ...] of ``prefix.{0,2,4,...}`` as one float32 vector (the layout go2sim_mlp_create takes) + the layer sizes."""
    chunks, dims = [], []
    for l in range(n_layers):
        w = np.asarray(state_dict[f"{prefix}.{2 * l}.weight"].detach().cpu().numpy() if isinstance(state_dict[f"{prefix}.{2 * l}.weight"], torch.Tensor)
                       else state_dict[f"{prefix}.{2 * l}.weight"], dtype=np.float32)
        b = state_dict[f"{prefix}.{2 * l}.bias"]
        b = np.asarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float32)
        if l == 0:
            dims.append(w.shape[1])
        dims.append(w.shape[0])
        chunks += [w.reshape(-1), b.reshape(-1)]
    return np.concatenate(chunks), dims


def policy_act(lib, actor, critic, obs, critic_obs, std, n_rows, seed, step, deterministic, actions, mean, values, log_prob, stream=0):
    rc = lib.fn("policy_act")(actor.h, critic.h if critic is not None else ctypes.c_void_p(0), _ptr(obs), _ptr(critic_obs), _ptr(std),
                              ctypes.c_int(n_rows), ctypes.c_uint64(seed), ctypes.c_uint32(step), ctypes.c_int(int(deterministic)),
                              _ptr(actions), _ptr(mean), _ptr(values), _ptr(log_prob), ctypes.c_void_p(stream))
    lib.check(rc, "policy_act")


class ActorCritic(PolicyModule):
    _mdims = None                                                              # the memories' ((n_in, H), (n_in, H)): the recurrent subclass's

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(512, 256, 128), critic_hidden_dims=(512, 256, 128),
                 activation="elu", init_noise_std=1.0, *, device=None, seed=1, **kwargs):
        self.activation = resolve_activation(activation)                          # before anything touches the device: a refusal needs no GPU
        PolicyModule.__init__(self, num_actions, device, seed)
        self._adims = [num_actor_obs, *actor_hidden_dims, num_actions]
        self._cdims = [num_critic_obs, *critic_hidden_dims, 1]
        self.load_state_dict(self._initial_state(init_noise_std, seed))

    # ---- parameters ------------------------------------------------------------------------------
    def _initial_state(self, init_noise_std, seed):
        return actor_critic_init(self._adims, self._cdims, init_noise_std, seed)

    def _parts(self):
        return [("_actor", "mlp", "actor", self._adims), ("_critic", "mlp", "critic", self._cdims)]

    def load_state_dict(self, state_dict, strict=True):
        self._set_parts(self._parts(), state_dict)
        self._set_std(state_dict)
        return True

    def state_dict(self):
        """The parameters as they are on the device: once a trainer is attached the optimizer has written them there, and the host copy of the last
        load_state_dict is stale."""
        if self._trainer is None:
            return self._host_state()
        return unflatten(self._trainer.export("PARAMS", self.std).cpu(), self._adims, self._cdims, self._mdims)

    def attach_trainer(self, max_rows_per_minibatch, **hyper):
        """The go2sim_ppo handle (ppo.PpoHandle) that updates this policy's device parameters in place; the optimizer state lives in it."""
        self._trainer = PpoHandle(self._L, self._actor, self._critic, self.num_actions, max_rows_per_minibatch, device=self.device, **hyper)
        return self._trainer

    def load_checkpoint(self, path, strict=False):
        """Load ``model_<it>.pt`` of a training run (rsl_rl 2.2.4 ``OnPolicyRunner.save`` layout), read with ``torch.load(weights_only=True)``.
        strict=False is the eval scripts' compatibility load (go2_eval_stairs.py:368-450): layers whose shapes differ from this model -- a critic
        trained with another privileged-observation width -- keep their current values, everything else (the actor in particular) is taken from the
        file.  -> (loaded keys, skipped {key: reason}, iteration)"""
        from .eval_io import compatible_state_dict, read_checkpoint

        ckpt = read_checkpoint(path)
        saved = ckpt["model_state_dict"]
        if strict:
            self.load_state_dict(saved)
            return sorted(saved), {}, int(ckpt.get("iter", 0) or 0)
        merged, loaded, skipped = compatible_state_dict(self.state_dict(), saved)
        self.load_state_dict(merged)
        return loaded, skipped, int(ckpt.get("iter", 0) or 0)

    # ---- rsl_rl ActorCritic surface (inference side) ---------------------------------------------------
    def _run(self, obs, critic_obs, deterministic):
        B = obs.shape[0]
        obs = obs.to(device=self.device, dtype=torch.float32).contiguous()
        co = None if critic_obs is None else critic_obs.to(device=self.device, dtype=torch.float32).contiguous()
        self._actions, self._mean = self._buf("actions", (B, self.num_actions)), self._buf("mean", (B, self.num_actions))
        self._values = self._buf("values", (B,)) if co is not None else None
        self._logp = self._buf("logp", (B,))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        policy_act(self._L, self._actor, self._critic if co is not None else None, obs, co, self.std, B, self._seed, self._step, deterministic,
                   self._actions, self._mean, self._values, self._logp, stream)
        self._step += 1
        return self._actions

    def act(self, observations, critic_observations=None, **kwargs):
        """ActorCritic.act (+ evaluate when critic observations are given: PPO.act calls both on every step)."""
        return self._run(observations, critic_observations, False)

    def act_inference(self, observations):
        return self._run(observations, None, True)

    def evaluate(self, critic_observations, **kwargs):
        B = critic_observations.shape[0]
        co = critic_observations.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(B, 1, device=self.device)
        self._critic.forward(co, out, B, torch.cuda.current_stream(self.device).cuda_stream)
        return out

    def get_actions_log_prob(self, actions):
        """Normal(mean, std).log_prob(actions).sum(-1) for the distribution of the last act()."""
        if actions.data_ptr() == self._actions.data_ptr():
            return self._logp
        var = self.std * self.std
        return (-((actions - self._mean) ** 2) / (2 * var) - torch.log(self.std) - 0.9189385332046727).sum(-1)

    @property
    def values(self):
        return None if self._values is None else self._values.unsqueeze(-1)

    @property
    def actions_log_prob(self):
        return self._logp


# ---- recurrent policy (include/go2sim_rnn.h) --------------------------------------------------------------------------------------------------
def flatten_lstm(state_dict, prefix):
    """[weight_ih, weight_hh, bias_ih, bias_hh] of ``prefix.rnn.*`` as one float32 vector (the layout go2sim_lstm_create takes) + (n_in, n_hidden)."""
    ts = []
    for k in LSTM_KEYS:
        v = state_dict[f"{prefix}.rnn.{k}"]
        ts.append(np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32))
    if ts[0].ndim != 2 or ts[0].shape[0] % 4 or ts[1].shape != (ts[0].shape[0], ts[0].shape[0] // 4) or ts[2].shape != (ts[0].shape[0],) or ts[3].shape != ts[2].shape:
        raise Go2SimError(f"{prefix}: not the tensors of a one-layer nn.LSTM: {[t.shape for t in ts]}")
    return np.concatenate([t.reshape(-1) for t in ts]), (ts[0].shape[1], ts[0].shape[0] // 4)


class Lstm(Handle):
    """One go2sim_lstm handle of the product library."""

    def __init__(self, lib, n_in, n_hidden, params, device=0):
        Handle.__init__(self, lib, "lstm_destroy")
        self.L, self.n_in, self.n_hidden = lib, int(n_in), int(n_hidden)
        params = np.ascontiguousarray(params, dtype=np.float32)
        self.n_params = params.size
        h = ctypes.c_void_p()
        lib.check(lib.fn("lstm_create")(ctypes.c_int(device), ctypes.c_int(n_in), ctypes.c_int(n_hidden), params.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.c_size_t(params.size), ctypes.byref(h)), "lstm_create")
        self.h = h

    def set_params(self, params, stream=0):
        params = np.ascontiguousarray(params, dtype=np.float32)
        self.L.check(self.L.fn("lstm_set_params")(self.h, params.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(params.size), ctypes.c_void_p(stream)),
                     "lstm_set_params")

    def get_params(self, stream=0):
        out = np.empty(self.n_params, np.float32)
        self.L.check(self.L.fn("lstm_get_params")(self.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(out.size), ctypes.c_void_p(stream)), "lstm_get_params")
        return out

def lstm_step(lib, mem_a, x_a, h_in_a, c_in_a, h_out_a, c_out_a, mem_c=None, x_c=None, h_in_c=None, c_in_c=None, h_out_c=None, c_out_c=None, reset=None, n_rows=None,
              stream=0):
    """go2sim_lstm_step: one cell step of one or two memories in one launch (h_out must not be h_in)"""
    n = x_a.shape[0] if n_rows is None else n_rows
    rc = lib.fn("lstm_step")(mem_a.h, _ptr(x_a), _ptr(h_in_a), _ptr(c_in_a), _ptr(h_out_a), _ptr(c_out_a), mem_c.h if mem_c is not None else ctypes.c_void_p(0),
                             _ptr(x_c), _ptr(h_in_c), _ptr(c_in_c), _ptr(h_out_c), _ptr(c_out_c), _ptr(reset), ctypes.c_int(n), ctypes.c_void_p(stream))
    lib.check(rc, "lstm_step")


class ActorCriticRecurrent(ActorCritic):
    """``rsl_rl.modules.ActorCriticRecurrent`` (rsl-rl-lib==2.2.4) with ``rnn_type="lstm"`` and one layer: ``memory_a = LSTM(num_actor_obs -> H)`` in front of
    the actor MLP, ``memory_c = LSTM(num_critic_obs -> H)`` in front of the critic MLP (include/go2sim_rnn.h).  ``act`` steps memory_a (and, given critic
    observations, memory_c), ``evaluate`` steps memory_c, ``reset(dones)`` zeroes the state of the done envs at once.  State-dict keys beside the parent's:
    the four ``nn.LSTM`` keys under ``memory_{a,c}.rnn.``."""
    is_recurrent = True

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256), critic_hidden_dims=(256, 256, 256), activation="elu",
                 init_noise_std=1.0, rnn_type="lstm", rnn_hidden_size=256, rnn_num_layers=1, *, device=None, seed=1, **kwargs):
        H = self.rnn_hidden_size = check_lstm_config("ActorCriticRecurrent", rnn_type, rnn_num_layers, rnn_hidden_size, "rnn_hidden_size")
        self._mdims = ((int(num_actor_obs), H), (int(num_critic_obs), H))
        super().__init__(H, H, num_actions, actor_hidden_dims, critic_hidden_dims, activation, init_noise_std, device=device, seed=seed, **kwargs)
        self._hid = (MemoryState(H, self.device), MemoryState(H, self.device))      # memory_a's, memory_c's

    # ---- parameters ------------------------------------------------------------------------------
    def _initial_state(self, init_noise_std, seed):
        return actor_critic_recurrent_init(self._adims, self._cdims, self._mdims, init_noise_std, seed)

    def _parts(self):
        return super()._parts() + [("_mem_a", "lstm", "memory_a", self._mdims[0]), ("_mem_c", "lstm", "memory_c", self._mdims[1])]

    def attach_trainer(self, n_steps, max_envs_per_minibatch, **hyper):
        """The recurrent go2sim_ppo handle: workspaces for n_steps x max_envs_per_minibatch rows, the memories' parameters in the optimizer's vectors."""
        self._trainer = PpoHandle(self._L, self._actor, self._critic, self.num_actions, int(n_steps) * int(max_envs_per_minibatch), device=self.device,
                                  memories=(self._mem_a, self._mem_c), n_steps=int(n_steps), **hyper)
        return self._trainer

    # ---- the memories' state ---------------------------------------------------------------------------
    def _step_memories(self, obs, critic_obs):
        """One launch for the memories whose observations are given; -> (h_a or None, h_c or None)"""
        B = (obs if obs is not None else critic_obs).shape[0]
        args, outs = [], []
        for state, mem, x in ((self._hid[0].rows(B), self._mem_a, obs), (self._hid[1].rows(B), self._mem_c, critic_obs)):
            if x is None:
                outs.append(None)
                continue
            step = state.advance()
            args += [mem, x.to(device=self.device, dtype=torch.float32).contiguous(), *step]
            outs.append(step[2])
        lstm_step(self._L, *args, n_rows=B, stream=torch.cuda.current_stream(self.device).cuda_stream)
        return outs

    def _run(self, obs, critic_obs, deterministic):
        h_a, h_c = self._step_memories(obs, critic_obs)
        return super()._run(h_a, h_c, deterministic)

    def evaluate(self, critic_observations, **kwargs):
        _, h_c = self._step_memories(None, critic_observations)
        return super().evaluate(h_c)

    def save_memory_state(self, h_a, c_a, h_c, c_c):
        """The memories' state as the next step enters it, copied into the caller's [B][H] arrays: what PPO keeps of a rollout's first act."""
        B = h_a.shape[0]
        self._hid[0].rows(B).copy_entering(h_a, c_a); self._hid[1].rows(B).copy_entering(h_c, c_c)

    def reset(self, dones=None, hidden_states=None):
        """Zero h and c of the done envs (all envs without `dones`), now."""
        for state in self._hid:
            state.zero(dones)

    def get_hidden_states(self):
        """((h_a, c_a), (h_c, c_c)), each [1][B][H] as nn.LSTM shapes them; views of the live state (None, None before the first step)"""
        return hidden_state_views(self._hid)
