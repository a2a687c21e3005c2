"""Teacher-student distillation -- host-side mirror of ``rsl_rl.algorithms.Distillation`` and ``rsl_rl.modules.StudentTeacher`` (rsl_rl 2.3 on) on the
entry points of include/go2sim_distill.h.  A teacher that reads the clean, privileged rows is distilled into a student that reads what the robot can
deliver: the student collects the data and is regressed onto the teacher's action (DAgger style).  Student and teacher run side by side in one launch
per env step; the update (windows of ``gradient_length`` steps, behaviour loss, optional clip, Adam) runs as HIP kernels on the arrays ``act`` reads.

    policy = StudentTeacher(49, 104, 16, student_hidden_dims=[256, 256, 256], teacher_hidden_dims=[512, 256, 128], device=dev, seed=1)
    policy.load_state_dict(read_checkpoint("teacher/model_1000.pt")["model_state_dict"])     # a PPO checkpoint: teacher.* <- actor.*
    alg = Distillation(policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3)
    alg.init_storage(env.num_envs, 24, [49], [104], [16])
    for t in range(24):
        actions = alg.act(obs, teacher_obs)
        obs, rew, dones, infos = env.step(actions)
        alg.process_env_step(rew, dones, infos)
    behavior_loss = alg.update()                                  # one host synchronisation: the read of the statistics

State-dict keys: ``student.{0,2,..}.{weight,bias}``, ``teacher.{0,2,..}.{weight,bias}``, ``std``.  ``std`` gets no gradient and is outside the optimizer.
"""
import ctypes

import torch

from .capi import C, DistillCfg, Go2SimError, _ptr, load_hip_lib
from .distributed import is_multi
from .policy import Mlp, flatten_sequential, policy_act, resolve_activation
from .trainer import OptimizerState, TrainerHandle, mlp_keys, unflatten_keys

LOSS_TYPES = ("mse", "huber")


# ---- pure functions (no GPU) ---------------------------------------------------------------------------------------------------------------------
def distill_windows(T, E, G):
    """The window schedule of one update: -> (windows, tail), lists of (e, t).  The pairs are counted through epochs and steps; a window closes whenever
    the count is a multiple of G, runs across epoch boundaries, may hold a step twice when G > T; the pairs of the last, open window are the dropped tail."""
    T, E, G = int(T), int(E), int(G)
    if T < 1 or E < 1 or G < 1:
        raise Go2SimError(f"distill_windows needs T, E, G >= 1, got {(T, E, G)}")
    windows, cur, cnt = [], [], 0
    for e in range(E):
        for t in range(T):
            cnt += 1
            cur.append((e, t))
            if cnt % G == 0:
                windows.append(cur)
                cur = []
    return windows, cur


def _check_shapes(sd, prefix, dims, what):
    want = mlp_keys(prefix, dims)
    have = sorted(k for k in sd if k.startswith(prefix + "."))
    if have != sorted(k for k, _ in want):
        raise Go2SimError(f"{what}: the keys {have} are not those of a network with layer sizes {list(dims)}")
    for k, shape in want:
        if tuple(sd[k].shape) != tuple(shape):
            raise Go2SimError(f"{what}: {k} has shape {tuple(sd[k].shape)}, this model's is {tuple(shape)}")


def teacher_state_from_checkpoint(state_dict, student_dims=None, teacher_dims=None):
    """What a ``model_state_dict`` means to a StudentTeacher, as rsl_rl reads it: -> (mapped state dict, resume).
      * a dict with ``actor.*`` keys is a PPO checkpoint: ``teacher.* <- actor.*`` and nothing else (critic and std are dropped), resume = False;
      * a dict with ``student.*`` keys is a distillation checkpoint: ``student.*``, ``teacher.*`` and ``std`` are all required, resume = True.
    With the layer sizes given, every mapped tensor's shape is checked and a mismatch refused with both shapes named."""
    keys = list(state_dict)
    if any(k.startswith("memory_") for k in keys):
        raise Go2SimError("the checkpoint is a recurrent policy's (memory_a / memory_c): a recurrent teacher or student (StudentTeacherRecurrent) is not implemented")
    has_actor, has_student = any(k.startswith("actor.") for k in keys), any(k.startswith("student.") for k in keys)
    if has_actor and has_student:
        raise Go2SimError("the state dict has both actor.* and student.* keys: neither a PPO nor a distillation checkpoint")
    if has_actor:
        mapped = {"teacher." + k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
        if teacher_dims is not None:
            _check_shapes(mapped, "teacher", teacher_dims, "teacher from a PPO checkpoint's actor")
        return mapped, False
    if has_student:
        if "std" not in state_dict or not any(k.startswith("teacher.") for k in keys):
            raise Go2SimError("a distillation checkpoint needs student.*, teacher.* and std")
        unknown = [k for k in keys if k != "std" and not k.startswith(("student.", "teacher."))]
        if unknown:
            raise Go2SimError(f"a distillation checkpoint holds student.*, teacher.* and std; unexpected keys {sorted(unknown)}")
        mapped = dict(state_dict)
        if student_dims is not None:
            _check_shapes(mapped, "student", student_dims, "student")
            if tuple(mapped["std"].shape) != (student_dims[-1],):
                raise Go2SimError(f"std has shape {tuple(mapped['std'].shape)}, this model's is {(student_dims[-1],)}")
        if teacher_dims is not None:
            _check_shapes(mapped, "teacher", teacher_dims, "teacher")
        return mapped, True
    raise Go2SimError("the state dict has neither actor.* keys (a PPO checkpoint, the teacher) nor student.* keys (a distillation checkpoint)")


def unflatten_student(flat, dims):
    return unflatten_keys(flat, mlp_keys("student", dims))


# ---- the trainer handle --------------------------------------------------------------------------------------------------------------------------
class DistillHandle(TrainerHandle):
    """One go2sim_distill handle: pointers only.  `student` is a policy.Mlp of the product library."""

    def __init__(self, lib, student, n_actions, max_window_rows, *, learning_rate=1e-3, max_grad_norm=None, loss_type="mse", betas=(0.9, 0.999), eps=1e-8, sub_rows=0,
                 device=None):
        if loss_type not in LOSS_TYPES:
            raise Go2SimError(f"loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
        TrainerHandle.__init__(self, lib, "distill", device)
        self.student = student
        cfg = DistillCfg(float(learning_rate), float(max_grad_norm) if max_grad_norm is not None else 0.0, betas[0], betas[1], eps,
                         C["GO2SIM_DISTILL_" + loss_type.upper()], int(sub_rows))
        h = ctypes.c_void_p()
        lib.check(lib.fn("distill_create")(student.h, ctypes.c_int(n_actions), ctypes.byref(cfg), ctypes.c_int(int(max_window_rows)), ctypes.byref(h)), "distill_create")
        self._created(h)

    def window_grad(self, obs, teacher_actions, idx, n_envs, n_rows=None):
        n = idx.numel() if n_rows is None else n_rows
        self._call("window_grad", _ptr(obs), _ptr(teacher_actions), _ptr(idx), ctypes.c_int(n), ctypes.c_int(n_envs))

    def loss_only(self, obs, teacher_actions, idx, n_envs, n_rows=None):
        n = idx.numel() if n_rows is None else n_rows
        self._call("loss_only", _ptr(obs), _ptr(teacher_actions), _ptr(idx), ctypes.c_int(n), ctypes.c_int(n_envs))

    def apply(self):
        self._call("apply")

    def update(self, obs, teacher_actions, n_steps, n_envs, n_epochs, gradient_length):
        self._call("update", _ptr(obs), _ptr(teacher_actions), ctypes.c_int(n_steps), ctypes.c_int(n_envs), ctypes.c_int(n_epochs), ctypes.c_int(gradient_length))

    def export(self, which):
        """flat float32 device vector in state-dict order: student W0, b0, W1, b1, ..."""
        return TrainerHandle.export(self, which)

    def stats(self):
        """float64 device tensor [mean behaviour loss, learning rate, grad norm, step, pairs, windows]; no synchronisation"""
        return TrainerHandle.stats(self)


def distill_act(lib, student, teacher, obs, teacher_obs, std, n_rows, seed, step, deterministic, actions, mean, teacher_actions, stream=0):
    rc = lib.fn("distill_act")(student.h, teacher.h, _ptr(obs), _ptr(teacher_obs), _ptr(std), ctypes.c_int(n_rows), ctypes.c_uint64(seed), ctypes.c_uint32(step),
                               ctypes.c_int(int(deterministic)), _ptr(actions), _ptr(mean), _ptr(teacher_actions), ctypes.c_void_p(stream))
    lib.check(rc, "distill_act")


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------
class StudentTeacher:
    is_recurrent = False

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256), activation="elu",
                 init_noise_std=0.1, *, device=None, seed=1, **kwargs):
        self.activation = resolve_activation(activation)                          # one name for student and teacher, as in rsl_rl; refused before the device is touched
        unknown = {k: v for k, v in kwargs.items() if k != "class_name" and v is not None}
        if unknown:
            raise Go2SimError(f"StudentTeacher does not implement {sorted(unknown)}")
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_actions = int(num_actions)
        self._L = load_hip_lib()
        self._sdims = [int(num_student_obs), *[int(d) for d in student_hidden_dims], self.num_actions]
        self._tdims = [int(num_teacher_obs), *[int(d) for d in teacher_hidden_dims], self.num_actions]
        g = torch.Generator().manual_seed(int(seed))
        sd = {}
        for prefix, dims in (("student", self._sdims), ("teacher", self._tdims)):      # nn.Linear default init
            for l in range(len(dims) - 1):
                bound = 1.0 / (dims[l] ** 0.5)
                sd[f"{prefix}.{2 * l}.weight"] = (torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * bound
                sd[f"{prefix}.{2 * l}.bias"] = (torch.rand(dims[l + 1], generator=g) * 2 - 1) * bound
        sd["std"] = float(init_noise_std) * torch.ones(self.num_actions)
        self._student = self._teacher = self._trainer = None
        self.std = torch.ones(self.num_actions, device=self.device)
        self._teacher_state = {}
        self._load_all(sd)
        self.loaded_teacher = False
        self._seed, self._step = int(seed), 0
        self._bufs = {}
        self._mean = self._teacher_actions = None

    # ---- parameters ------------------------------------------------------------------------------
    def _set_net(self, which, sd):
        prefix, dims = ("student", self._sdims) if which == "student" else ("teacher", self._tdims)
        flat, d = flatten_sequential(sd, prefix, len(dims) - 1)
        if d != dims:
            raise Go2SimError(f"state dict has {prefix} layer sizes {d}, this model's are {dims}")
        cur = self._student if which == "student" else self._teacher
        if cur is None:
            net = Mlp(self._L, dims, flat, self.device.index or 0, self.activation)
            if which == "student":
                self._student = net
            else:
                self._teacher = net
        else:
            cur.set_params(flat)

    def _load_all(self, sd):
        self._set_net("student", sd)
        self._set_net("teacher", sd)
        self.std.copy_(sd["std"].detach().reshape(self.num_actions))
        self._student_state = {k: sd[k].detach().clone() for k, _ in mlp_keys("student", self._sdims)}
        self._teacher_state = {k: sd[k].detach().clone() for k, _ in mlp_keys("teacher", self._tdims)}

    def load_state_dict(self, state_dict, strict=True):
        """rsl_rl's StudentTeacher.load_state_dict: a PPO checkpoint (``actor.*``) loads the teacher only and returns False (not a resume); a distillation
        checkpoint (``student.*``) loads student, teacher and std strictly and returns True.  ``loaded_teacher`` is set either way."""
        mapped, resume = teacher_state_from_checkpoint(state_dict, self._sdims, self._tdims)
        if resume:
            self._load_all(mapped)
        else:
            self._set_net("teacher", mapped)
            self._teacher_state = {k: mapped[k].detach().clone() for k, _ in mlp_keys("teacher", self._tdims)}
        self.loaded_teacher = True
        return resume

    def state_dict(self):
        """student.* as they are on the device (the optimizer writes them there once a trainer is attached), teacher.* as loaded, std."""
        if self._trainer is None:
            out = dict(self._student_state)
        else:
            out = unflatten_student(self._trainer.export("PARAMS").cpu(), self._sdims)
        out.update({k: v.clone() for k, v in self._teacher_state.items()})
        out["std"] = self.std.detach().cpu().clone()
        return out

    def attach_trainer(self, max_window_rows, **hyper):
        """The go2sim_distill handle that updates the student's device parameters in place; the optimizer state lives in it."""
        self._trainer = DistillHandle(self._L, self._student, self.num_actions, max_window_rows, device=self.device, **hyper)
        return self._trainer

    # ---- rsl_rl StudentTeacher surface -------------------------------------------------------------------
    def _buf(self, name, shape):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(*shape, device=self.device, dtype=torch.float32)
            self._bufs[name] = t
        return t

    def act(self, observations, teacher_observations, deterministic=False):
        """One launch for both networks and the sampling kernel: -> the student's actions; ``action_mean`` and ``teacher_actions`` hold the rest."""
        B = observations.shape[0]
        obs = observations.to(device=self.device, dtype=torch.float32).contiguous()
        tobs = teacher_observations.to(device=self.device, dtype=torch.float32).contiguous()
        if obs.shape[1] != self._sdims[0] or tobs.shape[1] != self._tdims[0] or tobs.shape[0] != B:
            raise Go2SimError(f"act: observations {tuple(obs.shape)} / {tuple(tobs.shape)}, the networks read [{B}][{self._sdims[0]}] / [{B}][{self._tdims[0]}]")
        actions, self._mean = self._buf("actions", (B, self.num_actions)), self._buf("mean", (B, self.num_actions))
        self._teacher_actions = self._buf("teacher_actions", (B, self.num_actions))
        distill_act(self._L, self._student, self._teacher, obs, tobs, self.std, B, self._seed, self._step, deterministic, actions, self._mean, self._teacher_actions,
                    torch.cuda.current_stream(self.device).cuda_stream)
        self._step += 1
        return actions

    def act_inference(self, observations):
        """The deterministic student."""
        B = observations.shape[0]
        obs = observations.to(device=self.device, dtype=torch.float32).contiguous()
        actions, self._mean = self._buf("actions", (B, self.num_actions)), self._buf("mean", (B, self.num_actions))
        policy_act(self._L, self._student, None, obs, None, self.std, B, self._seed, self._step, True, actions, self._mean, None, None,
                   torch.cuda.current_stream(self.device).cuda_stream)
        self._step += 1
        return actions

    def evaluate(self, teacher_observations):
        """The teacher's actions."""
        B = teacher_observations.shape[0]
        tobs = teacher_observations.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(B, self.num_actions, device=self.device)
        self._teacher.forward(tobs, out, B, torch.cuda.current_stream(self.device).cuda_stream)
        return out

    @property
    def action_mean(self):
        return self._mean

    @property
    def action_std(self):
        return self.std.expand_as(self._mean)

    @property
    def teacher_actions(self):
        return self._teacher_actions

    def reset(self, dones=None, hidden_states=None):
        pass


# ---- the algorithm ---------------------------------------------------------------------------------------------------------------------------------
class Distillation(OptimizerState):
    """rsl_rl's Distillation on a StudentTeacher.  The activation is the policy's (``train_cfg["policy"]["activation"]``, one name for student and teacher):
    as in rsl_rl it lives in the config (``cfgs.pkl``), not in ``model_<it>.pt``, so a teacher checkpoint is interpreted with the student config's
    activation -- a teacher trained with another one loads without complaint and computes something else."""

    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse", device=None, *, group=None, **kwargs):
        unknown = {k: v for k, v in kwargs.items() if k != "class_name" and v is not None}
        if unknown:
            raise Go2SimError(f"go2sim's Distillation does not implement {sorted(unknown)}")
        if loss_type not in LOSS_TYPES:
            raise Go2SimError(f"Distillation: loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
        if getattr(policy, "is_recurrent", False) or not isinstance(policy, StudentTeacher):
            raise Go2SimError(f"Distillation needs a StudentTeacher policy, got {type(policy).__name__} (a recurrent class, StudentTeacherRecurrent, is not implemented)")
        if group is not None and is_multi(group):
            raise Go2SimError("Distillation over a multi-rank group is not implemented (the sharded distillation update is a follow-up)")
        if int(num_learning_epochs) < 1 or int(gradient_length) < 1 or not float(learning_rate) > 0.0:
            raise Go2SimError("Distillation needs num_learning_epochs >= 1, gradient_length >= 1 and learning_rate > 0")
        self.policy = policy
        self.device = policy.device if device is None else torch.device(device)
        self.num_learning_epochs, self.gradient_length = int(num_learning_epochs), int(gradient_length)
        self.learning_rate, self.max_grad_norm, self.loss_type = float(learning_rate), max_grad_norm, loss_type
        self._h = None
        self.last_stats = None

    def init_storage(self, num_envs, num_transitions_per_env, student_obs_shape, teacher_obs_shape, action_shape):
        T, B, dev = int(num_transitions_per_env), int(num_envs), self.device
        self.T, self.B, self.t = T, B, 0
        self.obs = torch.zeros(T, B, *student_obs_shape, device=dev)
        self.teacher_actions = torch.zeros(T, B, *action_shape, device=dev)
        self.dones = torch.zeros(T, B, dtype=torch.uint8, device=dev)
        self._h = self.policy.attach_trainer(self.gradient_length * B, learning_rate=self.learning_rate, max_grad_norm=self.max_grad_norm, loss_type=self.loss_type)

    def act(self, obs, teacher_obs):
        actions = self.policy.act(obs, teacher_obs)
        self.obs[self.t].copy_(obs)
        self.teacher_actions[self.t].copy_(self.policy.teacher_actions)
        return actions

    def process_env_step(self, rewards, dones, infos):
        self.dones[self.t].copy_(dones.reshape(-1))
        self.t += 1
        self.policy.reset(dones)

    def update(self):
        self._h.update(self.obs, self.teacher_actions, self.T, self.B, self.num_learning_epochs, self.gradient_length)
        s = self._h.stats().cpu()                                              # the update's only host synchronisation
        self.last_stats = s
        self.t = 0
        return float(s[C["GO2SIM_DISTILL_ST_LOSS"]])
