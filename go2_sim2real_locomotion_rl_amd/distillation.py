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

``StudentTeacherRecurrent`` (rsl_rl 2.3; include/go2sim_rdistill.h) puts an LSTM memory in front of the student, and optionally one in front of the teacher:
``Distillation`` takes it as it takes a StudentTeacher, collects in three launches per env step (both memories, both MLPs, the sampling) and updates by truncated
backpropagation through time over the same gradient windows, which carry the memory's state from one to the next and cut the gradient at the dones.

    policy = StudentTeacherRecurrent(49, 104, 16, student_hidden_dims=[256, 256, 256], teacher_hidden_dims=[512, 256, 128], rnn_hidden_dim=256, device=dev)
"""
import ctypes

import torch

from .capi import C, DistillCfg, Go2SimError, RDistillCfg, RDistillRoll, RDistillSeg, _ptr, load_hip_lib
from .distributed import is_multi
from .policy import Lstm, Mlp, flatten_lstm, flatten_sequential, lstm_shapes, lstm_step, policy_act, resolve_activation
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


def rdistill_schedule(T, E, G):
    """distill_windows as a recurrent student's update walks it: -> (windows, tail); a window is a list of segments (e, t0, t1), runs of consecutive steps
    t0 .. t1 of epoch e, and so is the tail.  Inside a segment the backward pass carries from step to step; a segment with t0 = 0 starts from the state
    saved at the rollout's first act, one with t0 > 0 (a window's first only) continues the carried state.  (3, 2, 4): [[(0, 0, 2), (1, 0, 0)]], [(1, 1, 2)]."""
    def segments(pairs):
        segs = []
        for e, t in pairs:
            if segs and segs[-1][0] == e and segs[-1][2] == t - 1:
                segs[-1] = (e, segs[-1][1], t)
            else:
                segs.append((e, t, t))
        return segs
    windows, tail = distill_windows(T, E, G)
    return [segments(w) for w in windows], segments(tail)


def _check_shapes(sd, prefix, dims, what):
    want = mlp_keys(prefix, dims)
    have = sorted(k for k in sd if k.startswith(prefix + "."))
    if have != sorted(k for k, _ in want):
        raise Go2SimError(f"{what}: the keys {have} are not those of a network with layer sizes {list(dims)}")
    for k, shape in want:
        if tuple(sd[k].shape) != tuple(shape):
            raise Go2SimError(f"{what}: {k} has shape {tuple(sd[k].shape)}, this model's is {tuple(shape)}")


def _check_memory(sd, prefix, dims, what):
    for k, shape in lstm_shapes(*dims):
        key = f"{prefix}.rnn.{k}"
        if key not in sd:
            raise Go2SimError(f"{what}: {key} is missing")
        if tuple(sd[key].shape) != tuple(shape):
            raise Go2SimError(f"{what}: {key} has shape {tuple(sd[key].shape)}, this model's is {tuple(shape)}")


def _recurrent_state_from_checkpoint(state_dict, student_dims, teacher_dims, student_memory, teacher_memory):
    """teacher_state_from_checkpoint(recurrent=True): the mapping of a StudentTeacherRecurrent.  `student_memory` / `teacher_memory` are (n_in, H) of
    memory_s / memory_t; teacher_memory None is a teacher without a memory."""
    keys = list(state_dict)
    has_actor, has_student = any(k.startswith("actor.") for k in keys), any(k.startswith("student.") for k in keys)
    if has_actor and has_student:
        raise Go2SimError("the state dict has both actor.* and student.* keys: neither a PPO nor a distillation checkpoint")
    if has_actor:
        has_mem = any(k.startswith("memory_a.") for k in keys)
        if has_mem and teacher_memory is None:
            raise Go2SimError("the checkpoint is a recurrent policy's (memory_a), but this StudentTeacherRecurrent's teacher has no memory: build it with teacher_recurrent=True")
        if not has_mem and teacher_memory is not None:
            raise Go2SimError("this StudentTeacherRecurrent's teacher is recurrent (teacher_recurrent=True), but the checkpoint has no memory_a.* keys: it is an ActorCritic's")
        mapped = {"teacher." + k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
        mapped.update({"memory_t." + k[len("memory_a."):]: v for k, v in state_dict.items() if k.startswith("memory_a.")})
        if teacher_dims is not None:
            _check_shapes(mapped, "teacher", teacher_dims, "teacher from a PPO checkpoint's actor")
        if teacher_memory is not None:
            _check_memory(mapped, "memory_t", teacher_memory, "memory_t from a PPO checkpoint's memory_a")
        return mapped, False
    if has_student:
        if "std" not in state_dict or not any(k.startswith("teacher.") for k in keys) or not any(k.startswith("memory_s.") for k in keys):
            raise Go2SimError("a recurrent distillation checkpoint needs student.*, memory_s.*, teacher.* and std")
        has_mem = any(k.startswith("memory_t.") for k in keys)
        if has_mem and teacher_memory is None:
            raise Go2SimError("the distillation checkpoint's teacher is recurrent (memory_t), but this StudentTeacherRecurrent's teacher has no memory")
        if not has_mem and teacher_memory is not None:
            raise Go2SimError("this StudentTeacherRecurrent's teacher is recurrent, but the distillation checkpoint has no memory_t.* keys")
        unknown = [k for k in keys if k != "std" and not k.startswith(("student.", "teacher.", "memory_s.", "memory_t."))]
        if unknown:
            raise Go2SimError(f"a recurrent distillation checkpoint holds student.*, memory_s.*, teacher.*, memory_t.* and std; unexpected keys {sorted(unknown)}")
        mapped = dict(state_dict)
        if student_dims is not None:
            _check_shapes(mapped, "student", student_dims, "student")
            if tuple(mapped["std"].shape) != (student_dims[-1],):
                raise Go2SimError(f"std has shape {tuple(mapped['std'].shape)}, this model's is {(student_dims[-1],)}")
        if teacher_dims is not None:
            _check_shapes(mapped, "teacher", teacher_dims, "teacher")
        if student_memory is not None:
            _check_memory(mapped, "memory_s", student_memory, "memory_s")
        if teacher_memory is not None:
            _check_memory(mapped, "memory_t", teacher_memory, "memory_t")
        return mapped, True
    raise Go2SimError("the state dict has neither actor.* keys (a PPO checkpoint, the teacher) nor student.* keys (a distillation checkpoint)")


def teacher_state_from_checkpoint(state_dict, student_dims=None, teacher_dims=None, *, recurrent=False, student_memory=None, teacher_memory=None):
    """What a ``model_state_dict`` means to a StudentTeacher, as rsl_rl reads it: -> (mapped state dict, resume).
      * a dict with ``actor.*`` keys is a PPO checkpoint: ``teacher.* <- actor.*`` and nothing else (critic and std are dropped), resume = False;
      * a dict with ``student.*`` keys is a distillation checkpoint: ``student.*``, ``teacher.*`` and ``std`` are all required, resume = True.
    With the layer sizes given, every mapped tensor's shape is checked and a mismatch refused with both shapes named.
    ``recurrent=True`` is the mapping of a StudentTeacherRecurrent: a PPO checkpoint of an ActorCriticRecurrent gives ``teacher.* <- actor.*`` and
    ``memory_t.* <- memory_a.*`` (critic, memory_c and std are dropped); a distillation checkpoint also needs ``memory_s.*`` (and ``memory_t.*`` when the
    teacher is recurrent).  ``student_memory`` / ``teacher_memory`` are the memories' (n_in, H); ``teacher_memory=None`` is a teacher without a memory: a
    recurrent checkpoint is refused for it, and a checkpoint without ``memory_a.*`` for a recurrent teacher."""
    if recurrent:
        return _recurrent_state_from_checkpoint(state_dict, student_dims, teacher_dims, student_memory, teacher_memory)
    keys = list(state_dict)
    if any(k.startswith("memory_") for k in keys):
        raise Go2SimError("the checkpoint is a recurrent policy's (memory_a / memory_c): StudentTeacher has no memories; a StudentTeacherRecurrent reads it "
                          "(teacher_state_from_checkpoint(..., recurrent=True))")
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


# ---- the recurrent student (include/go2sim_rdistill.h) --------------------------------------------------------------------------------------------
def memory_keys(prefix, n_in, n_hidden):
    """[(key, shape)] of one memory in state-dict (and flat) order"""
    return [(f"{prefix}.rnn.{k}", shape) for k, shape in lstm_shapes(n_in, n_hidden)]


def unflatten_recurrent_student(flat, dims, memory):
    """go2sim_rdistill_export's flat vector -> {student.*, memory_s.rnn.*}"""
    return unflatten_keys(flat, mlp_keys("student", dims) + memory_keys("memory_s", *memory))


class RDistillHandle(TrainerHandle):
    """One go2sim_rdistill handle over memory_s + student: pointers only.  `memory` is a policy.Lstm, `student` a policy.Mlp of the product library."""

    def __init__(self, lib, memory, student, n_actions, max_window_rows, *, learning_rate=1e-3, max_grad_norm=None, loss_type="mse", betas=(0.9, 0.999), eps=1e-8,
                 sub_envs=0, device=None):
        if loss_type not in LOSS_TYPES:
            raise Go2SimError(f"loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
        TrainerHandle.__init__(self, lib, "rdistill", device)
        self.memory, self.student = memory, student
        cfg = RDistillCfg(float(learning_rate), float(max_grad_norm) if max_grad_norm is not None else 0.0, betas[0], betas[1], eps,
                          C["GO2SIM_RDISTILL_" + loss_type.upper()], int(sub_envs))
        h = ctypes.c_void_p()
        lib.check(lib.fn("rdistill_create")(memory.h, student.h, ctypes.c_int(n_actions), ctypes.byref(cfg), ctypes.c_int(int(max_window_rows)), ctypes.byref(h)),
                  "rdistill_create")
        self._created(h)

    @staticmethod
    def roll(obs, teacher_actions, dones, h0, c0, h, c, n_steps, n_envs):
        ptrs = [_ptr(t).value for t in (obs, teacher_actions, dones, h0, c0, h, c)]
        return RDistillRoll(*ptrs, int(n_steps), int(n_envs))

    @staticmethod
    def _segs(segs):
        """[(t0, n_steps)] -> a C array"""
        return (RDistillSeg * len(segs))(*[RDistillSeg(int(t0), int(n)) for t0, n in segs])

    def window_grad(self, roll, segs):
        self._call("window_grad", ctypes.byref(roll), self._segs(segs), ctypes.c_int(len(segs)))

    def loss_only(self, roll, segs):
        self._call("loss_only", ctypes.byref(roll), self._segs(segs), ctypes.c_int(len(segs)))

    def apply(self):
        self._call("apply")

    def update(self, obs, teacher_actions, dones, h0, c0, h, c, n_steps, n_envs, n_epochs, gradient_length):
        roll = self.roll(obs, teacher_actions, dones, h0, c0, h, c, n_steps, n_envs)
        self._call("update", ctypes.byref(roll), ctypes.c_int(n_epochs), ctypes.c_int(gradient_length))


def rdistill_act(lib, mem_s, student, mem_t, teacher, obs, teacher_obs, std, reset, state_s, state_t, n_rows, seed, step, deterministic, actions, mean, teacher_actions,
                 stream=0):
    """go2sim_rdistill_act.  state_s / state_t: (h_in, c_in, h_out, c_out); mem_t and state_t are None for a teacher without a memory."""
    st = state_t if mem_t is not None else (None, None, None, None)
    rc = lib.fn("rdistill_act")(mem_s.h, student.h, mem_t.h if mem_t is not None else ctypes.c_void_p(0), teacher.h, _ptr(obs), _ptr(teacher_obs), _ptr(std), _ptr(reset),
                                *[_ptr(t) for t in state_s], *[_ptr(t) for t in st], ctypes.c_int(n_rows), ctypes.c_uint64(seed), ctypes.c_uint32(step),
                                ctypes.c_int(int(deterministic)), _ptr(actions), _ptr(mean), _ptr(teacher_actions), ctypes.c_void_p(stream))
    lib.check(rc, "rdistill_act")


class StudentTeacherRecurrent:
    """``rsl_rl.modules.StudentTeacherRecurrent`` (rsl_rl 2.3) with ``rnn_type="lstm"`` and one layer: ``memory_s = LSTM(num_student_obs -> H)`` in front of the
    student MLP and, with ``teacher_recurrent``, ``memory_t = LSTM(num_teacher_obs -> Ht)`` in front of the teacher MLP (include/go2sim_rdistill.h; Ht is
    ``teacher_rnn_hidden_dim``, by default H as in rsl_rl).  State-dict
    keys: ``student.*``, ``teacher.*``, ``std``, ``memory_s.rnn.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}`` and the same four under ``memory_t.rnn.``
    when the teacher is recurrent.  A PPO checkpoint of an ActorCriticRecurrent loads ``teacher.* <- actor.*`` and ``memory_t.* <- memory_a.*``.

    ``rnn_hidden_dim`` (alias ``rnn_hidden_size``) has NO default: a config without it is refused with an error that names this class and the key -- a
    StudentTeacher config whose class_name alone was changed is not silently given a memory of some size.  ``rnn_type="gru"`` and ``rnn_num_layers > 1`` are
    refused by name.

    ``reset(dones)`` does not touch the state: the dones become the ``reset`` argument of the next step's cell launch, which enters the done envs with h = c = 0.
    Unlike rsl_rl, the update leaves memory_t's state alone (DESIGN.md "Recurrent student")."""
    is_recurrent = True

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256), activation="elu",
                 init_noise_std=0.1, rnn_type="lstm", rnn_hidden_dim=None, rnn_num_layers=1, teacher_recurrent=False, *, rnn_hidden_size=None, teacher_rnn_hidden_dim=None, device=None, seed=1,
                 **kwargs):
        self.activation = resolve_activation(activation)
        unknown = {k: v for k, v in kwargs.items() if k != "class_name" and v is not None}
        if unknown:
            raise Go2SimError(f"StudentTeacherRecurrent does not implement {sorted(unknown)}")
        if str(rnn_type).lower() != "lstm":
            raise Go2SimError(f"StudentTeacherRecurrent's memories are LSTMs; rnn_type {rnn_type!r} (GRU) is not implemented")
        if int(rnn_num_layers) != 1:
            raise Go2SimError(f"StudentTeacherRecurrent's memories have one LSTM layer, got rnn_num_layers = {rnn_num_layers}")
        if rnn_hidden_dim is None:
            rnn_hidden_dim = rnn_hidden_size
        elif rnn_hidden_size is not None and int(rnn_hidden_size) != int(rnn_hidden_dim):
            raise Go2SimError(f"StudentTeacherRecurrent: rnn_hidden_dim = {rnn_hidden_dim} and its alias rnn_hidden_size = {rnn_hidden_size} disagree")
        if rnn_hidden_dim is None:
            raise Go2SimError("StudentTeacherRecurrent needs 'rnn_hidden_dim' (or its alias 'rnn_hidden_size') in its config: the memory's width has no default")
        H = int(rnn_hidden_dim)
        if H < 1 or H > C["GO2SIM_MLP_MAX_WIDTH"]:
            raise Go2SimError(f"StudentTeacherRecurrent: rnn_hidden_dim must be in 1 .. {C['GO2SIM_MLP_MAX_WIDTH']} (GO2SIM_MLP_MAX_WIDTH), got {H}")
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_actions, self.rnn_hidden_dim, self.teacher_recurrent = int(num_actions), H, bool(teacher_recurrent)
        Ht = int(teacher_rnn_hidden_dim) if teacher_rnn_hidden_dim is not None else H    # a teacher trained with another memory width keeps it
        if teacher_rnn_hidden_dim is not None and (not self.teacher_recurrent or Ht < 1 or Ht > C["GO2SIM_MLP_MAX_WIDTH"]):
            raise Go2SimError(f"StudentTeacherRecurrent: teacher_rnn_hidden_dim = {teacher_rnn_hidden_dim} needs teacher_recurrent=True and a width in 1 .. "
                              f"{C['GO2SIM_MLP_MAX_WIDTH']}")
        self._L = load_hip_lib()
        self._smem = (int(num_student_obs), H)
        self._tmem = (int(num_teacher_obs), Ht) if self.teacher_recurrent else None
        self._sdims = [H, *[int(d) for d in student_hidden_dims], self.num_actions]
        self._tdims = [Ht if self.teacher_recurrent else int(num_teacher_obs), *[int(d) for d in teacher_hidden_dims], self.num_actions]
        g = torch.Generator().manual_seed(int(seed))
        sd = {}
        for prefix, dims in (("student", self._sdims), ("teacher", self._tdims)):      # nn.Linear default init
            for l in range(len(dims) - 1):
                bound = 1.0 / (dims[l] ** 0.5)
                sd[f"{prefix}.{2 * l}.weight"] = (torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * bound
                sd[f"{prefix}.{2 * l}.bias"] = (torch.rand(dims[l + 1], generator=g) * 2 - 1) * bound
        g = torch.Generator().manual_seed(int(seed) + 0x5eed)                          # nn.LSTM's default init: every tensor uniform(-1 / sqrt(H), 1 / sqrt(H))
        for prefix, mem in (("memory_s", self._smem), ("memory_t", self._tmem)):
            if mem is not None:
                for k, shape in memory_keys(prefix, *mem):
                    sd[k] = (torch.rand(*shape, generator=g) * 2 - 1) / (mem[1] ** 0.5)
        sd["std"] = float(init_noise_std) * torch.ones(self.num_actions)
        self._student = self._teacher = self._mem_s = self._mem_t = self._trainer = None
        self.std = torch.ones(self.num_actions, device=self.device)
        self._host = {}
        self._load(sd, ("student", "memory_s", "teacher", "memory_t", "std"))
        self.loaded_teacher = False
        self._seed, self._step = int(seed), 0
        self._bufs = {}
        self._hid = None
        self._pending = {"s": None, "t": None}
        self._mean = self._teacher_actions = None

    # ---- parameters ------------------------------------------------------------------------------
    def _load(self, sd, parts):
        """(re)loads the named parts from a full-key state dict and keeps a host copy of them"""
        dev = self.device.index or 0
        for part in parts:
            if part in ("student", "teacher"):
                dims = self._sdims if part == "student" else self._tdims
                flat, d = flatten_sequential(sd, part, len(dims) - 1)
                if d != dims:
                    raise Go2SimError(f"state dict has {part} layer sizes {d}, this model's are {dims}")
                cur = getattr(self, "_" + part)
                if cur is None:
                    setattr(self, "_" + part, Mlp(self._L, dims, flat, dev, self.activation))
                else:
                    cur.set_params(flat)
                self._host.update({k: sd[k].detach().clone() for k, _ in mlp_keys(part, dims)})
            elif part in ("memory_s", "memory_t"):
                mem = self._smem if part == "memory_s" else self._tmem
                if mem is None:
                    continue
                flat, d = flatten_lstm(sd, part)
                if d != mem:
                    raise Go2SimError(f"state dict has {part} sizes {d}, this model's are {mem}")
                attr = "_mem_s" if part == "memory_s" else "_mem_t"
                if getattr(self, attr) is None:
                    setattr(self, attr, Lstm(self._L, *mem, flat, dev))
                else:
                    getattr(self, attr).set_params(flat)
                self._host.update({k: sd[k].detach().clone() for k, _ in memory_keys(part, *mem)})
            else:
                self.std.copy_(sd["std"].detach().reshape(self.num_actions))

    def load_state_dict(self, state_dict, strict=True):
        """A PPO checkpoint (``actor.*``; with a recurrent teacher also ``memory_a.*``) loads the teacher only and returns False (not a resume); a distillation
        checkpoint (``student.*``) loads everything strictly and returns True.  ``loaded_teacher`` is set either way."""
        mapped, resume = teacher_state_from_checkpoint(state_dict, self._sdims, self._tdims, recurrent=True, student_memory=self._smem, teacher_memory=self._tmem)
        self._load(mapped, ("student", "memory_s", "teacher", "memory_t", "std") if resume else ("teacher", "memory_t"))
        self.loaded_teacher = True
        return resume

    def state_dict(self):
        """student.* and memory_s.* as they are on the device (the optimizer writes them there once a trainer is attached), the teacher's as loaded, std."""
        out = {k: v.clone() for k, v in self._host.items()}
        if self._trainer is not None:
            out.update(unflatten_recurrent_student(self._trainer.export("PARAMS").cpu(), self._sdims, self._smem))
        out["std"] = self.std.detach().cpu().clone()
        return out

    def attach_trainer(self, gradient_length, num_envs, sub_envs=0, **hyper):
        """The go2sim_rdistill handle that updates memory_s and the student in place; its workspace holds a window of gradient_length steps of one env block."""
        block = min(int(num_envs), int(sub_envs) if sub_envs else C["GO2SIM_RDISTILL_SUB_ENVS"])
        self._trainer = RDistillHandle(self._L, self._mem_s, self._student, self.num_actions, int(gradient_length) * block, sub_envs=sub_envs, device=self.device, **hyper)
        return self._trainer

    # ---- the memories' state -----------------------------------------------------------------------
    def _state_for(self, B):
        """{"s": [h, c, spare h], "t": [...]} of [B][H] device tensors, zero at the start"""
        if self._hid is None or self._hid["s"][0].shape[0] != B:
            z = lambda H: torch.zeros(B, H, device=self.device, dtype=torch.float32)
            self._hid = {"s": [z(self._smem[1]) for _ in range(3)], "t": [z(self._tmem[1]) for _ in range(3)] if self.teacher_recurrent else None}
            self._pending = {"s": None, "t": None}
        return self._hid

    def student_state(self, B):
        """(h, c) of memory_s: the live arrays"""
        hid = self._state_for(B)
        return hid["s"][0], hid["s"][1]

    def _apply_pending(self, key):
        """the deferred zeroing done now, for a reader of the state that is not the cell launch"""
        d = self._pending[key]
        if d is not None and self._hid is not None and self._hid[key] is not None:
            for t in self._hid[key][:2]:
                t.masked_fill_(d.reshape(-1, 1) != 0, 0.0)
        self._pending[key] = None

    def save_student_state(self, h_out, c_out):
        """S: memory_s's state as the next step enters it (pending dones applied), copied into the caller's arrays"""
        h, c = self.student_state(h_out.shape[0])
        h_out.copy_(h); c_out.copy_(c)
        d = self._pending["s"]
        if d is not None:
            h_out.masked_fill_(d.reshape(-1, 1) != 0, 0.0); c_out.masked_fill_(d.reshape(-1, 1) != 0, 0.0)

    def _advance(self, key):
        """-> (h_in, c_in, h_out, c_out) of the next step of memory `key`, the pending reset; the step's h' becomes the state"""
        h, c, spare = self._hid[key]
        self._hid[key] = [spare, c, h]
        reset, self._pending[key] = self._pending[key], None
        return (h, c, spare, c), reset

    # ---- rsl_rl StudentTeacherRecurrent surface -------------------------------------------------------
    def _buf(self, name, shape):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(*shape, device=self.device, dtype=torch.float32)
            self._bufs[name] = t
        return t

    def act(self, observations, teacher_observations, deterministic=False):
        """Three launches: both memories' cell step (the done envs of the last step enter it with a zero state), both MLPs, the sampling kernel.  -> the
        student's actions; ``action_mean`` and ``teacher_actions`` hold the rest."""
        B = observations.shape[0]
        obs = observations.to(device=self.device, dtype=torch.float32).contiguous()
        tobs = teacher_observations.to(device=self.device, dtype=torch.float32).contiguous()
        if obs.shape[1] != self._smem[0] or tobs.shape[1] != (self._tmem[0] if self._tmem else self._tdims[0]) or tobs.shape[0] != B:
            raise Go2SimError(f"act: observations {tuple(obs.shape)} / {tuple(tobs.shape)}, the model reads [{B}][{self._smem[0]}] / "
                              f"[{B}][{self._tmem[0] if self._tmem else self._tdims[0]}]")
        self._state_for(B)
        if self.teacher_recurrent and self._pending["t"] is not self._pending["s"]:      # the two memories were stepped apart (evaluate / act_inference)
            self._apply_pending("s"); self._apply_pending("t")
        state_s, reset = self._advance("s")
        state_t = self._advance("t")[0] if self.teacher_recurrent else None
        actions, self._mean = self._buf("actions", (B, self.num_actions)), self._buf("mean", (B, self.num_actions))
        self._teacher_actions = self._buf("teacher_actions", (B, self.num_actions))
        rdistill_act(self._L, self._mem_s, self._student, self._mem_t, self._teacher, obs, tobs, self.std, reset, state_s, state_t, B, self._seed, self._step,
                     deterministic, actions, self._mean, self._teacher_actions, torch.cuda.current_stream(self.device).cuda_stream)
        self._step += 1
        return actions

    def act_inference(self, observations):
        """The deterministic student with its memory: one cell step of memory_s, then the student."""
        B = observations.shape[0]
        obs = observations.to(device=self.device, dtype=torch.float32).contiguous()
        self._state_for(B)
        (h, c, h_out, c_out), reset = self._advance("s")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        lstm_step(self._L, self._mem_s, obs, h, c, h_out, c_out, reset=reset, n_rows=B, stream=stream)
        actions, self._mean = self._buf("actions", (B, self.num_actions)), self._buf("mean", (B, self.num_actions))
        policy_act(self._L, self._student, None, h_out, None, self.std, B, self._seed, self._step, True, actions, self._mean, None, None, stream)
        self._step += 1
        return actions

    def evaluate(self, teacher_observations):
        """The teacher's actions (a recurrent teacher's memory steps)."""
        B = teacher_observations.shape[0]
        tobs = teacher_observations.to(device=self.device, dtype=torch.float32).contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        out = torch.empty(B, self.num_actions, device=self.device)
        if self.teacher_recurrent:
            self._state_for(B)
            (h, c, h_out, c_out), reset = self._advance("t")
            lstm_step(self._L, self._mem_t, tobs, h, c, h_out, c_out, reset=reset, n_rows=B, stream=stream)
            tobs = h_out
        self._teacher.forward(tobs, out, B, stream)
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
        """``dones`` ([B], any dtype): h and c of the done envs are zero when the next step enters them -- the mask is handed to that step's cell launch, a
        uint8 device tensor is kept by reference.  Without ``dones`` every state becomes zero.  ``hidden_states`` (((h_s, c_s), (h_t, c_t) or None), the
        shapes of get_hidden_states) replaces the state."""
        if hidden_states is not None:
            for key, hc in zip(("s", "t"), hidden_states):
                if hc is None or (key == "t" and not self.teacher_recurrent):
                    continue
                self._state_for(hc[0].reshape(-1, (self._smem if key == "s" else self._tmem)[1]).shape[0])
                for dst, src in zip(self._hid[key][:2], hc):
                    dst.copy_(src.reshape(dst.shape))
                self._pending[key] = None
        if self._hid is None:
            return
        if dones is None:
            if hidden_states is None:
                for key in ("s", "t"):
                    if self._hid[key] is not None:
                        for t in self._hid[key][:2]:
                            t.zero_()
                    self._pending[key] = None
            return
        d = dones.reshape(-1)
        if d.dtype != torch.uint8 or d.device != self._hid["s"][0].device or not d.is_contiguous():
            d = (d != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        for key in ("s", "t"):
            if self._hid[key] is None:
                continue
            if self._pending[key] is not None:                                 # two resets without a step between them: the first is applied now
                self._apply_pending(key)
            self._pending[key] = d

    def get_hidden_states(self):
        """((h_s, c_s), (h_t, c_t) or None), each [1][B][H] as nn.LSTM shapes them; views of the live state with the pending dones applied (None, None
        before the first step)"""
        if self._hid is None:
            return None, None
        for key in ("s", "t"):
            self._apply_pending(key)
        return tuple(None if self._hid[k] is None else (self._hid[k][0].unsqueeze(0), self._hid[k][1].unsqueeze(0)) for k in ("s", "t"))

    def detach_hidden_states(self, dones=None):
        """no-op: the state carries no autograd graph"""


# ---- the algorithm ---------------------------------------------------------------------------------------------------------------------------------
class Distillation(OptimizerState):
    """rsl_rl's Distillation on a StudentTeacher.  The activation is the policy's (``train_cfg["policy"]["activation"]``, one name for student and teacher):
    as in rsl_rl it lives in the config (``cfgs.pkl``), not in ``model_<it>.pt``, so a teacher checkpoint is interpreted with the student config's
    activation -- a teacher trained with another one loads without complaint and computes something else."""

    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse", device=None, *, group=None, sub_envs=None,
                 **kwargs):
        unknown = {k: v for k, v in kwargs.items() if k != "class_name" and v is not None}
        if unknown:
            raise Go2SimError(f"go2sim's Distillation does not implement {sorted(unknown)}")
        if loss_type not in LOSS_TYPES:
            raise Go2SimError(f"Distillation: loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
        if not isinstance(policy, (StudentTeacher, StudentTeacherRecurrent)):
            raise Go2SimError(f"Distillation needs a StudentTeacher or StudentTeacherRecurrent policy, got {type(policy).__name__}")
        if group is not None and is_multi(group):
            raise Go2SimError("Distillation over a multi-rank group is not implemented (the sharded distillation update is a follow-up)")
        if int(num_learning_epochs) < 1 or int(gradient_length) < 1 or not float(learning_rate) > 0.0:
            raise Go2SimError("Distillation needs num_learning_epochs >= 1, gradient_length >= 1 and learning_rate > 0")
        self.policy = policy
        self.device = policy.device if device is None else torch.device(device)
        self.num_learning_epochs, self.gradient_length = int(num_learning_epochs), int(gradient_length)
        self.learning_rate, self.max_grad_norm, self.loss_type = float(learning_rate), max_grad_norm, loss_type
        self.recurrent = bool(policy.is_recurrent)
        if sub_envs is not None and (not self.recurrent or int(sub_envs) < 1):
            raise Go2SimError("Distillation: sub_envs (the envs of a block of the recurrent update's window walk) needs a StudentTeacherRecurrent policy and a value >= 1")
        self.sub_envs = int(sub_envs) if sub_envs is not None else 0              # 0: GO2SIM_RDISTILL_SUB_ENVS
        self._h = None
        self.last_stats = None

    def init_storage(self, num_envs, num_transitions_per_env, student_obs_shape, teacher_obs_shape, action_shape):
        T, B, dev = int(num_transitions_per_env), int(num_envs), self.device
        self.T, self.B, self.t = T, B, 0
        self.obs = torch.zeros(T, B, *student_obs_shape, device=dev)
        self.teacher_actions = torch.zeros(T, B, *action_shape, device=dev)
        self.dones = torch.zeros(T, B, dtype=torch.uint8, device=dev)
        hyper = dict(learning_rate=self.learning_rate, max_grad_norm=self.max_grad_norm, loss_type=self.loss_type)
        if self.recurrent:                                                     # S: the student's state at the rollout's first act
            H = self.policy.rnn_hidden_dim
            self.saved_h, self.saved_c = torch.zeros(B, H, device=dev), torch.zeros(B, H, device=dev)
            self._h = self.policy.attach_trainer(self.gradient_length, B, sub_envs=self.sub_envs, **hyper)
        else:
            self._h = self.policy.attach_trainer(self.gradient_length * B, **hyper)

    def act(self, obs, teacher_obs):
        if self.recurrent and self.t == 0:
            self.policy.save_student_state(self.saved_h, self.saved_c)
        actions = self.policy.act(obs, teacher_obs)
        self.obs[self.t].copy_(obs)
        self.teacher_actions[self.t].copy_(self.policy.teacher_actions)
        return actions

    def process_env_step(self, rewards, dones, infos):
        self.dones[self.t].copy_(dones.reshape(-1))
        self.t += 1
        self.policy.reset(self.dones[self.t - 1] if self.recurrent else dones)   # the stored row is the next act's `reset`: no zeroing launch

    def update(self):
        if self.recurrent:
            h, c = self.policy.student_state(self.B)                          # the update carries the state in the live arrays and leaves the final one there
            self._h.update(self.obs, self.teacher_actions, self.dones, self.saved_h, self.saved_c, h, c, self.T, self.B, self.num_learning_epochs, self.gradient_length)
        else:
            self._h.update(self.obs, self.teacher_actions, self.T, self.B, self.num_learning_epochs, self.gradient_length)
        s = self._h.stats().cpu()                                              # the update's only host synchronisation
        self.last_stats = s
        self.t = 0
        return float(s[C["GO2SIM_DISTILL_ST_LOSS"]])
