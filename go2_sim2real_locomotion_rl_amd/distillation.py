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

from .capi import C, DistillCfg, Go2SimError, RDistillCfg, RDistillRoll, RDistillSeg, _ptr
from .distributed import is_multi
from .module_core import (MemoryState, PolicyModule, check_lstm_config, hidden_state_views, memory_keys, mlp_keys, student_teacher_init,
                          student_teacher_recurrent_init, unflatten_keys)
from .policy import lstm_step, policy_act, resolve_activation
from .trainer import OptimizerState, TrainerHandle

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
    for key, shape in memory_keys(prefix, *dims):
        if key not in sd:
            raise Go2SimError(f"{what}: {key} is missing")
        if tuple(sd[key].shape) != tuple(shape):
            raise Go2SimError(f"{what}: {key} has shape {tuple(sd[key].shape)}, this model's is {tuple(shape)}")


def teacher_state_from_checkpoint(state_dict, student_dims=None, teacher_dims=None, *, recurrent=False, student_memory=None, teacher_memory=None):
    """What a ``model_state_dict`` means to a StudentTeacher, as rsl_rl reads it: -> (mapped state dict, resume).
      * a dict with ``actor.*`` keys is a PPO checkpoint: ``teacher.* <- actor.*`` and nothing else (critic and std are dropped), resume = False;
      * a dict with ``student.*`` keys is a distillation checkpoint: ``student.*``, ``teacher.*`` and ``std`` are all required, resume = True.
    With the layer sizes given, every mapped tensor's shape is checked and a mismatch refused with both shapes named.
    ``recurrent=True`` is the mapping of a StudentTeacherRecurrent: a PPO checkpoint of an ActorCriticRecurrent gives ``teacher.* <- actor.*`` and
    ``memory_t.* <- memory_a.*`` (critic, memory_c and std are dropped); a distillation checkpoint also needs ``memory_s.*`` (and ``memory_t.*`` when the
    teacher is recurrent).  ``student_memory`` / ``teacher_memory`` are the memories' (n_in, H); ``teacher_memory=None`` is a teacher without a memory: a
    recurrent checkpoint is refused for it, and a checkpoint without ``memory_a.*`` for a recurrent teacher.  Without ``recurrent`` it is the same mapping
    with both memories absent, and any ``memory_*`` key is refused."""
    has = lambda prefix: any(k.startswith(prefix) for k in state_dict)
    if not recurrent:
        student_memory = teacher_memory = None
        if has("memory_"):
            raise Go2SimError("the checkpoint is a recurrent policy's (memory_a / memory_c): StudentTeacher has no memories; a StudentTeacherRecurrent reads it "
                              "(teacher_state_from_checkpoint(..., recurrent=True))")
    if has("actor.") and has("student."):
        raise Go2SimError("the state dict has both actor.* and student.* keys: neither a PPO nor a distillation checkpoint")
    if has("actor."):
        if has("memory_a.") and teacher_memory is None:
            raise Go2SimError("the checkpoint is a recurrent policy's (memory_a), but this StudentTeacherRecurrent's teacher has no memory: build it with teacher_recurrent=True")
        if not has("memory_a.") and teacher_memory is not None:
            raise Go2SimError("this StudentTeacherRecurrent's teacher is recurrent (teacher_recurrent=True), but the checkpoint has no memory_a.* keys: it is an ActorCritic's")
        mapped = {"teacher." + k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
        mapped.update({"memory_t." + k[len("memory_a."):]: v for k, v in state_dict.items() if k.startswith("memory_a.")})
        resume, teacher_from, memory_from = False, "teacher from a PPO checkpoint's actor", "memory_t from a PPO checkpoint's memory_a"
    elif has("student."):
        kind = "a recurrent distillation checkpoint" if recurrent else "a distillation checkpoint"
        needed = ["student.", "memory_s.", "teacher."] if recurrent else ["student.", "teacher."]
        if "std" not in state_dict or not all(has(p) for p in needed):
            raise Go2SimError(f"{kind} needs {', '.join(p + '*' for p in needed)} and std")
        if has("memory_t.") and teacher_memory is None:
            raise Go2SimError("the distillation checkpoint's teacher is recurrent (memory_t), but this StudentTeacherRecurrent's teacher has no memory")
        if not has("memory_t.") and teacher_memory is not None:
            raise Go2SimError("this StudentTeacherRecurrent's teacher is recurrent, but the distillation checkpoint has no memory_t.* keys")
        allowed = needed + ["memory_t."] * recurrent
        unknown = [k for k in state_dict if k != "std" and not k.startswith(tuple(allowed))]
        if unknown:
            raise Go2SimError(f"{kind} holds {', '.join(p + '*' for p in allowed)} and std; unexpected keys {sorted(unknown)}")
        mapped = dict(state_dict)
        if student_dims is not None:
            _check_shapes(mapped, "student", student_dims, "student")
            if tuple(mapped["std"].shape) != (student_dims[-1],):
                raise Go2SimError(f"std has shape {tuple(mapped['std'].shape)}, this model's is {(student_dims[-1],)}")
        if student_memory is not None:
            _check_memory(mapped, "memory_s", student_memory, "memory_s")
        resume, teacher_from, memory_from = True, "teacher", "memory_t"
    else:
        raise Go2SimError("the state dict has neither actor.* keys (a PPO checkpoint, the teacher) nor student.* keys (a distillation checkpoint)")
    if teacher_dims is not None:
        _check_shapes(mapped, "teacher", teacher_dims, teacher_from)
    if teacher_memory is not None:
        _check_memory(mapped, "memory_t", teacher_memory, memory_from)
    return mapped, resume


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
class StudentTeacher(PolicyModule):
    _smem = _tmem = _mem_s = _mem_t = None                                   # the memories' (n_in, H) and handles: the recurrent subclass's

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims=(256, 256, 256), teacher_hidden_dims=(256, 256, 256), activation="elu",
                 init_noise_std=0.1, *, device=None, seed=1, **kwargs):
        self.activation = resolve_activation(activation)                          # one name for student and teacher, as in rsl_rl; refused before the device is touched
        unknown = {k: v for k, v in kwargs.items() if k != "class_name" and v is not None}
        if unknown:
            raise Go2SimError(f"{type(self).__name__} does not implement {sorted(unknown)}")
        PolicyModule.__init__(self, num_actions, device, seed)
        self._sdims = [int(num_student_obs), *[int(d) for d in student_hidden_dims], self.num_actions]
        self._tdims = [int(num_teacher_obs), *[int(d) for d in teacher_hidden_dims], self.num_actions]
        self._load(self._initial_state(init_noise_std, seed), resume=True)
        self.loaded_teacher = False
        self._teacher_actions = None

    # ---- parameters ------------------------------------------------------------------------------
    def _initial_state(self, init_noise_std, seed):
        return student_teacher_init(self._sdims, self._tdims, init_noise_std, seed)

    def _load(self, sd, resume):
        """the teacher's side from a full-key state dict; with `resume` the student's side and std as well"""
        parts = [("_teacher", "mlp", "teacher", self._tdims), ("_mem_t", "lstm", "memory_t", self._tmem)]
        if resume:
            parts = [("_student", "mlp", "student", self._sdims), ("_mem_s", "lstm", "memory_s", self._smem)] + parts
        self._set_parts(parts, sd)
        if resume:
            self._set_std(sd)

    def load_state_dict(self, state_dict, strict=True):
        """rsl_rl's StudentTeacher.load_state_dict: a PPO checkpoint (``actor.*``; for a recurrent teacher also ``memory_a.*``) loads the teacher only and
        returns False (not a resume); a distillation checkpoint (``student.*``) loads everything strictly and returns True.  ``loaded_teacher`` is set either way."""
        mapped, resume = teacher_state_from_checkpoint(state_dict, self._sdims, self._tdims, recurrent=self.is_recurrent, student_memory=self._smem,
                                                       teacher_memory=self._tmem)
        self._load(mapped, resume)
        self.loaded_teacher = True
        return resume

    def state_dict(self):
        """The student's side as it is on the device (the optimizer writes it there once a trainer is attached), the teacher's as loaded, std."""
        out = self._host_state()
        if self._trainer is not None:
            flat = self._trainer.export("PARAMS").cpu()
            out.update(unflatten_recurrent_student(flat, self._sdims, self._smem) if self._smem else unflatten_student(flat, self._sdims))
        return out

    def attach_trainer(self, max_window_rows, **hyper):
        """The go2sim_distill handle that updates the student's device parameters in place; the optimizer state lives in it."""
        self._trainer = DistillHandle(self._L, self._student, self.num_actions, max_window_rows, device=self.device, **hyper)
        return self._trainer

    @property
    def num_teacher_obs(self):
        """the width of the rows the teacher's side reads (a recurrent teacher's memory reads them)"""
        return self._tmem[0] if self._tmem else self._tdims[0]

    # ---- rsl_rl StudentTeacher surface -------------------------------------------------------------------
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
    def teacher_actions(self):
        return self._teacher_actions


# ---- the recurrent student (include/go2sim_rdistill.h) --------------------------------------------------------------------------------------------
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


class StudentTeacherRecurrent(StudentTeacher):
    """``rsl_rl.modules.StudentTeacherRecurrent`` (rsl_rl 2.3) with ``rnn_type="lstm"`` and one layer: ``memory_s = LSTM(num_student_obs -> H)`` in front of the
    student MLP and, with ``teacher_recurrent``, ``memory_t = LSTM(num_teacher_obs -> Ht)`` in front of the teacher MLP (include/go2sim_rdistill.h; Ht is
    ``teacher_rnn_hidden_dim``, by default H as in rsl_rl).  State-dict
    keys: ``student.*``, ``teacher.*``, ``std``, the four ``nn.LSTM`` keys (module_core.lstm_shapes) under ``memory_s.rnn.`` and the same four under ``memory_t.rnn.``
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
        if rnn_hidden_dim is None:
            rnn_hidden_dim = rnn_hidden_size
        elif rnn_hidden_size is not None and int(rnn_hidden_size) != int(rnn_hidden_dim):
            raise Go2SimError(f"StudentTeacherRecurrent: rnn_hidden_dim = {rnn_hidden_dim} and its alias rnn_hidden_size = {rnn_hidden_size} disagree")
        if rnn_hidden_dim is None:
            raise Go2SimError("StudentTeacherRecurrent needs 'rnn_hidden_dim' (or its alias 'rnn_hidden_size') in its config: the memory's width has no default")
        H = self.rnn_hidden_dim = check_lstm_config("StudentTeacherRecurrent", rnn_type, rnn_num_layers, rnn_hidden_dim, "rnn_hidden_dim")
        self.teacher_recurrent = bool(teacher_recurrent)
        Ht = int(teacher_rnn_hidden_dim) if teacher_rnn_hidden_dim is not None else H    # a teacher trained with another memory width keeps it
        if teacher_rnn_hidden_dim is not None and (not self.teacher_recurrent or Ht < 1 or Ht > C["GO2SIM_MLP_MAX_WIDTH"]):
            raise Go2SimError(f"StudentTeacherRecurrent: teacher_rnn_hidden_dim = {teacher_rnn_hidden_dim} needs teacher_recurrent=True and a width in 1 .. "
                              f"{C['GO2SIM_MLP_MAX_WIDTH']}")
        self._smem = (int(num_student_obs), H)
        self._tmem = (int(num_teacher_obs), Ht) if self.teacher_recurrent else None
        super().__init__(H, Ht if self.teacher_recurrent else num_teacher_obs, num_actions, student_hidden_dims, teacher_hidden_dims, activation, init_noise_std,
                         device=device, seed=seed, **kwargs)
        self._hid = (MemoryState(H, self.device), MemoryState(Ht, self.device) if self.teacher_recurrent else None)      # memory_s's, memory_t's

    def _initial_state(self, init_noise_std, seed):
        return student_teacher_recurrent_init(self._sdims, self._tdims, self._smem, self._tmem, init_noise_std, seed)

    def attach_trainer(self, gradient_length, num_envs, sub_envs=0, **hyper):
        """The go2sim_rdistill handle that updates memory_s and the student in place; its workspace holds a window of gradient_length steps of one env block."""
        block = min(int(num_envs), int(sub_envs) if sub_envs else C["GO2SIM_RDISTILL_SUB_ENVS"])
        self._trainer = RDistillHandle(self._L, self._mem_s, self._student, self.num_actions, int(gradient_length) * block, sub_envs=sub_envs, device=self.device, **hyper)
        return self._trainer

    # ---- the memories' state -----------------------------------------------------------------------
    def _states(self, B):
        """(memory_s's MemoryState, memory_t's or None) for B rows"""
        s, t = self._hid
        return s.rows(B), t.rows(B) if t is not None else None

    def student_state(self, B):
        """(h, c) of memory_s: the live arrays"""
        s, _ = self._states(B)
        return s.h, s.c

    def save_student_state(self, h_out, c_out):
        """S: memory_s's state as the next step enters it (pending dones applied), copied into the caller's arrays"""
        self._states(h_out.shape[0])[0].copy_entering(h_out, c_out)

    # ---- rsl_rl StudentTeacherRecurrent surface -------------------------------------------------------
    def act(self, observations, teacher_observations, deterministic=False):
        """Three launches: both memories' cell step (the done envs of the last step enter it with a zero state), both MLPs, the sampling kernel.  -> the
        student's actions; ``action_mean`` and ``teacher_actions`` hold the rest."""
        B = observations.shape[0]
        obs = observations.to(device=self.device, dtype=torch.float32).contiguous()
        tobs = teacher_observations.to(device=self.device, dtype=torch.float32).contiguous()
        if obs.shape[1] != self._smem[0] or tobs.shape[1] != self.num_teacher_obs or tobs.shape[0] != B:
            raise Go2SimError(f"act: observations {tuple(obs.shape)} / {tuple(tobs.shape)}, the model reads [{B}][{self._smem[0]}] / [{B}][{self.num_teacher_obs}]")
        s, t = self._states(B)
        if t is not None and t.pending is not s.pending:                   # the two memories were stepped apart (evaluate / act_inference)
            s.apply_pending(); t.apply_pending()
        reset, state_s, state_t = s.take_pending(), s.advance(), None
        if t is not None:
            t.take_pending()                                                  # the same mask: one `reset` argument serves both memories
            state_t = t.advance()
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
        s, _ = self._states(B)
        reset, (h, c, h_out, c_out) = s.take_pending(), s.advance()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        lstm_step(self._L, self._mem_s, obs, h, c, h_out, c_out, reset=reset, n_rows=B, stream=stream)
        actions, self._mean = self._buf("actions", (B, self.num_actions)), self._buf("mean", (B, self.num_actions))
        policy_act(self._L, self._student, None, h_out, None, self.std, B, self._seed, self._step, True, actions, self._mean, None, None, stream)
        self._step += 1
        return actions

    def evaluate(self, teacher_observations):
        """The teacher's actions (a recurrent teacher's memory steps)."""
        if self._tmem is None:
            return super().evaluate(teacher_observations)
        B = teacher_observations.shape[0]
        tobs = teacher_observations.to(device=self.device, dtype=torch.float32).contiguous()
        _, t = self._states(B)
        reset, (h, c, h_out, c_out) = t.take_pending(), t.advance()
        lstm_step(self._L, self._mem_t, tobs, h, c, h_out, c_out, reset=reset, n_rows=B, stream=torch.cuda.current_stream(self.device).cuda_stream)
        return super().evaluate(h_out)

    def reset(self, dones=None, hidden_states=None):
        """``dones`` ([B], any dtype): h and c of the done envs are zero when the next step enters them -- the mask is handed to that step's cell launch, a
        uint8 device tensor is kept by reference.  Without ``dones`` every state becomes zero.  ``hidden_states`` (((h_s, c_s), (h_t, c_t) or None), the
        shapes of get_hidden_states) replaces the state."""
        states = [st for st in self._hid if st is not None]
        if hidden_states is not None:
            for st, hc in zip(self._hid, hidden_states):
                if st is not None and hc is not None:
                    st.replace(*hc)
                    self._states(st.B)                                        # both memories hold the same rows: another B allocates the other afresh
        if self._hid[0].B == 0:
            return
        if dones is None:
            if hidden_states is None:
                for st in states:
                    st.zero()
            return
        d = dones.reshape(-1)
        if d.dtype != torch.uint8 or d.device != self._hid[0].h.device or not d.is_contiguous():
            d = (d != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        for st in states:
            st.defer(d)

    def get_hidden_states(self):
        """((h_s, c_s), (h_t, c_t) or None), each [1][B][H] as nn.LSTM shapes them; views of the live state with the pending dones applied (None, None
        before the first step)"""
        return hidden_state_views(self._hid)

    def detach_hidden_states(self, dones=None):
        """no-op: the state carries no autograd graph"""


# ---- the algorithm ---------------------------------------------------------------------------------------------------------------------------------
class Distillation(OptimizerState):
    """rsl_rl's Distillation on a StudentTeacher.  The activation is the policy's (``train_cfg["policy"]["activation"]``, one name for student and teacher):
    as in rsl_rl it lives in the config (``cfgs.pkl``), not in ``model_<it>.pt``, so a teacher checkpoint is interpreted with the student config's
    activation -- a teacher trained with another one loads without complaint and computes something else."""
    result_names, symmetry = ("behavior_loss",), None                         # of what update() returns, as the runner logs it; no symmetry_cfg

    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse", device=None, *, group=None, sub_envs=None,
                 **kwargs):
        unknown = {k: v for k, v in kwargs.items() if k != "class_name" and v is not None}
        if unknown:
            raise Go2SimError(f"go2sim's Distillation does not implement {sorted(unknown)}")
        if loss_type not in LOSS_TYPES:
            raise Go2SimError(f"Distillation: loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
        if not isinstance(policy, StudentTeacher):
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

    def compute_returns(self, last_critic_obs):
        """rsl_rl's no-op: the targets are the stored teacher actions"""

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
