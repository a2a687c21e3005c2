"""ctypes binding of the go2sim C ABI (include/go2sim.h).

One wrapper class serves both libraries that export the ABI:
  * csrc/libgo2sim.so        (prefix ``go2sim_``,     HIP/gfx950 product, device pointers)
  * oracle/libgo2sim_cpu.so  (prefix ``go2sim_cpu_``, CPU twin used ONLY by tests / smoke / cpu_baseline)

Enum values (fields, cfg indices, rewards, env buffers) are parsed from the header text so that the
Python side can never drift from the C side.
"""
import ctypes
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(REPO_ROOT, "include", "go2sim.h")
HIP_LIB = os.path.join(_HERE, "csrc", "libgo2sim.so")
CPU_LIB = os.path.join(REPO_ROOT, "oracle", "libgo2sim_cpu.so")
CPU_LIB_FAST = os.path.join(REPO_ROOT, "oracle", "libgo2sim_cpu_fast.so")


def _parse_header(path=HEADER):
    txt = open(path).read()
    txt_nc = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    consts = {}
    for m in re.finditer(r"#define\s+(GO2SIM_\w+)\s+(-?(?:0x[0-9A-Fa-f]+|\d+))\s*$", txt_nc, flags=re.M):
        consts[m.group(1)] = int(m.group(2), 0)
    for em in re.finditer(r"enum\s+\w+\s*\{(.*?)\}", txt_nc, flags=re.S):
        val = -1
        for item in em.group(1).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                name, expr = [s.strip() for s in item.split("=", 1)]
                val = int(eval(expr, {}, dict(consts)))
            else:
                name, val = item, val + 1
            consts[name] = val
    decls = re.findall(r"^int\s+(go2sim_\w+)\s*\(", txt_nc, flags=re.M)
    return consts, decls


C, DECLARED_FUNCS = _parse_header()
PRODUCT_ONLY_FUNCS = []


def _product_header(name, funcs=PRODUCT_ONLY_FUNCS):
    """include/go2sim_<name>.h: its constants go into C, its functions onto `funcs` -- by default the list of what only the product library has (no
    go2sim_cpu_ twin; the diagnostic and shape builds do not carry it either).  -> (path, the header's declared functions)"""
    path = os.path.join(REPO_ROOT, "include", f"go2sim_{name}.h")
    consts, decls = _parse_header(path)
    C.update(consts)
    funcs.extend(decls)
    return path, decls


_product_header("policy", DECLARED_FUNCS)                                      # policy inference lives in both libraries
TRAIN_HEADER, DECLARED_TRAIN_FUNCS = _product_header("train")                  # the PPO update
RNN_HEADER, DECLARED_RNN_FUNCS = _product_header("rnn")                        # the recurrent (LSTM) policy: the memory cell and the update through time
NORM_HEADER, DECLARED_NORM_FUNCS = _product_header("norm")                     # the empirical observation normaliser
LIDAR_HEADER, DECLARED_LIDAR_FUNCS = _product_header("lidar")                  # the LIDAR terrain scan
STAIRINFO_HEADER, DECLARED_STAIRINFO_FUNCS = _product_header("stairinfo")      # the four-value stair info
DISTILL_HEADER, DECLARED_DISTILL_FUNCS = _product_header("distill")            # teacher-student distillation
RDISTILL_HEADER, DECLARED_RDISTILL_FUNCS = _product_header("rdistill")         # distillation with a recurrent student
ACT_HEADER, DECLARED_ACT_FUNCS = _product_header("activation")                 # the hidden-layer activation of an MLP
RND_HEADER, DECLARED_RND_FUNCS = _product_header("rnd")                        # random network distillation: the intrinsic reward and the predictor's update
TILES_HEADER, DECLARED_TILES_FUNCS = _product_header("tiles")                  # the rough-terrain walk env: float heightfield, ground query
WELLS_HEADER, DECLARED_WELLS_FUNCS = _product_header("wells")                  # the stairwell env: 11 x 11 scan, alive term
STATE_HEADER, DECLARED_STATE_FUNCS = _product_header("state")                  # env snapshots: the record's size, save, load
CTERMS_HEADER, DECLARED_CTERMS_FUNCS = _product_header("cterms")                # the contact terms: body_contact, stumble
EVALSTATS_HEADER, DECLARED_EVALSTATS_FUNCS = _product_header("evalstats")       # the evaluation statistics: per-env and per-bin records
RNG_HEADER, _ = _product_header("rng", [])                                     # the purposes of the random stream (constants only; both libraries)
# train_cfg["policy"]["activation"] as rsl_rl's resolve_nn_activation spells it -> GO2SIM_ACT_*
ACTIVATIONS = {n: C["GO2SIM_ACT_" + n.upper()] for n in ("elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "identity")}


class PpoCfg(ctypes.Structure):
    """go2sim_ppo_cfg_t"""
    _fields_ = [(n, ctypes.c_double) for n in ("clip_param", "desired_kl", "entropy_coef", "learning_rate", "max_grad_norm", "value_loss_coef",
                                               "beta1", "beta2", "eps", "lr_min", "lr_max")] + [("use_clipped_value_loss", ctypes.c_int), ("adaptive", ctypes.c_int)]


class DistillCfg(ctypes.Structure):
    """go2sim_distill_cfg_t"""
    _fields_ = [(n, ctypes.c_double) for n in ("learning_rate", "max_grad_norm", "beta1", "beta2", "eps")] + [("loss_type", ctypes.c_int), ("sub_rows", ctypes.c_int)]


class RndCfg(ctypes.Structure):
    """go2sim_rnd_cfg_t"""
    _fields_ = [(n, ctypes.c_double) for n in ("learning_rate", "beta1", "beta2", "eps")] + [("reward_normalization", ctypes.c_int)]


class RDistillCfg(ctypes.Structure):
    """go2sim_rdistill_cfg_t"""
    _fields_ = [(n, ctypes.c_double) for n in ("learning_rate", "max_grad_norm", "beta1", "beta2", "eps")] + [("loss_type", ctypes.c_int), ("sub_envs", ctypes.c_int)]


class RDistillRoll(ctypes.Structure):
    """go2sim_rdistill_roll_t: device pointers of one rollout, the state S at its first act and the carried state"""
    FIELDS = ("obs", "teacher_actions", "dones", "h0", "c0", "h", "c")
    _fields_ = [(n, ctypes.c_void_p) for n in FIELDS] + [("n_steps", ctypes.c_int), ("n_envs", ctypes.c_int)]


class RDistillSeg(ctypes.Structure):
    """go2sim_rdistill_seg_t"""
    _fields_ = [("t0", ctypes.c_int), ("n_steps", ctypes.c_int)]


class PpoBatch(ctypes.Structure):
    """go2sim_ppo_batch_t: device pointers of the rollout's flat row arrays"""
    FIELDS = ("obs", "critic_obs", "actions", "target_values", "returns", "advantages", "old_log_prob", "old_mu", "old_sigma")
    _fields_ = [(n, ctypes.c_void_p) for n in FIELDS]


class PpoMirror(ctypes.Structure):
    """go2sim_ppo_mirror_t: three signed permutations as device tables, the two flags and the mirror-loss coefficient"""
    TABLES = ("obs_src", "obs_sign", "critic_src", "critic_sign", "action_src", "action_sign")
    _fields_ = [(n, ctypes.c_void_p) for n in TABLES] + [("use_data_augmentation", ctypes.c_int), ("use_mirror_loss", ctypes.c_int),
                                                         ("mirror_loss_coeff", ctypes.c_double)]


class PpoRnnState(ctypes.Structure):
    """go2sim_ppo_rnn_state_t: the memories' state at the rollout's first act and the rollout's dones"""
    FIELDS = ("h_a", "c_a", "h_c", "c_c", "dones")
    _fields_ = [(n, ctypes.c_void_p) for n in FIELDS]


class EnvGlobals(ctypes.Structure):
    _fields_ = [
        ("level", ctypes.c_double), ("timeout_rate_ema", ctypes.c_double), ("tracking_ema", ctypes.c_double), ("fall_rate_ema", ctypes.c_double),
        ("curr_timeout_total", ctypes.c_double), ("curr_tracking_sum", ctypes.c_double),
        ("obs_noise_level_cur", ctypes.c_double), ("action_noise_std_cur", ctypes.c_double),
        ("push_force_lo", ctypes.c_double), ("push_force_hi", ctypes.c_double),
        ("cmd_x_lo", ctypes.c_double), ("cmd_x_hi", ctypes.c_double), ("cmd_y_lo", ctypes.c_double), ("cmd_y_hi", ctypes.c_double),
        ("cmd_yaw_lo", ctypes.c_double), ("cmd_yaw_hi", ctypes.c_double), ("t_sample", ctypes.c_double),
        ("ema_valid", ctypes.c_int), ("ready_streak", ctypes.c_int), ("hard_streak", ctypes.c_int), ("cooldown", ctypes.c_int),
        ("curr_ep_total", ctypes.c_int), ("curr_tracking_n", ctypes.c_int),
        ("push_enable", ctypes.c_int), ("push_interval", ctypes.c_int), ("push_counter", ctypes.c_int), ("delay_max_cur", ctypes.c_int),
        ("global_dr_reset_counter", ctypes.c_int),
        ("friction", ctypes.c_float), ("mass_shift", ctypes.c_float), ("com_shift", ctypes.c_float * 3), ("leg_mass_shift", ctypes.c_float * 4),
        ("action_write_idx", ctypes.c_int), ("step_count", ctypes.c_uint), ("reset_calls", ctypes.c_uint),
        ("last_reset_count", ctypes.c_int), ("last_episode_rew", ctypes.c_float * 32),
        ("n_reset_now", ctypes.c_int), ("ep_acc", ctypes.c_float * 32), ("terrain_mean_row", ctypes.c_float), ("terrain_row_sum", ctypes.c_int),
        ("lock_terrain_rows", ctypes.c_int), ("sync_calls", ctypes.c_int), ("shard_counters", ctypes.c_double * 5),
        ("engine_kp", ctypes.c_float), ("engine_kd", ctypes.c_float),
    ]

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out


def _ptr(x, strided=False):
    """The one pointer helper of the package: None (NULL), a raw address (int), a numpy array, a torch tensor or a ctypes object -> what ctypes passes.
    Arrays and tensors must be contiguous unless `strided`: then the caller hands the strides over next to the base address."""
    if x is None:
        return ctypes.c_void_p(0)
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if isinstance(x, np.ndarray):
        assert strided or x.flags["C_CONTIGUOUS"]
        return ctypes.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        assert strided or x.is_contiguous()
        return ctypes.c_void_p(x.data_ptr())
    return x


class Go2SimError(RuntimeError):
    pass


class Go2SimLib:
    """Thin, explicit binding: one Python method per exported C function."""

    def __init__(self, path, prefix):
        if not os.path.exists(path):
            raise Go2SimError(
                f"go2sim shared library not found: {path}. Build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (the product has no CPU fallback)."
            )
        self.path, self.prefix = path, prefix
        self.lib = ctypes.CDLL(path)
        self.is_device = prefix == "go2sim_"
        for name in DECLARED_FUNCS:
            fn = getattr(self.lib, prefix + name[len("go2sim_"):])
            fn.restype = ctypes.c_int
        if self.is_device:
            for name in PRODUCT_ONLY_FUNCS:                                    # the diagnostic and shape builds (build.build_hip_variant) do not carry the update
                if hasattr(self.lib, name):
                    getattr(self.lib, name).restype = ctypes.c_int

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def check(self, rc, what):
        if rc != 0:
            raise Go2SimError(f"{self.prefix}{what} failed with status {rc}")


class Handle:
    """Owns one handle of a library: (lib, h, the name of the entry that destroys it).  A subclass calls Handle.__init__ before its create call and sets
    `h` after it, so a refused create leaves nothing to release; close() may be called any number of times."""

    def __init__(self, lib, destroy):
        self._owner, self._destroy, self.h = lib, destroy, None

    def close(self):
        if getattr(self, "h", None):
            self._owner.fn(self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_device_tensor(ptr, shape, dtype, device):
    """Zero-copy torch view of library-owned device memory (no ownership transfer, include/go2sim.h)."""
    itemsize = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s

    class _Mem:
        __cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": {torch.float32: "<f4", torch.int32: "<i4", torch.uint8: "|u1"}[dtype],
            "data": (int(ptr), False), "version": 2, "strides": None,
        }

    assert n * itemsize > 0
    return torch.as_tensor(_Mem(), device=device)


def check_layout_widths(name, env_cfg, obs_cfg, widths):
    """The proprioceptive width n_in of a cfg whose obs_cfg carries `widths` = (n_in, num_obs, num_privileged_obs), what the `name` layout gives;
    Go2SimError (naming both pairs) otherwise."""
    n_in, want_obs, want_priv = widths
    num_actions, have = int(env_cfg["num_actions"]), (obs_cfg["num_obs"], obs_cfg.get("num_privileged_obs"))
    if num_actions not in ((16,) if env_cfg.get("pls_enable", False) else (16, 12)):
        raise Go2SimError(f"the {name} layout has 16 actions (12 with pls_enable=False), got {num_actions}")
    if have != (want_obs, want_priv):
        raise Go2SimError(f"obs_cfg gives num_obs / num_privileged_obs = {have[0]} / {have[1]}, the {name} layout gives {want_obs} / {want_priv}")
    return n_in


class EnvLaunch(Handle):
    """One of the launches Go2Env runs after the step's own (LidarScan, StairInfo, WellScan, ContactTerms): the handle of go2sim_<NAME>_create with its
    device, stream, clear and host-array state, and what Go2Env asks of every launch:

        inner_widths(env_cfg, obs_cfg)   (num_obs, num_privileged_obs) of the rows the step kernels write for it (a layout launch; checks obs_cfg)
        launch(env, inner_obs, inner_priv), clear(idx), log(mask), episode_entries(), curriculum_entries(level)
        state_schema(B), state_dict(), load_state_dict(state)      its keys of Go2Env.state_dict() (ENV_STATE.md)

    An episode term keeps `ep`, the device view [..., n_envs] of the per-env records of the last finished episode, and `ep_log`, their logged means."""
    NAME = STATE_FAMILY = None
    WIDENS_OBS = True                  # the launch writes the actor row as well: the step kernels write an inner one
    logs, ep, ep_log = False, None, None

    def __init__(self, n_envs, device=None):
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_envs = int(n_envs)
        self._L = load_hip_lib()
        Handle.__init__(self, self._L, self.NAME + "_destroy")

    def _call(self, entry, *args):
        self._L.check(self._L.fn(f"{self.NAME}_{entry}")(self.h, *args), f"{self.NAME}_{entry}")

    def _create(self, cfg, *arrays):
        h = ctypes.c_void_p()
        self._L.check(self._L.fn(self.NAME + "_create")(ctypes.c_int(self.device.index or 0), ctypes.byref(cfg), *arrays, ctypes.byref(h)), self.NAME + "_create")
        self.h = h
        self._step_fn = self._L.fn(self.NAME + "_step")                    # looked up once: step() runs every env step

    def _step(self, *args):
        rc = self._step_fn(self.h, *args, self._stream())
        if rc:
            self._L.check(rc, self.NAME + "_step")

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def clear(self, envs_idx=None):
        """For ``envs_idx`` (int32 device tensor) or for every env: stored rows := 0; an episode term's hand-over without a step (record the per-second
        value, zero sum and count)."""
        self._call("clear", _ptr(envs_idx), ctypes.c_int(0 if envs_idx is None else envs_idx.numel()), self._stream())

    def _get_host(self, entry, shape, *dtypes):
        """CPU tensors of `shape`, one per dtype, filled by go2sim_<NAME>_<entry>; waits for the stream."""
        out = [np.zeros(shape, t) for t in dtypes]
        self._call(entry, *(_ptr(a) for a in out), self._stream())
        return tuple(torch.from_numpy(a) for a in out)

    def _set_host(self, entry, what, shape, *values):
        """go2sim_<NAME>_<entry> with `values` = (tensor, torch dtype) ..., each of `shape`; Go2SimError "<what> shape ..., got ..." otherwise."""
        arrs = [np.ascontiguousarray(torch.as_tensor(v).detach().cpu().to(t).numpy()) for v, t in values]
        if any(a.shape != shape for a in arrs):
            got = [str(a.shape) for a in arrs]
            raise Go2SimError(f"{what} shape {shape}, got {' and '.join([', '.join(got[:-1])] * (len(got) > 1) + got[-1:])}")
        self._call(entry, *(_ptr(a) for a in arrs), self._stream())

    def log(self, mask):
        """ep_log := the means of `ep` over the envs of `mask`, as the core reports its terms (the mean, over the envs of the last reset, of episode sum /
        episode seconds); kept while no env is reset.  Device arithmetic on [n_envs] values, no synchronisation."""
        if self.logs:
            m = mask.to(torch.float32)
            n = m.sum()
            self.ep_log = torch.where(n > 0, (self.ep * m).sum(-1) / n.clamp(min=1.0), self.ep_log)

    def episode_entries(self):
        return {}

    def curriculum_entries(self, level):
        return {}

    def state_schema(self, B):
        return self.schema_of(B)


class Go2Sim(Handle):
    """One simulator handle (n_envs environments on one device)."""

    def __init__(self, lib: Go2SimLib, model_blob: bytes, n_envs: int, device: int = 0, seed: int = 1):
        Handle.__init__(self, lib, "destroy")
        self.L = lib
        self.n_envs = n_envs
        self._blob = model_blob
        h = ctypes.c_void_p()
        rc = lib.fn("create")(model_blob, ctypes.c_size_t(len(model_blob)), ctypes.c_int(n_envs), ctypes.c_int(device),
                              ctypes.c_uint64(seed), ctypes.byref(h))
        lib.check(rc, "create")
        self.h = h

    # ---- scene level ---------------------------------------------------------------------------
    def _call(self, name, *args):
        self.L.check(self.L.fn(name)(self.h, *args), name)

    def scene_reset(self, stream=None):
        self._call("scene_reset", _ptr(stream))

    def substep(self, stream=None):
        self._call("substep", _ptr(stream))

    def scene_step(self, substeps=2, stream=None):
        self._call("scene_step", ctypes.c_int(substeps), _ptr(stream))

    def forward_kinematics(self, stream=None):
        self._call("forward_kinematics", _ptr(stream))

    def field_size(self, field):
        k, is_int = ctypes.c_int(), ctypes.c_int()
        self.L.check(self.L.fn("field_size")(ctypes.c_int(field), ctypes.byref(k), ctypes.byref(is_int)), "field_size")
        return k.value, bool(is_int.value)

    def get_field(self, field, dst, stream=None):
        self._call("get_field", ctypes.c_int(field), _ptr(dst), _ptr(stream))

    def set_field(self, field, src, stream=None):
        self._call("set_field", ctypes.c_int(field), _ptr(src), _ptr(stream))

    def field_ptr(self, field):
        p = ctypes.c_void_p()
        self._call("field_ptr", ctypes.c_int(field), ctypes.byref(p))
        return p.value

    def reset_caches(self, envs_idx=None, n_sel=0, stream=None):
        self._call("reset_caches", _ptr(envs_idx), ctypes.c_int(n_sel), _ptr(stream))

    def set_friction(self, mu, stream=None):
        self._call("set_friction", ctypes.c_float(mu), _ptr(stream))

    def set_terrain(self, hf_int16, horizontal_scale, vertical_scale, origin, stream=None):
        hf = np.ascontiguousarray(hf_int16, dtype=np.int16)
        org = np.ascontiguousarray(origin, dtype=np.float32)
        self._terrain_keepalive = (hf, org)
        self._call("set_terrain", _ptr(hf), ctypes.c_int(hf.shape[0]), ctypes.c_int(hf.shape[1]), ctypes.c_float(horizontal_scale),
                   ctypes.c_float(vertical_scale), _ptr(org), _ptr(stream))

    def _tiles_call(self, name, *args):
        """An entry of include/go2sim_tiles.h: the product library alone has it."""
        if not self.L.is_device or not hasattr(self.L.lib, name):
            raise Go2SimError(f"{name} is an entry of the HIP product library (include/go2sim_tiles.h); {self.L.path} does not have it")
        self.L.check(getattr(self.L.lib, name)(self.h, *args), name)

    def set_terrain_f32(self, hf_metres, horizontal_scale, origin, stream=None):
        """go2sim_set_terrain_f32: heights as float32 metres [rows][cols]"""
        hf = np.ascontiguousarray(hf_metres, dtype=np.float32)
        org = np.ascontiguousarray(origin, dtype=np.float32)
        assert hf.ndim == 2 and org.size == 3
        self._terrain_keepalive = (hf, org)
        self._tiles_call("go2sim_set_terrain_f32", _ptr(hf), ctypes.c_int(hf.shape[0]), ctypes.c_int(hf.shape[1]), ctypes.c_float(horizontal_scale),
                         _ptr(org), _ptr(stream))

    def tiles_query(self, xy, out, n=None, stream=None):
        """go2sim_tiles_query: xy float32 [n][2] -> out float32 [n], device memory"""
        self._tiles_call("go2sim_tiles_query", _ptr(xy), ctypes.c_int(len(xy) if n is None else n), _ptr(out), _ptr(stream))

    def set_dof_gains(self, dof, kp, kv, flo, fhi):
        self._call("set_dof_gains", ctypes.c_int(dof), ctypes.c_float(kp), ctypes.c_float(kv), ctypes.c_float(flo), ctypes.c_float(fhi))

    def check_errno(self, stream=None):
        v = ctypes.c_int()
        self._call("check_errno", ctypes.byref(v), _ptr(stream))
        return v.value

    # ---- env level -----------------------------------------------------------------------------
    def env_configure(self, fcfg: np.ndarray, icfg: np.ndarray):
        fcfg = np.ascontiguousarray(fcfg, dtype=np.float64)
        icfg = np.ascontiguousarray(icfg, dtype=np.int32)
        self._call("env_configure", _ptr(fcfg), ctypes.c_int(fcfg.size), _ptr(icfg), ctypes.c_int(icfg.size))

    def env_step(self, actions, obs, priv, rew, reset, timeout, stream=None):
        self._call("env_step", _ptr(actions), _ptr(obs), _ptr(priv), _ptr(rew), _ptr(reset), _ptr(timeout), _ptr(stream))

    def env_reset(self, stream=None):
        self._call("env_reset", _ptr(stream))

    def env_reset_idx(self, envs_idx, n=None, stream=None):
        self._call("env_reset_idx", _ptr(envs_idx), ctypes.c_int(len(envs_idx) if n is None else n), _ptr(stream))

    def env_respawn(self, envs_idx, pos, quat=None, clear_buffers=True, n=None, stream=None):
        self._call("env_respawn", _ptr(envs_idx), ctypes.c_int(len(envs_idx) if n is None else n), _ptr(pos), _ptr(quat),
                   ctypes.c_int(int(clear_buffers)), _ptr(stream))

    def env_lock_terrain_rows(self, lock=True, stream=None):
        self._call("env_lock_terrain_rows", ctypes.c_int(int(lock)), _ptr(stream))

    def env_set_terrain_rows(self, rows, stream=None):
        self._call("env_set_terrain_rows", _ptr(rows), _ptr(stream))

    def errno_poll_begin(self, stream=None):
        self._call("errno_poll_begin", _ptr(stream))

    def errno_poll_result(self):
        v, ready = ctypes.c_int(), ctypes.c_int()
        self._call("errno_poll_result", ctypes.byref(v), ctypes.byref(ready))
        return (v.value if ready.value else None)

    def errno_poll_wait(self):
        v = ctypes.c_int()
        self._call("errno_poll_wait", ctypes.byref(v))
        return v.value

    def graph_status(self):
        using, nfb = ctypes.c_int(), ctypes.c_int()
        self._call("graph_status", ctypes.byref(using), ctypes.byref(nfb))
        return bool(using.value), nfb.value

    def env_get(self, buf, dst, stream=None):
        self._call("env_get", ctypes.c_int(buf), _ptr(dst), _ptr(stream))

    def env_set_episode_length(self, ep, stream=None):
        self._call("env_set_episode_length", _ptr(ep), _ptr(stream))

    def env_set_commands(self, cmd, stream=None):
        self._call("env_set_commands", _ptr(cmd), _ptr(stream))

    def env_globals(self, stream=None):
        g = EnvGlobals()
        self._call("env_globals", ctypes.byref(g), _ptr(stream))
        return g

    def env_globals_ptr(self):
        p = ctypes.c_void_p()
        self._call("env_globals_ptr", ctypes.byref(p))
        return p.value

    def env_sync_counters(self, stream=None):
        out = (ctypes.c_double * 5)()
        self._call("env_sync_counters", out, _ptr(stream))
        return np.array(out[:], np.float64)

    def env_sync_apply(self, summed_counters, stream=None):
        c = (ctypes.c_double * 5)(*[float(v) for v in summed_counters])
        dr = (ctypes.c_double * 10)()
        self._call("env_sync_apply", c, dr, _ptr(stream))
        return np.array(dr[:], np.float64)

    def env_set_global_dr(self, dr10, stream=None):
        self._call("env_set_global_dr", (ctypes.c_double * 10)(*[float(v) for v in dr10]), _ptr(stream))

    def env_sync_counters_dev(self, counters5, stream=None):
        """float64[5] tensor / array in the library's memory space (device for the HIP library); stream-ordered, no synchronisation"""
        self._call("env_sync_counters_dev", _ptr(counters5), _ptr(stream))

    def env_sync_apply_dev(self, summed5, dr_out10, stream=None):
        self._call("env_sync_apply_dev", _ptr(summed5), _ptr(dr_out10), _ptr(stream))

    def env_set_global_dr_dev(self, dr10, stream=None):
        self._call("env_set_global_dr_dev", _ptr(dr10), _ptr(stream))

    def env_set_level(self, level, stream=None):
        self._call("env_set_level", ctypes.c_double(level), _ptr(stream))

    # ---- snapshots (include/go2sim_state.h; the product library alone has them) ------------------
    def _state_call(self, name, *args):
        if not self.L.is_device or not hasattr(self.L.lib, name):
            raise Go2SimError(f"{name} is an entry of the HIP product library (include/go2sim_state.h); {self.L.path} does not have it")
        return getattr(self.L.lib, name)(self.h, *args)

    def state_size(self):
        n = ctypes.c_size_t()
        self.L.check(self._state_call("go2sim_state_size", ctypes.byref(n)), "state_size")
        return n.value

    def state_save(self, dst, nbytes=None, stream=None):
        """go2sim_state_save into `dst`: a contiguous uint8 / int32 device tensor (or a raw device address with `nbytes`); stream-ordered"""
        n = dst.numel() * dst.element_size() if nbytes is None else int(nbytes)
        self.L.check(self._state_call("go2sim_state_save", _ptr(dst), ctypes.c_size_t(n), _ptr(stream)), "state_save")

    def state_load(self, src, nbytes=None, stream=None):
        """go2sim_state_load from `src`; -> the status (GO2SIM_E_OK, or GO2SIM_E_BADARG for a refused record: the handle is then untouched)"""
        n = src.numel() * src.element_size() if nbytes is None else int(nbytes)
        return self._state_call("go2sim_state_load", _ptr(src), ctypes.c_size_t(n), _ptr(stream))

    def enable_timing(self, enable=True):
        self._call("enable_timing", ctypes.c_int(int(enable)))

    def read_timing(self, reset=True):
        ms = (ctypes.c_float * 8)()
        cnt = (ctypes.c_int * 8)()
        self._call("read_timing", ms, cnt, ctypes.c_int(int(reset)))
        return list(ms), list(cnt)

    # ---- numpy convenience (host library only; used by tests) ----------------------------------
    def get_field_np(self, field):
        assert not self.L.is_device
        k, is_int = self.field_size(field)
        out = np.zeros((k, self.n_envs), dtype=np.int32 if is_int else np.float32)
        self.get_field(field, out)
        return out

    def set_field_np(self, field, arr):
        assert not self.L.is_device
        k, is_int = self.field_size(field)
        arr = np.ascontiguousarray(arr, dtype=np.int32 if is_int else np.float32).reshape(k, self.n_envs)
        self.set_field(field, arr)


# the words of a snapshot's header that go2sim_state_load compares, by name (include/go2sim_state.h): (first word, words, name)
STATE_HEADER_FIELDS = [(C["GO2SIM_STATE_W_MAGIC"], 1, "magic"), (C["GO2SIM_STATE_W_VERSION"], 1, "format version"), (C["GO2SIM_STATE_W_N_ENVS"], 1, "n_envs"),
                       (C["GO2SIM_STATE_W_NQ"], C["GO2SIM_STATE_W_SEED"] - C["GO2SIM_STATE_W_NQ"], "layout constants"), (C["GO2SIM_STATE_W_SEED"], 2, "seed"),
                       (C["GO2SIM_STATE_W_MODEL_DIGEST"], 2, "model digest"), (C["GO2SIM_STATE_W_CFG_DIGEST"], 2, "configuration digest"),
                       (C["GO2SIM_STATE_W_BYTES"], 2, "record size")]


def state_header_mismatch(words_a, words_b):
    """Names of the compared header fields in which two snapshot headers (sequences of uint32 words) differ."""
    return [name for w0, n, name in STATE_HEADER_FIELDS if [int(v) for v in words_a[w0:w0 + n]] != [int(v) for v in words_b[w0:w0 + n]]]


def state_record_parts(words):
    """[(name, first byte, bytes)] of the parts of a snapshot's body, from its header's words (include/go2sim_state.h): for telling where two records differ."""
    W = lambda name: int(words[C["GO2SIM_STATE_W_" + name]]) & 0xFFFFFFFF
    B = W("N_ENVS")
    sizes = [("globals", W("GLOB_BYTES")), ("accumulator", W("ACC_BYTES")), ("soa_float", 4 * W("F_CARRIED") * B), ("soa_int", 4 * W("I_CARRIED") * B),
             ("aos_float", 16 * W("AF_CARRIED") * B), ("aos_int", 16 * W("AI_CARRIED") * B)]
    at, parts = 4 * C["GO2SIM_STATE_HDR_WORDS"], []
    for name, n in sizes:
        parts.append((name, at, n))
        at += (n + 15) // 16 * 16
    return parts


def load_hip_lib():
    """The product library.  Fails loudly when the HIP extension has not been built."""
    return Go2SimLib(HIP_LIB, "go2sim_")


def load_cpu_oracle_lib(fast=False):
    """The CPU oracle.  Test infrastructure only (tests/, smoke(), bench cpu_baseline).  fast=False: the strict build (the reference's CPU /
    serial summation order); fast=True: the -DGO2SIM_FAST_ORDER build that mirrors the HIP product's reduction order bit for bit."""
    return Go2SimLib(CPU_LIB_FAST if fast else CPU_LIB, "go2sim_cpu_")
