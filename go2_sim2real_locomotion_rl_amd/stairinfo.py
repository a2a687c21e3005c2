"""StairInfo -- the four-value stair info of the reference's later exteroceptive stair env (examples/locomotion/go2_env_stair_lidar_2.py) on the
entry points of include/go2sim_stairinfo.h: distance to the next height change ahead, riser height, tread depth and direction; a degraded copy for the
actor, the clean four for the critic, and the wider rows.

    info = StairInfo(env_cfg["stair_info"], n_envs, hf_int16, horizontal_scale, vertical_scale, origin, step_heights_m, step_depths_m, seed=1)
    actor, both = info.info(pos, quat, rows=rows_i32, reset=reset_u8, level=level_f64)     # [n, 3] / [n, 4] device tensors -> [n, 4], [n, 8]

``stair_info_layout(cfg)`` reads the dictionary as the reference's ``StairInfoConfig`` (:331) does and needs no GPU; ``Go2Env`` drives the handle
through ``StairInfo.step`` with the env's own pose and terrain-row buffers (one launch per env step)."""
import ctypes
import math

import numpy as np
import torch

from .capi import C, Go2SimError, Handle, _ptr, load_hip_lib


class StairInfoCfg(ctypes.Structure):
    """go2sim_stairinfo_cfg_t"""
    DOUBLES = ("max_range", "threshold", "edge_dist_scale", "height_scale", "depth_scale", "direction_scale", "edge_noise_std", "height_noise_std",
               "depth_noise_std", "direction_flip_prob", "latency_prob", "full_blackout_prob", "dr_phase1_level", "dr_terrain_gate", "origin_x",
               "origin_y", "horizontal_scale", "vertical_scale")
    INTS = ("dr_schedule", "curriculum_enabled", "n_envs", "n_samples", "n_rows", "hf_rows", "hf_cols")
    _fields_ = [(n, ctypes.c_double) for n in DOUBLES] + [(n, ctypes.c_int) for n in INTS]


NUM_STAIR_INFO = C["GO2SIM_STAIRINFO_N"]


def stair_info_enabled(env_cfg):
    """True when the cfg selects the stair-info layout: a ``stair_info`` block that is enabled (StairInfoConfig's default) on an enabled terrain."""
    info, terrain = env_cfg.get("stair_info"), env_cfg.get("terrain")
    return bool(info) and bool(info.get("enabled", True)) and bool(terrain) and bool(terrain.get("enabled", False))


def check_one_exteroceptive_layout(env_cfg):
    """Go2SimError for a cfg that enables both `lidar` and `stair_info`: the reference has one env file per layout."""
    from .lidar import lidar_enabled

    if stair_info_enabled(env_cfg) and lidar_enabled(env_cfg):
        raise Go2SimError("env_cfg enables both `lidar` and `stair_info`: an env has one exteroceptive layout (go2_env_stair_lidar.py or "
                          "go2_env_stair_lidar_2.py)")


def stair_info_layout(cfg):
    """StairInfoConfig.__init__ (go2_env_stair_lidar_2.py:347-377) as data: the samples as the float32 array torch.linspace forms, the detector's
    constants, the four scales and the noise constants.  Go2SimError for what the library refuses: fewer than 2 or more than 64 samples, a negative
    or non-finite range or threshold."""
    e, nz = cfg.get("edge_detection", {}), cfg.get("noise", {})
    max_range, threshold, n = float(e.get("max_range", 0.27)), float(e.get("threshold", 0.02)), int(e.get("num_samples", 14))
    if not 2 <= n <= C["GO2SIM_STAIRINFO_MAX_SAMPLES"]:
        raise Go2SimError(f"stair_info edge_detection num_samples must be 2 .. {C['GO2SIM_STAIRINFO_MAX_SAMPLES']}, got {n}")
    for name, v in (("max_range", max_range), ("threshold", threshold)):
        if not (math.isfinite(v) and v >= 0.0):
            raise Go2SimError(f"stair_info edge_detection {name} must be finite and >= 0, got {v}")
    return {"sample_x": np.ascontiguousarray(torch.linspace(0.0, max_range, n).numpy(), dtype=np.float32), "max_range": max_range, "threshold": threshold,
            "edge_dist_scale": float(cfg.get("edge_dist_scale", 1.0 / 0.27)), "height_scale": float(cfg.get("height_scale", 1.0 / 0.20)),
            "depth_scale": float(cfg.get("depth_scale", 1.0 / 0.30)), "direction_scale": float(cfg.get("direction_scale", 1.0)),
            "edge_noise_std": float(nz.get("edge_noise_std", 0.04)), "height_noise_std": float(nz.get("height_noise_std", 0.01)),
            "depth_noise_std": float(nz.get("depth_noise_std", 0.01)), "direction_flip_prob": float(nz.get("direction_flip_prob", 0.03)),
            "full_blackout_prob": float(nz.get("full_blackout_prob", 0.05)), "latency_prob": float(nz.get("latency_prob", 0.10))}


def stair_info_widths(env_cfg):
    """(n_in, num_obs, num_privileged_obs) of the stair-info layout: the proprioceptive width, then go2_stair_train_lidar_2.py:318-327."""
    n_in = 33 + int(env_cfg["num_actions"])
    return n_in, n_in + NUM_STAIR_INFO, n_in + NUM_STAIR_INFO + C["GO2SIM_STAIRINFO_PRIV_EXTRA"] + NUM_STAIR_INFO


def check_stair_info_widths(env_cfg, obs_cfg):
    """The proprioceptive width n_in of a stair-info cfg whose obs_cfg carries the layout's widths; Go2SimError (naming both pairs) otherwise."""
    n_in, want_obs, want_priv = stair_info_widths(env_cfg)
    num_actions, have = int(env_cfg["num_actions"]), (obs_cfg["num_obs"], obs_cfg.get("num_privileged_obs"))
    if num_actions not in ((16,) if env_cfg.get("pls_enable", False) else (16, 12)):
        raise Go2SimError(f"the stair-info layout has 16 actions (12 with pls_enable=False), got {num_actions}")
    if have != (want_obs, want_priv):
        raise Go2SimError(f"obs_cfg gives num_obs / num_privileged_obs = {have[0]} / {have[1]}, the stair_info layout gives {want_obs} / {want_priv}")
    return n_in


def env_rows_ptr(sim):
    """The device address of a Go2Sim handle's terrain-row buffer, int32 [n_envs] (go2sim_stairinfo_env_rows)."""
    rows = ctypes.c_void_p()
    sim.L.check(sim.L.fn("stairinfo_env_rows")(sim.h, ctypes.byref(rows)), "stairinfo_env_rows")
    return rows.value


class StairInfo(Handle):
    def __init__(self, cfg, n_envs, hf_int16, horizontal_scale, vertical_scale, origin, step_heights_m, step_depths_m, *, seed=1, dr_schedule=None,
                 curriculum_enabled=False, device=None):
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        if not cfg.get("enabled", True):
            raise Go2SimError("the stair_info cfg is disabled: there is nothing to detect")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_envs = int(n_envs)
        self.layout = lay = stair_info_layout(cfg)
        # torch.tensor(list, dtype=float32), as go2_env_stair_lidar_2.py:470-473 forms the two tables
        self.row_heights = np.ascontiguousarray(np.asarray(step_heights_m, np.float64).astype(np.float32))
        self.row_depths = np.ascontiguousarray(np.asarray(step_depths_m, np.float64).astype(np.float32))
        if self.row_heights.ndim != 1 or self.row_heights.shape != self.row_depths.shape or not 1 <= len(self.row_heights) <= C["GO2SIM_STAIRINFO_MAX_ROWS"]:
            raise Go2SimError(f"the per-row step heights and depths must be two lists of one length, 1 .. {C['GO2SIM_STAIRINFO_MAX_ROWS']} rows, "
                              f"got {self.row_heights.shape} and {self.row_depths.shape}")
        self.n_rows = len(self.row_heights)
        hf = np.ascontiguousarray(hf_int16, dtype=np.int16)
        c = StairInfoCfg()
        for name in ("max_range", "threshold", "edge_dist_scale", "height_scale", "depth_scale", "direction_scale", "edge_noise_std", "height_noise_std",
                     "depth_noise_std", "direction_flip_prob", "latency_prob", "full_blackout_prob"):
            setattr(c, name, lay[name])
        c.dr_schedule = int(dr_schedule is not None)
        if dr_schedule is not None:                                         # the defaults of flatten_walk_cfg
            c.dr_phase1_level, c.dr_terrain_gate = float(dr_schedule.get("phase1_level", 0.15)), float(dr_schedule.get("terrain_gate", 0.50))
        c.curriculum_enabled = int(bool(curriculum_enabled))
        c.origin_x, c.origin_y = float(origin[0]), float(origin[1])
        c.horizontal_scale, c.vertical_scale = float(horizontal_scale), float(vertical_scale)
        c.n_envs, c.n_samples, c.n_rows, c.hf_rows, c.hf_cols = self.n_envs, len(lay["sample_x"]), self.n_rows, hf.shape[0], hf.shape[1]
        self._L = load_hip_lib()
        Handle.__init__(self, self._L, "stairinfo_destroy")
        h = ctypes.c_void_p()
        self._L.check(self._L.fn("stairinfo_create")(ctypes.c_int(self.device.index or 0), ctypes.byref(c), hf.ctypes.data_as(ctypes.c_void_p),
                                                     lay["sample_x"].ctypes.data_as(ctypes.c_void_p), self.row_heights.ctypes.data_as(ctypes.c_void_p),
                                                     self.row_depths.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(int(seed)), ctypes.byref(h)),
                      "stairinfo_create")
        self.h = h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the step counter and the stored actor rows ---------------------------------------------------------------------------
    @property
    def step_count(self):
        v = ctypes.c_uint32()
        self._L.check(self._L.fn("stairinfo_get_step")(self.h, ctypes.byref(v)), "stairinfo_get_step")
        return v.value

    @step_count.setter
    def step_count(self, value):
        self._L.check(self._L.fn("stairinfo_set_step")(self.h, ctypes.c_uint32(int(value))), "stairinfo_set_step")

    def stored_rows(self):
        """float32 [n_envs, 4] CPU tensor; waits for the stream."""
        out = np.zeros((self.n_envs, NUM_STAIR_INFO), np.float32)
        self._L.check(self._L.fn("stairinfo_get_state")(self.h, out.ctypes.data_as(ctypes.c_void_p), self._stream()), "stairinfo_get_state")
        return torch.from_numpy(out)

    def set_stored_rows(self, rows4):
        a = np.ascontiguousarray(torch.as_tensor(rows4).detach().cpu().to(torch.float32).numpy())
        if a.shape != (self.n_envs, NUM_STAIR_INFO):
            raise Go2SimError(f"the stored rows have shape {(self.n_envs, NUM_STAIR_INFO)}, got {a.shape}")
        self._L.check(self._L.fn("stairinfo_set_state")(self.h, a.ctypes.data_as(ctypes.c_void_p), self._stream()), "stairinfo_set_state")

    def clear(self, envs_idx=None):
        """Stored actor row := 0 for ``envs_idx`` (int32 device tensor) or for every env."""
        n = 0 if envs_idx is None else envs_idx.numel()
        self._L.check(self._L.fn("stairinfo_clear")(self.h, _ptr(envs_idx), ctypes.c_int(n), self._stream()), "stairinfo_clear")

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def step(self, pos, pos_strides, quat, quat_strides, rows, reset, level, obs, priv, n_in, obs_out, priv_out):
        """go2sim_stairinfo_step with device tensors or raw device addresses; strides are (component, env) in elements."""
        rc = self._L.fn("stairinfo_step")(self.h, ctypes.c_int(self.n_envs), _ptr(pos, True), ctypes.c_longlong(pos_strides[0]), ctypes.c_longlong(pos_strides[1]),
                                          _ptr(quat, True), ctypes.c_longlong(quat_strides[0]), ctypes.c_longlong(quat_strides[1]), _ptr(rows), _ptr(reset), _ptr(level),
                                          _ptr(obs), _ptr(priv), ctypes.c_int(n_in), _ptr(obs_out), _ptr(priv_out), self._stream())
        self._L.check(rc, "stairinfo_step")

    def info(self, pos, quat, rows=None, reset=None, level=None):
        """The fours alone of poses given as [n, 3] / [n, 4] float32 device tensors and rows as an int32 [n] device tensor:
        -> (actor [n, 4], actor | clean [n, 8])."""
        pos, quat = pos.contiguous(), quat.contiguous()
        actor = torch.empty(self.n_envs, NUM_STAIR_INFO, device=self.device)
        both = torch.empty(self.n_envs, 2 * NUM_STAIR_INFO, device=self.device)
        self.step(pos, (1, 3), quat, (1, 4), rows, reset, level, None, None, 0, actor, both)
        return actor, both
