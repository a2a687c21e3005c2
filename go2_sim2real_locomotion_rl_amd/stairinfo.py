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

from .capi import C, EnvLaunch, Go2SimError, _ptr, check_layout_widths
from .configs import dr_schedule_params


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
    return check_layout_widths("stair-info", env_cfg, obs_cfg, stair_info_widths(env_cfg))


def env_rows_ptr(sim):
    """The device address of a Go2Sim handle's terrain-row buffer, int32 [n_envs] (go2sim_stairinfo_env_rows)."""
    rows = ctypes.c_void_p()
    sim.L.check(sim.L.fn("stairinfo_env_rows")(sim.h, ctypes.byref(rows)), "stairinfo_env_rows")
    return rows.value


class StairInfo(EnvLaunch):
    NAME, STATE_FAMILY = "stairinfo", "stairs_info"

    def __init__(self, cfg, n_envs, hf_int16, horizontal_scale, vertical_scale, origin, step_heights_m, step_depths_m, *, seed=1, dr_schedule=None,
                 curriculum_enabled=False, device=None):
        EnvLaunch.__init__(self, n_envs, device)
        if not cfg.get("enabled", True):
            raise Go2SimError("the stair_info cfg is disabled: there is nothing to detect")
        self.layout = lay = stair_info_layout(cfg)
        # torch.tensor(list, dtype=float32), as go2_env_stair_lidar_2.py:470-473 forms the two tables
        self.row_heights = np.ascontiguousarray(np.asarray(step_heights_m, np.float64).astype(np.float32))
        self.row_depths = np.ascontiguousarray(np.asarray(step_depths_m, np.float64).astype(np.float32))
        if self.row_heights.ndim != 1 or self.row_heights.shape != self.row_depths.shape or not 1 <= len(self.row_heights) <= C["GO2SIM_STAIRINFO_MAX_ROWS"]:
            raise Go2SimError(f"the per-row step heights and depths must be two lists of one length, 1 .. {C['GO2SIM_STAIRINFO_MAX_ROWS']} rows, "
                              f"got {self.row_heights.shape} and {self.row_depths.shape}")
        self.n_rows = len(self.row_heights)
        self._sched, self._curriculum = dr_schedule_params(dr_schedule), bool(curriculum_enabled)
        hf = np.ascontiguousarray(hf_int16, dtype=np.int16)
        c = StairInfoCfg()
        for name in ("max_range", "threshold", "edge_dist_scale", "height_scale", "depth_scale", "direction_scale", "edge_noise_std", "height_noise_std",
                     "depth_noise_std", "direction_flip_prob", "latency_prob", "full_blackout_prob"):
            setattr(c, name, lay[name])
        c.dr_schedule, c.dr_phase1_level, c.dr_terrain_gate = self._sched
        c.curriculum_enabled = int(self._curriculum)
        c.origin_x, c.origin_y = float(origin[0]), float(origin[1])
        c.horizontal_scale, c.vertical_scale = float(horizontal_scale), float(vertical_scale)
        c.n_envs, c.n_samples, c.n_rows, c.hf_rows, c.hf_cols = self.n_envs, len(lay["sample_x"]), self.n_rows, hf.shape[0], hf.shape[1]
        self._create(c, _ptr(hf), _ptr(lay["sample_x"]), _ptr(self.row_heights), _ptr(self.row_depths), ctypes.c_uint64(int(seed)))

    # ---- the step counter and the stored actor rows ---------------------------------------------------------------------------
    @property
    def step_count(self):
        v = ctypes.c_uint32()
        self._call("get_step", ctypes.byref(v))
        return v.value

    @step_count.setter
    def step_count(self, value):
        self._call("set_step", ctypes.c_uint32(int(value)))

    def stored_rows(self):
        """float32 [n_envs, 4] CPU tensor; waits for the stream."""
        return self._get_host("get_state", (self.n_envs, NUM_STAIR_INFO), np.float32)[0]

    def set_stored_rows(self, rows4):
        self._set_host("set_state", "the stored rows have", (self.n_envs, NUM_STAIR_INFO), (rows4, torch.float32))

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def step(self, pos, pos_strides, quat, quat_strides, rows, reset, level, obs, priv, n_in, obs_out, priv_out):
        """go2sim_stairinfo_step with device tensors or raw device addresses; strides are (component, env) in elements."""
        self._step(ctypes.c_int(self.n_envs), _ptr(pos, True), ctypes.c_longlong(pos_strides[0]), ctypes.c_longlong(pos_strides[1]), _ptr(quat, True),
                   ctypes.c_longlong(quat_strides[0]), ctypes.c_longlong(quat_strides[1]), _ptr(rows), _ptr(reset), _ptr(level), _ptr(obs), _ptr(priv),
                   ctypes.c_int(n_in), _ptr(obs_out), _ptr(priv_out))

    def info(self, pos, quat, rows=None, reset=None, level=None):
        """The fours alone of poses given as [n, 3] / [n, 4] float32 device tensors and rows as an int32 [n] device tensor:
        -> (actor [n, 4], actor | clean [n, 8])."""
        pos, quat = pos.contiguous(), quat.contiguous()
        actor = torch.empty(self.n_envs, NUM_STAIR_INFO, device=self.device)
        both = torch.empty(self.n_envs, 2 * NUM_STAIR_INFO, device=self.device)
        self.step(pos, (1, 3), quat, (1, 4), rows, reset, level, None, None, 0, actor, both)
        return actor, both

    # ---- for Go2Env (capi.EnvLaunch) -------------------------------------------------------------------------------------------
    @staticmethod
    def inner_widths(env_cfg, obs_cfg):
        n_in = check_stair_info_widths(env_cfg, obs_cfg)
        return n_in, n_in + C["GO2SIM_STAIRINFO_PRIV_EXTRA"]

    def launch(self, env, inner_obs, inner_priv):
        """Both fours and the wider rows, straight into the env's fresh tensors; pose, terrain rows and level are read where the step left them."""
        pos, quat, cs = env._base_pose
        self.step(pos, (cs, 1), quat, (cs, 1), env._terrain_rows_ptr, env.reset_buf, env._level_ptr, inner_obs, inner_priv, inner_obs.shape[1], env.obs_buf,
                  env.privileged_obs_buf)

    def curriculum_entries(self, level):
        """go2_env_stair_lidar_2.py:1232: the DR level the noise scales with, _get_dr_level of the curriculum level (a 0-dim float64 device tensor)."""
        scheduled, p1, gate = self._sched
        t = level if self._curriculum else torch.ones_like(level)
        if scheduled:
            pr = ((t - gate) / max(1e-6, 1.0 - gate)).clamp(0.0, 1.0)
            t = torch.where(t < gate, torch.full_like(t, p1), p1 + (1.0 - p1) * pr)
        return {"stair_noise_level": t}

    @staticmethod
    def schema_of(B, _=None):
        return {"stairinfo_step": int, "stairinfo_rows": (torch.float32, (B, NUM_STAIR_INFO))}

    def state_dict(self):
        return {"stairinfo_step": int(self.step_count), "stairinfo_rows": self.stored_rows()}

    def load_state_dict(self, state):
        self.step_count = state["stairinfo_step"]
        self.set_stored_rows(state["stairinfo_rows"])
