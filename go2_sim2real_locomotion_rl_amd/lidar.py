"""LidarScan -- the LIDAR terrain scan of the reference's exteroceptive stair env (examples/locomotion/go2_env_stair_lidar.py) on the scan entry points
of the C ABI (include/go2sim_lidar.h): a noisy 5 x 3 body-frame height profile for the actor, a clean 9 x 5 one for the critic, and the wider rows.

    scan = LidarScan(env_cfg["lidar"], n_envs, hf_int16, horizontal_scale, vertical_scale, origin, seed=1)
    actor, critic = scan.scan(pos, quat, reset=reset_u8, level=level_f64)     # [n, 3] / [n, 4] device tensors -> [n, n_actor], [n, n_actor + n_critic]

``lidar_layout(cfg)`` reads the dictionary as the reference's ``LidarScanConfig`` (:304) does and needs no GPU; ``Go2Env`` drives the handle through
``LidarScan.step`` with the env's own pose buffers (one launch per env step)."""
import ctypes

import numpy as np
import torch

from .capi import C, EnvLaunch, Go2SimError, _ptr, check_layout_widths
from .configs import dr_schedule_params


class LidarCfg(ctypes.Structure):
    """go2sim_lidar_cfg_t"""
    DOUBLES = ("height_noise_std", "dropout_prob", "vertical_offset_std", "latency_prob", "full_blackout_prob", "height_clip", "height_scale",
               "dr_phase1_level", "dr_terrain_gate", "origin_x", "origin_y", "horizontal_scale", "vertical_scale")
    INTS = ("dr_schedule", "curriculum_enabled", "n_envs", "n_actor", "n_critic", "hf_rows", "hf_cols")
    _fields_ = [(n, ctypes.c_double) for n in DOUBLES] + [(n, ctypes.c_int) for n in INTS]


def lidar_enabled(env_cfg):
    """True when the cfg selects the LIDAR layout: a ``lidar`` block that is enabled (LidarScanConfig's default) on an enabled terrain."""
    lidar, terrain = env_cfg.get("lidar"), env_cfg.get("terrain")
    return bool(lidar) and bool(lidar.get("enabled", True)) and bool(terrain) and bool(terrain.get("enabled", False))


def lidar_layout(cfg):
    """LidarScanConfig.__init__ (go2_env_stair_lidar.py:326-391) as data: the two grids as float32 arrays in point order ix * ny + iy, their shapes,
    the noise constants, clip and scale.  The grids are formed by torch (linspace, meshgrid) as the reference forms them."""
    a, c, nz = cfg.get("actor_scan", {}), cfg.get("critic_scan", {}), cfg.get("noise", {})
    if "x_points" in a:
        ax, ay = torch.tensor(a["x_points"], dtype=torch.float32), torch.tensor(a["y_points"], dtype=torch.float32)
        actor_y = [float(v) for v in a["y_points"]]
    else:
        xr, yr = a.get("x_range", [0.0, 0.8]), a.get("y_range", [-0.15, 0.15])
        actor_y = [float(yr[0]), float(yr[1])]
        ax = torch.linspace(float(xr[0]), float(xr[1]), int(a.get("num_x", 5)))
        ay = torch.linspace(float(yr[0]), float(yr[1]), int(a.get("num_y", 3)))
    cxr, cyr = c.get("x_range", [-0.4, 0.8]), c.get("y_range", [-0.3, 0.3])
    cx = torch.linspace(float(cxr[0]), float(cxr[1]), int(c.get("num_x", 9)))
    cy = torch.linspace(float(cyr[0]), float(cyr[1]), int(c.get("num_y", 5)))

    def grid(x, y):
        gx, gy = torch.meshgrid(x, y, indexing="ij")
        return np.ascontiguousarray(torch.stack([gx.reshape(-1), gy.reshape(-1)]).numpy(), dtype=np.float32)

    return {"actor_xy": grid(ax, ay), "critic_xy": grid(cx, cy), "actor_shape": (len(ax), len(ay)), "critic_shape": (len(cx), len(cy)),
            "actor_y": actor_y, "critic_y": [float(cyr[0]), float(cyr[1])],     # the cfg's own y points or y range: what a mirror needs symmetric
            "height_noise_std": float(nz.get("height_noise_std", 0.02)), "dropout_prob": float(nz.get("dropout_prob", 0.15)),
            "full_blackout_prob": float(nz.get("full_blackout_prob", 0.05)), "latency_prob": float(nz.get("latency_prob", 0.1)),
            "vertical_offset_std": float(nz.get("vertical_offset_std", 0.01)),
            "height_clip": float(cfg.get("height_clip", 1.0)), "height_scale": float(cfg.get("height_scale", 1.0))}


def lidar_widths(env_cfg):
    """(n_in, num_obs, num_privileged_obs) of the LIDAR layout these cfgs give: the proprioceptive width, then go2_stair_train_lidar.py:342-360."""
    lay = lidar_layout(env_cfg["lidar"])
    n_in = 33 + int(env_cfg["num_actions"])
    n_actor, n_critic = lay["actor_xy"].shape[1], lay["critic_xy"].shape[1]
    return n_in, n_in + n_actor, n_in + n_actor + C["GO2SIM_LIDAR_PRIV_EXTRA"] + n_critic


def check_lidar_widths(env_cfg, obs_cfg):
    """The proprioceptive width n_in of a LIDAR cfg whose obs_cfg carries the widths its grids give; Go2SimError (naming both) otherwise."""
    return check_layout_widths("LIDAR", env_cfg, obs_cfg, lidar_widths(env_cfg))


def env_pose_ptrs(sim):
    """(pos, quat, component stride): the device addresses of a Go2Sim handle's base pose buffers (go2sim_lidar_env_pose)."""
    pos, quat, cs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_longlong()
    sim.L.check(sim.L.fn("lidar_env_pose")(sim.h, ctypes.byref(pos), ctypes.byref(quat), ctypes.byref(cs)), "lidar_env_pose")
    return pos.value, quat.value, cs.value


class LidarScan(EnvLaunch):
    NAME, STATE_FAMILY = "lidar", "stairs_lidar"

    def __init__(self, cfg, n_envs, hf_int16, horizontal_scale, vertical_scale, origin, *, seed=1, dr_schedule=None, curriculum_enabled=False, device=None):
        EnvLaunch.__init__(self, n_envs, device)
        if not cfg.get("enabled", True):
            raise Go2SimError("the lidar cfg is disabled: there is nothing to scan")
        self.layout = lay = lidar_layout(cfg)
        self.n_actor, self.n_critic = lay["actor_xy"].shape[1], lay["critic_xy"].shape[1]
        hf = np.ascontiguousarray(hf_int16, dtype=np.int16)
        c = LidarCfg()
        for name in ("height_noise_std", "dropout_prob", "vertical_offset_std", "latency_prob", "full_blackout_prob", "height_clip", "height_scale"):
            setattr(c, name, lay[name])
        c.dr_schedule, c.dr_phase1_level, c.dr_terrain_gate = dr_schedule_params(dr_schedule)
        c.curriculum_enabled = int(bool(curriculum_enabled))
        c.origin_x, c.origin_y = float(origin[0]), float(origin[1])
        c.horizontal_scale, c.vertical_scale = float(horizontal_scale), float(vertical_scale)
        c.n_envs, c.n_actor, c.n_critic, c.hf_rows, c.hf_cols = self.n_envs, self.n_actor, self.n_critic, hf.shape[0], hf.shape[1]
        self._create(c, _ptr(hf), _ptr(lay["actor_xy"]), _ptr(lay["critic_xy"]), ctypes.c_uint64(int(seed)))

    # ---- the step counter and the stored actor scan ---------------------------------------------------------------------------
    @property
    def step_count(self):
        v = ctypes.c_uint32()
        self._call("get_step", ctypes.byref(v))
        return v.value

    @step_count.setter
    def step_count(self, value):
        self._call("set_step", ctypes.c_uint32(int(value)))

    def stored_scan(self):
        """float32 [n_envs, n_actor] CPU tensor; waits for the stream."""
        return self._get_host("get_scan", (self.n_envs, self.n_actor), np.float32)[0]

    def set_stored_scan(self, scan):
        self._set_host("set_scan", "the stored scan has", (self.n_envs, self.n_actor), (scan, torch.float32))

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def step(self, pos, pos_strides, quat, quat_strides, reset, level, obs, priv, n_in, obs_out, priv_out):
        """go2sim_lidar_step with device tensors or raw device addresses; strides are (component, env) in elements."""
        self._step(ctypes.c_int(self.n_envs), _ptr(pos, True), ctypes.c_longlong(pos_strides[0]), ctypes.c_longlong(pos_strides[1]), _ptr(quat, True),
                   ctypes.c_longlong(quat_strides[0]), ctypes.c_longlong(quat_strides[1]), _ptr(reset), _ptr(level), _ptr(obs), _ptr(priv), ctypes.c_int(n_in),
                   _ptr(obs_out), _ptr(priv_out))

    def scan(self, pos, quat, reset=None, level=None):
        """The scans alone of poses given as [n, 3] / [n, 4] float32 device tensors: -> (actor [n, n_actor], actor | critic [n, n_actor + n_critic])."""
        pos, quat = pos.contiguous(), quat.contiguous()
        actor = torch.empty(self.n_envs, self.n_actor, device=self.device)
        both = torch.empty(self.n_envs, self.n_actor + self.n_critic, device=self.device)
        self.step(pos, (1, 3), quat, (1, 4), reset, level, None, None, 0, actor, both)
        return actor, both

    # ---- for Go2Env (capi.EnvLaunch) -------------------------------------------------------------------------------------------
    @staticmethod
    def inner_widths(env_cfg, obs_cfg):
        n_in = check_lidar_widths(env_cfg, obs_cfg)
        return n_in, n_in + C["GO2SIM_LIDAR_PRIV_EXTRA"]

    def launch(self, env, inner_obs, inner_priv):
        """The scans and the wider rows, straight into the env's fresh tensors; pose and level are read where the step left them."""
        pos, quat, cs = env._base_pose
        self.step(pos, (cs, 1), quat, (cs, 1), env.reset_buf, env._level_ptr, inner_obs, inner_priv, inner_obs.shape[1], env.obs_buf, env.privileged_obs_buf)

    @staticmethod
    def schema_of(B, n_points=None):
        return {"lidar_step": int, "lidar_scan": (torch.float32, (B, n_points))}

    def state_schema(self, B):
        return self.schema_of(B, self.n_actor)

    def state_dict(self):
        return {"lidar_step": int(self.step_count), "lidar_scan": self.stored_scan()}

    def load_state_dict(self, state):
        self.step_count = state["lidar_step"]
        self.set_stored_scan(state["lidar_scan"])
