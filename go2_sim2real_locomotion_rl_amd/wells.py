"""WellScan -- the scan handle of the stairwell env (examples/locomotion/go2_env_stair6_Omni.py) on the entry points of include/go2sim_wells.h: the
critic's 11 x 11 body-frame height scan, the wider privileged row and the alive reward term.

    scan = WellScan(env_cfg["terrain"], n_envs, hf_int16, horizontal_scale, vertical_scale, origin, n_levels=9, alive_scale=0.2)
    rows = scan.scan(pos, quat)                                  # [n, 3] / [n, 4] device tensors -> [n, nx * ny]

``well_widths(env_cfg)`` needs no GPU; ``Go2Env`` drives the handle through ``WellScan.step`` with the env's own pose buffers (one launch per env step)."""
import ctypes

import numpy as np
import torch

from .capi import C, EnvLaunch, Go2SimError, _as_device_tensor, _ptr, check_layout_widths
from .terrain_wells import well_scan_axes


class WellsCfg(ctypes.Structure):
    """go2sim_wells_cfg_t"""
    DOUBLES = ("origin_x", "origin_y", "horizontal_scale", "vertical_scale", "alive_scale", "dt")
    INTS = ("n_envs", "nx", "ny", "hf_rows", "hf_cols", "n_levels")
    _fields_ = [(n, ctypes.c_double) for n in DOUBLES] + [(n, ctypes.c_int) for n in INTS]


def well_scan_shape(terrain_cfg):
    hs = terrain_cfg.get("height_scan", {})
    return int(hs.get("num_x", 11)), int(hs.get("num_y", 11))


def check_well_scan_shape(terrain_cfg):
    nx, ny = well_scan_shape(terrain_cfg)
    top = C["GO2SIM_WELLS_AXIS_MAX"]
    if not (1 <= nx <= top and 1 <= ny <= top):
        raise Go2SimError(f"the stairwell height scan has at most {top} points per axis, got {nx} x {ny}")
    return nx, ny


def well_widths(env_cfg):
    """(n_in, num_obs, num_privileged_obs) of the stairwell layout: the proprioceptive width, then go2_stair_train6_Omni.py: n_in + 55 + 1 + nx ny."""
    nx, ny = well_scan_shape(env_cfg["terrain"])
    n_in = 33 + int(env_cfg["num_actions"])
    return n_in, n_in, n_in + C["GO2SIM_WELLS_PRIV_EXTRA"] + nx * ny


def check_well_widths(env_cfg, obs_cfg):
    """The proprioceptive width n_in of a stairwell cfg whose obs_cfg carries the widths its scan grid gives; Go2SimError (naming both) otherwise."""
    check_well_scan_shape(env_cfg["terrain"])
    return check_layout_widths("stairwell", env_cfg, obs_cfg, well_widths(env_cfg))


class WellScan(EnvLaunch):
    NAME, STATE_FAMILY, WIDENS_OBS = "wells", "stairwell", False         # the actor row is the step kernels' own

    def __init__(self, terrain_cfg, n_envs, hf_int16, horizontal_scale, vertical_scale, origin, *, n_levels=1, alive_scale=0.0, dt=0.02, device=None):
        """``alive_scale=None``: a reward_cfg without the `alive` key -- Go2Env hands no reward over and reports no rew_alive."""
        EnvLaunch.__init__(self, n_envs, device)
        self.nx, self.ny = check_well_scan_shape(terrain_cfg)
        self.n_points, self.logs = self.nx * self.ny, alive_scale is not None
        self.xs, self.ys = well_scan_axes(terrain_cfg)
        hf = np.ascontiguousarray(hf_int16, dtype=np.int16)
        c = WellsCfg()
        c.origin_x, c.origin_y = float(origin[0]), float(origin[1])
        c.horizontal_scale, c.vertical_scale = float(horizontal_scale), float(vertical_scale)
        c.alive_scale, c.dt = float(alive_scale or 0.0), float(dt)
        c.n_envs, c.nx, c.ny, c.hf_rows, c.hf_cols, c.n_levels = self.n_envs, self.nx, self.ny, hf.shape[0], hf.shape[1], int(n_levels)
        self._create(c, _ptr(hf), _ptr(self.xs), _ptr(self.ys))
        ep, inc = ctypes.c_void_p(), ctypes.c_float()
        self._call("alive_ep", ctypes.byref(ep), ctypes.byref(inc))
        self.alive_ep_ptr, self.inc = ep.value, inc.value                  # the per-env record of the last finished episode; f32(alive_scale * dt)
        self.ep = _as_device_tensor(ep.value, (self.n_envs,), torch.float32, self.device)
        self.ep_log = torch.zeros((), device=self.device)

    # ---- the alive sums ---------------------------------------------------------------------------------------------------------
    def alive_state(self):
        """(alive sum float32 [n_envs], step count int32 [n_envs]) CPU tensors; waits for the stream."""
        return self._get_host("get_alive", (self.n_envs,), np.float32, np.int32)

    def set_alive_state(self, alive_sum, steps):
        self._set_host("set_alive", "the alive state has", (self.n_envs,), (alive_sum, torch.float32), (steps, torch.int32))

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def step(self, pos, pos_strides, quat, quat_strides, reset, priv, n_in, priv_out, rew):
        """go2sim_wells_step with device tensors or raw device addresses; strides are (component, env) in elements."""
        self._step(ctypes.c_int(self.n_envs), _ptr(pos, True), ctypes.c_longlong(pos_strides[0]), ctypes.c_longlong(pos_strides[1]), _ptr(quat, True),
                   ctypes.c_longlong(quat_strides[0]), ctypes.c_longlong(quat_strides[1]), _ptr(reset), _ptr(priv), ctypes.c_int(n_in), _ptr(priv_out),
                   _ptr(rew))

    def scan(self, pos, quat):
        """The scan alone of poses given as [n, 3] / [n, 4] float32 device tensors -> [n, nx * ny]."""
        pos, quat = pos.contiguous(), quat.contiguous()
        out = torch.empty(self.n_envs, self.n_points, device=self.device)
        self.step(pos, (1, 3), quat, (1, 4), None, None, 0, out, None)
        return out

    # ---- for Go2Env (capi.EnvLaunch) -------------------------------------------------------------------------------------------
    @staticmethod
    def inner_widths(env_cfg, obs_cfg):
        n_in = check_well_widths(env_cfg, obs_cfg)
        return n_in, n_in + C["GO2SIM_WELLS_PRIV_EXTRA"]

    def launch(self, env, inner_obs, inner_priv):
        """The 11 x 11 scan into the env's wider privileged row, and the alive term onto its reward."""
        pos, quat, cs = env._base_pose
        self.step(pos, (cs, 1), quat, (cs, 1), env.reset_buf, inner_priv, env.num_obs, env.privileged_obs_buf, env.rew_buf if self.logs else None)

    def episode_entries(self):
        return {"rew_alive": self.ep_log} if self.logs else {}

    @staticmethod
    def schema_of(B, _=None):
        f32 = torch.float32
        return {"wells_alive_sum": (f32, (B,)), "wells_alive_steps": (torch.int32, (B,)), "wells_alive_ep": (f32, (B,)), "wells_alive_log": (f32, ())}

    def state_dict(self):
        alive_sum, alive_steps = self.alive_state()
        return {"wells_alive_sum": alive_sum, "wells_alive_steps": alive_steps, "wells_alive_ep": self.ep.cpu().clone(), "wells_alive_log": self.ep_log.cpu().clone()}

    def load_state_dict(self, state):
        self.set_alive_state(state["wells_alive_sum"], state["wells_alive_steps"])
        self.ep.copy_(state["wells_alive_ep"])
        self.ep_log = state["wells_alive_log"].to(self.device)
