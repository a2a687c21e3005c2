"""WellScan -- the scan handle of the stairwell env (examples/locomotion/go2_env_stair6_Omni.py) on the entry points of include/go2sim_wells.h: the
critic's 11 x 11 body-frame height scan, the wider privileged row and the alive reward term.

    scan = WellScan(env_cfg["terrain"], n_envs, hf_int16, horizontal_scale, vertical_scale, origin, n_levels=9, alive_scale=0.2)
    rows = scan.scan(pos, quat)                                  # [n, 3] / [n, 4] device tensors -> [n, nx * ny]

``well_widths(env_cfg)`` needs no GPU; ``Go2Env`` drives the handle through ``WellScan.step`` with the env's own pose buffers (one launch per env step)."""
import ctypes

import numpy as np
import torch

from .capi import C, Go2SimError, Handle, _ptr, load_hip_lib
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
    n_in, want_obs, want_priv = well_widths(env_cfg)
    num_actions, have = int(env_cfg["num_actions"]), (obs_cfg["num_obs"], obs_cfg.get("num_privileged_obs"))
    if num_actions not in ((16,) if env_cfg.get("pls_enable", False) else (16, 12)):
        raise Go2SimError(f"the stairwell layout has 16 actions (12 with pls_enable=False), got {num_actions}")
    if have != (want_obs, want_priv):
        raise Go2SimError(f"obs_cfg gives num_obs / num_privileged_obs = {have[0]} / {have[1]}, the stairwell cfg's scan grid gives {want_obs} / {want_priv}")
    return n_in


class WellScan(Handle):
    def __init__(self, terrain_cfg, n_envs, hf_int16, horizontal_scale, vertical_scale, origin, *, n_levels=1, alive_scale=0.0, dt=0.02, device=None):
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.nx, self.ny = check_well_scan_shape(terrain_cfg)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_envs, self.n_points = int(n_envs), self.nx * self.ny
        self.xs, self.ys = well_scan_axes(terrain_cfg)
        hf = np.ascontiguousarray(hf_int16, dtype=np.int16)
        c = WellsCfg()
        c.origin_x, c.origin_y = float(origin[0]), float(origin[1])
        c.horizontal_scale, c.vertical_scale = float(horizontal_scale), float(vertical_scale)
        c.alive_scale, c.dt = float(alive_scale), float(dt)
        c.n_envs, c.nx, c.ny, c.hf_rows, c.hf_cols, c.n_levels = self.n_envs, self.nx, self.ny, hf.shape[0], hf.shape[1], int(n_levels)
        self._L = load_hip_lib()
        Handle.__init__(self, self._L, "wells_destroy")
        h = ctypes.c_void_p()
        self._L.check(self._L.fn("wells_create")(ctypes.c_int(self.device.index or 0), ctypes.byref(c), hf.ctypes.data_as(ctypes.c_void_p),
                                                 self.xs.ctypes.data_as(ctypes.c_void_p), self.ys.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)), "wells_create")
        self.h = h
        ep, inc = ctypes.c_void_p(), ctypes.c_float()
        self._L.check(self._L.fn("wells_alive_ep")(self.h, ctypes.byref(ep), ctypes.byref(inc)), "wells_alive_ep")
        self.alive_ep_ptr, self.inc = ep.value, inc.value                  # the per-env record of the last finished episode; f32(alive_scale * dt)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the alive sums ---------------------------------------------------------------------------------------------------------
    def alive_state(self):
        """(alive sum float32 [n_envs], step count int32 [n_envs]) CPU tensors; waits for the stream."""
        s, k = np.zeros(self.n_envs, np.float32), np.zeros(self.n_envs, np.int32)
        self._L.check(self._L.fn("wells_get_alive")(self.h, s.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), self._stream()), "wells_get_alive")
        return torch.from_numpy(s), torch.from_numpy(k)

    def set_alive_state(self, alive_sum, steps):
        s = np.ascontiguousarray(torch.as_tensor(alive_sum).detach().cpu().to(torch.float32).numpy())
        k = np.ascontiguousarray(torch.as_tensor(steps).detach().cpu().to(torch.int32).numpy())
        if s.shape != (self.n_envs,) or k.shape != (self.n_envs,):
            raise Go2SimError(f"the alive state has shape {(self.n_envs,)}, got {s.shape} and {k.shape}")
        self._L.check(self._L.fn("wells_set_alive")(self.h, s.ctypes.data_as(ctypes.c_void_p), k.ctypes.data_as(ctypes.c_void_p), self._stream()), "wells_set_alive")

    def clear(self, envs_idx=None):
        """The episode hand-over without a step for ``envs_idx`` (int32 device tensor) or for every env: record the per-second value, zero sum and count."""
        n = 0 if envs_idx is None else envs_idx.numel()
        self._L.check(self._L.fn("wells_clear")(self.h, _ptr(envs_idx), ctypes.c_int(n), self._stream()), "wells_clear")

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def step(self, pos, pos_strides, quat, quat_strides, reset, priv, n_in, priv_out, rew):
        """go2sim_wells_step with device tensors or raw device addresses; strides are (component, env) in elements."""
        rc = self._L.fn("wells_step")(self.h, ctypes.c_int(self.n_envs), _ptr(pos, True), ctypes.c_longlong(pos_strides[0]), ctypes.c_longlong(pos_strides[1]),
                                      _ptr(quat, True), ctypes.c_longlong(quat_strides[0]), ctypes.c_longlong(quat_strides[1]), _ptr(reset), _ptr(priv),
                                      ctypes.c_int(n_in), _ptr(priv_out), _ptr(rew), self._stream())
        self._L.check(rc, "wells_step")

    def scan(self, pos, quat):
        """The scan alone of poses given as [n, 3] / [n, 4] float32 device tensors -> [n, nx * ny]."""
        pos, quat = pos.contiguous(), quat.contiguous()
        out = torch.empty(self.n_envs, self.n_points, device=self.device)
        self.step(pos, (1, 3), quat, (1, 4), None, None, 0, out, None)
        return out
