"""ContactTerms -- the two reward terms on the links' net contact forces, on the entry points of include/go2sim_cterms.h: `body_contact` of
examples/locomotion/go2_env_stair_lidar_2.py (listed links whose contact force exceeds a threshold; the script lists the two front thighs) and
`stumble` of examples/locomotion/go2_env_terrain.py (the force above a threshold over every link that is not a foot).

    terms = ContactTerms(n_envs, body_links=resolve_body_links(["FR_thigh", "FL_thigh"]), body_contact_scale=-2.0)
    terms.step(cf, (n_envs, 3 * n_envs, 1), reset, rew, count)        # the pool's SoA contact-force field; one launch

``resolve_body_links``, ``non_foot_links`` and ``contact_term_scales`` need no GPU; ``Go2Env`` drives the handle with the env's own
GO2SIM_F_CONTACT_FORCE field (one launch per env step, after the step's own)."""
import ctypes

import numpy as np
import torch

from .capi import C, EnvLaunch, Go2SimError, _as_device_tensor, _ptr
from .configs import CONTACT_TERM_NAMES                              # ("body_contact", "stumble"): the order the launch applies them in
from .model_blob import load_model_json

DEFAULT_BODY_CONTACT_NAMES = ("FR_thigh", "FL_thigh")                # go2_env_stair_lidar_2.py:1105
FOOT_LINK_NAMES = ("FL_calf", "FR_calf", "RL_calf", "RR_calf")       # the feet are the calf links


class CtermsCfg(ctypes.Structure):
    """go2sim_cterms_cfg_t"""
    DOUBLES = ("dt", "body_contact_scale", "stumble_scale", "body_contact_threshold", "stumble_threshold")
    INTS = ("n_envs", "n_links")
    MASKS = ("body_mask", "stumble_mask")
    _fields_ = [(n, ctypes.c_double) for n in DOUBLES] + [(n, ctypes.c_int) for n in INTS] + [(n, ctypes.c_uint32) for n in MASKS]


def _link_ids(model=None):
    model = load_model_json() if model is None else model
    return {l["name"]: i for i, l in enumerate(model["links"])}


def resolve_body_links(names=DEFAULT_BODY_CONTACT_NAMES, model=None):
    """Model link indices (0 is the ground) of env_cfg["body_contact_names"].  A name that is no link of the model is refused -- the reference prints
    a warning and goes on without the term."""
    ids = _link_ids(model)
    unknown = [n for n in names if n not in ids or ids[n] == 0]
    if unknown:
        raise Go2SimError(f"body_contact_names {unknown} are no links of the robot; its links are {[n for n, i in ids.items() if i > 0]}")
    return [ids[n] for n in names]


def non_foot_links(model=None):
    """Every robot link that is not a foot (nine on Go2): the links `stumble` sums over."""
    ids = _link_ids(model)
    return [i for n, i in ids.items() if i > 0 and n not in FOOT_LINK_NAMES]


def link_mask(links):
    m = 0
    for l in links:
        if not 0 <= int(l) < C["GO2SIM_CTERMS_LINKS_MAX"]:
            raise Go2SimError(f"a contact-term link index lies in [0, {C['GO2SIM_CTERMS_LINKS_MAX']}), got {l}")
        m |= 1 << int(l)
    return m


def contact_term_scales(reward_cfg):
    """(body_contact scale, stumble scale) of a reward_cfg; 0.0 for an absent key."""
    scales = reward_cfg.get("reward_scales", {})
    return tuple(float(scales.get(n, 0.0)) for n in CONTACT_TERM_NAMES)


class ContactTerms(EnvLaunch):
    NAME, logs = "cterms", True

    def __init__(self, n_envs, *, body_links=(), stumble_links=None, body_contact_scale=0.0, stumble_scale=0.0, body_contact_threshold=1.0,
                 stumble_threshold=5.0, n_links=None, dt=0.02, device=None, body_mask=None, stumble_mask=None, report=CONTACT_TERM_NAMES, count_out=None):
        """``report``: the terms whose reward_cfg key exists, the ones episode_entries() lists (zero for a zero scale); ``count_out``: where launch() leaves
        the per-env count of body links in contact (Go2Env.body_contact_count)."""
        EnvLaunch.__init__(self, n_envs, device)
        self.n_links = int(C["GO2SIM_NL"] if n_links is None else n_links)
        c = CtermsCfg()
        c.dt, c.body_contact_scale, c.stumble_scale = float(dt), float(body_contact_scale), float(stumble_scale)
        c.body_contact_threshold, c.stumble_threshold = float(body_contact_threshold), float(stumble_threshold)
        c.n_envs, c.n_links = self.n_envs, self.n_links
        c.body_mask = link_mask(body_links) if body_mask is None else int(body_mask)
        c.stumble_mask = (link_mask(non_foot_links() if stumble_links is None else stumble_links)) if stumble_mask is None else int(stumble_mask)
        self.body_mask, self.stumble_mask = int(c.body_mask), int(c.stumble_mask)
        self._create(c)
        ep_b, ep_s, inc_b, inc_s = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float(), ctypes.c_float()
        self._call("ep", ctypes.byref(ep_b), ctypes.byref(ep_s), ctypes.byref(inc_b), ctypes.byref(inc_s))
        self.ep_ptrs = (ep_b.value, ep_s.value)                        # per-env records of the last finished episode, body_contact then stumble
        if ep_s.value != ep_b.value + 4 * self.n_envs:                 # the library keeps them as one [2][n_envs] array: both are reduced in one view
            raise Go2SimError("go2sim_cterms_ep: the two records are not adjacent")
        self.incs = (inc_b.value, inc_s.value)                         # f32(scale * dt) of each
        self.active = (float(body_contact_scale) != 0.0, float(stumble_scale) != 0.0)
        self.ep = _as_device_tensor(ep_b.value, (2, self.n_envs), torch.float32, self.device)
        self.ep_log = torch.zeros(2, device=self.device)              # the logged means, body_contact then stumble
        self.count = torch.zeros(self.n_envs, device=self.device) if count_out is None else count_out
        self._report, self._zero = tuple(report), torch.zeros((), device=self.device)

    # ---- the sums --------------------------------------------------------------------------------------------------------------
    def state(self):
        """(sum float32 [2, n_envs], steps int32 [2, n_envs], ep float32 [2, n_envs]) CPU tensors, body_contact then stumble; waits for the stream."""
        return self._get_host("get_state", (2, self.n_envs), np.float32, np.int32, np.float32)

    def set_state(self, sums, steps, ep):
        self._set_host("set_state", "the contact terms' state has", (2, self.n_envs), (sums, torch.float32), (steps, torch.int32), (ep, torch.float32))

    # ---- the step ----------------------------------------------------------------------------------------------------------
    def step(self, cf, strides, reset, rew, count_out):
        """go2sim_cterms_step with device tensors or raw device addresses; strides are (component, link, env) in elements."""
        self._step(ctypes.c_int(self.n_envs), _ptr(cf, True), ctypes.c_longlong(strides[0]), ctypes.c_longlong(strides[1]),
                   ctypes.c_longlong(strides[2]), _ptr(reset), _ptr(rew), _ptr(count_out))

    # ---- for Go2Env (capi.EnvLaunch) -------------------------------------------------------------------------------------------
    def launch(self, env, inner_obs, inner_priv):
        """Both terms onto the env's reward, from the links' contact forces where the solve left them (SoA [link * 3 + comp][n_envs])."""
        n = self.n_envs
        self.step(env._contact_force_ptr, (n, 3 * n, 1), env.reset_buf, env.rew_buf, self.count)

    def episode_entries(self):
        return {"rew_" + name: self.ep_log[t] if self.active[t] else self._zero for t, name in enumerate(CONTACT_TERM_NAMES) if name in self._report}

    @staticmethod
    def schema_of(B, _=None):                                                    # body_contact, then stumble (include/go2sim_cterms.h)
        f32 = torch.float32
        return {"cterms_sum": (f32, (2, B)), "cterms_steps": (torch.int32, (2, B)), "cterms_ep": (f32, (2, B)), "cterms_log": (f32, (2,)), "cterms_count": (f32, (B,))}

    def state_dict(self):
        sums, steps, ep = self.state()
        return {"cterms_sum": sums, "cterms_steps": steps, "cterms_ep": ep, "cterms_log": self.ep_log.cpu().clone(), "cterms_count": self.count.cpu().clone()}

    def load_state_dict(self, state):
        self.set_state(state["cterms_sum"], state["cterms_steps"], state["cterms_ep"])
        self.ep_log = state["cterms_log"].to(self.device)
        self.count.copy_(state["cterms_count"])
