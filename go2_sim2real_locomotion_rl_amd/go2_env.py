"""Go2Env -- host-side mirror of the reference's walk environment class on top of the go2sim C ABI.

Same constructor, methods, return values and attribute set as
``examples/locomotion/final/go2_env_walk.py`` (class Go2Env :154; step :985-1109; get_observations :1145;
get_privileged_observations :1151; reset :1242) so that ``rsl_rl.OnPolicyRunner`` and the reference's
train / eval scripts can use it unchanged:

    env = Go2Env(num_envs, env_cfg, obs_cfg, reward_cfg, command_cfg)
    obs, extras = env.get_observations()
    obs, rew, reset, extras = env.step(actions)         # all torch tensors on env.device

Differences that are deliberate (DESIGN.md "boundary"):
  * the whole step runs inside libgo2sim.so (HIP, gfx950); there is no per-call torch arithmetic and no
    host synchronisation: the curriculum state machine and the "global" domain randomisation live on the device;
  * ``extras["episode"]`` / ``extras["curriculum"]`` / ``extras["domain_randomization"]`` values are 0-dim device tensors
    (views of one per-step snapshot of the device globals) instead of python floats (rsl_rl accepts both);
  * the errno poll of ``scene.step`` (simulator.py:267, every 10 substeps = 5 env steps) is asynchronous: the reduction is
    enqueued after the step and examined at the following steps (at the latest when the next poll is due), so the loop does not wait for the device;
  * random numbers come from the counter-based Philox stream of the C ABI (include/go2sim.h), not from
    torch's global generator.
"""
import ctypes
import math

import torch

from .capi import C, EnvGlobals, Go2Sim, Go2SimError, _as_device_tensor, load_hip_lib, state_header_mismatch
from .configs import CONTACT_TERM_NAMES, build_stair_terrain, flatten_base_cfg, flatten_walk_cfg
from .contact_terms import DEFAULT_BODY_CONTACT_NAMES, ContactTerms, contact_term_scales, resolve_body_links
from .lidar import LidarScan, env_pose_ptrs, lidar_enabled, lidar_layout
from .model_blob import pack_model
from .stairinfo import NUM_STAIR_INFO, StairInfo, check_one_exteroceptive_layout, env_rows_ptr, stair_info_enabled
from .terrain_manager import TerrainManager
from .terrain_tiles import install_terrain, is_tile_terrain_cfg
from .terrain_wells import build_stairwell_terrain, is_well_terrain_cfg, well_centers
from .wells import WellScan, well_scan_shape

_DEVICE = None
_SEED = 1


def init(backend=None, precision="32", logging_level=None, performance_mode=True, seed=None, device_index=0, **_):
    """Counterpart of ``gs.init`` (genesis/__init__.py:60): selects the ROCm device and the RNG seed."""
    global _DEVICE, _SEED
    if str(precision) != "32":
        raise Go2SimError("go2sim computes in fp32 only (the reference path runs gs.init(precision='32'))")
    if not torch.cuda.is_available():
        raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
    torch.cuda.set_device(device_index)
    _DEVICE = torch.device("cuda", device_index)
    if seed is not None:
        _SEED = int(seed)
    return _DEVICE


def is_base_env_cfg(env_cfg, obs_cfg):
    """True for the cfg dicts of go2_env_base.py (crouch / jump: 12 actions, 45 observations, neither `pls_enable` nor `num_privileged_obs`)."""
    walk_family = "pls_enable" in env_cfg or obs_cfg.get("num_privileged_obs") is not None
    return not walk_family and obs_cfg["num_obs"] == 45 and env_cfg["num_actions"] == 12


def mirror_tables(env_cfg, obs_cfg):
    """The left-right mirror (reflection in the robot's x-z plane) of the observation and action layout these cfg dicts give an env, as three signed
    permutations ``{"policy": (src, sign), "critic": (src, sign), "actions": (src, sign)}`` with ``(M x)[j] = sign[j] * x[src[j]]`` (int32 / float32
    CPU tensors).  Joints and legs are ordered FR, FL, RR, RL: the mirror swaps FR <-> FL and RR <-> RL and hip angles change sign; polar vectors
    take (+, -, +), the angular velocity (-, +, -), the commands (vx, vy, wz) (+, -, -); scalars are fixed points; height-scan point
    ix * ny + iy maps to ix * ny + (ny - 1 - iy), and so does a point of either grid of the LIDAR layout (the actor scan closes the actor row and
    follows the observations in the critic row, the critic scan closes the critic row) and of the stairwell env's 11 x 11 scan.  The four columns of the stair-info layout (edge distance, riser
    height, tread depth, direction up / down along the forward axis) are fixed points with sign +1 in both rows."""
    num_actions, num_obs, num_priv = env_cfg["num_actions"], obs_cfg["num_obs"], obs_cfg.get("num_privileged_obs")
    base = is_base_env_cfg(env_cfg, obs_cfg)
    leg = [1, 0, 3, 2]
    joints = ([3 * leg[j // 3] + j % 3 for j in range(12)], [-1.0 if j % 3 == 0 else 1.0 for j in range(12)])
    joint_factors = (joints[0], [1.0] * 12)                              # kp / kd / motor strength: swap the legs, keep the sign
    legs = (leg, [1.0] * 4)
    polar, axial, cmd = ([0, 1, 2], [1.0, -1.0, 1.0]), ([0, 1, 2], [-1.0, 1.0, -1.0]), ([0, 1, 2], [1.0, -1.0, -1.0])
    scalar = ([0], [1.0])

    def cat(blocks):
        src, sign = [], []
        for b_src, b_sign in blocks:
            src += [len(sign) + k for k in b_src]
            sign += list(b_sign)
        return src, sign

    if num_actions not in (12, 16):
        raise Go2SimError(f"no mirror for {num_actions} actions (12 joint targets, optionally 4 per-leg stiffness actions)")
    actions = cat([joints] + ([legs] if num_actions == 16 else []))
    obs_blocks = [axial, polar, cmd, joints, joints, actions]            # angular velocity, gravity, commands, dof pos, dof vel, actions
    lidar = None
    if not base and lidar_enabled(env_cfg):                              # the LIDAR layout: the actor scan closes the actor row, the critic scan the critic row
        lidar = lidar_layout(env_cfg["lidar"])
        for name in ("actor", "critic"):
            ys = lidar[name + "_y"]
            if any(ys[k] != -ys[len(ys) - 1 - k] for k in range(len(ys))):
                raise Go2SimError(f"the lidar {name} scan's y points {ys} are not symmetric about 0: the scan has no mirror")

        def scan_block(shape):
            nx, ny = shape
            return ([ix * ny + (ny - 1 - iy) for ix in range(nx) for iy in range(ny)], [1.0] * (nx * ny))

        obs_blocks.append(scan_block(lidar["actor_shape"]))
    stair_info = not base and stair_info_enabled(env_cfg)
    four = (list(range(NUM_STAIR_INFO)), [1.0] * NUM_STAIR_INFO)
    if stair_info:                                                       # the stair-info layout: the actor four close the actor row, the clean four the critic row
        obs_blocks.append(four)
    obs = cat(obs_blocks)
    if base or num_priv is None:
        critic = obs
    else:
        # base_lin_vel, friction, kp / kd / motor-strength factors, mass shift, com shift, leg mass shifts, gravity offset, push force, delay
        blocks = [obs, polar, scalar, joint_factors, joint_factors, joint_factors, scalar, polar, legs, polar, polar, scalar]
        extra = num_priv - (num_obs + 55)
        terrain = env_cfg.get("terrain") or {}
        if lidar is not None:                                              # terrain row, then the critic scan
            blocks += [scalar, scan_block(lidar["critic_shape"])]
        elif stair_info:                                                   # terrain row, then the clean four
            blocks += [scalar, four]
        elif extra > 0 and terrain.get("enabled", False):                   # the stair layout: terrain row, then the height scan
            hs = terrain.get("height_scan", {})
            well = is_well_terrain_cfg(terrain)                             # the stairwell layout: well level, then the square scan (its defaults)
            nx, ny = (well_scan_shape(terrain) if well else (int(hs.get("num_x", 11)), int(hs.get("num_y", 7))))
            yr = hs.get("y_range", [-0.5, 0.5] if well else [-0.3, 0.3])
            if float(yr[0]) != -float(yr[1]):
                raise Go2SimError(f"the height scan's y_range {list(yr)} is not symmetric about 0: the scan has no mirror")
            blocks += [scalar, ([ix * ny + (ny - 1 - iy) for ix in range(nx) for iy in range(ny)], [1.0] * (nx * ny))]
        elif extra > 0:                                                    # a wider critic input without terrain holds zeros there
            blocks.append((list(range(extra)), [1.0] * extra))
        critic = cat(blocks)
    out = {}
    for key, (src, sign), width in zip(("policy", "critic", "actions"), (obs, critic, actions), (num_obs, num_obs if base or num_priv is None else num_priv, num_actions)):
        if len(src) != width:
            raise Go2SimError(f"mirror table {key!r} has {len(src)} entries, the layout's width is {width}")
        out[key] = (torch.tensor(src, dtype=torch.int32), torch.tensor(sign, dtype=torch.float32))
    return out


ENV_STATE_VERSION = 1
LAYOUT_LAUNCHES = (StairInfo, LidarScan, WellScan)       # the launches that widen the observation rows: an env has at most one


def env_state_schema(family, num_envs, num_obs, num_critic_obs, core_bytes=None, lidar_points=None, n_globals=None, cterms=False, launches=None):
    """What ``Go2Env.state_dict()`` of such an env holds: {key: int | str | (dtype, shape)}; a shape entry None is not checked.  `family` is one of
    base, walk, stairs, stairs_lidar, stairs_info, rough, stairwell; `num_critic_obs` the width of the privileged rows as the env keeps them;
    `cterms`: the env runs the contact-terms launch (a non-zero body_contact or stumble scale); `launches`: an env's own list, in place of both."""
    B, f32 = int(num_envs), torch.float32
    schema = {"version": int, "family": str, "num_envs": int, "num_obs": int, "num_critic_obs": int, "terrain_rows_locked": int, "steps_since_poll": int,
              "core": (torch.uint8, (core_bytes,)), "obs_buf": (f32, (B, int(num_obs))), "privileged_obs_buf": (f32, (B, int(num_critic_obs))),
              "rew_buf": (f32, (B,)), "reset_buf": (torch.uint8, (B,)), "time_outs": (f32, (B,)),
              "extras_snapshot": (f32, (None,)), "extras_full_snapshot": (f32, (None,))}
    if launches is None:                                                # each launch owns its keys
        for kind in [k for k in LAYOUT_LAUNCHES if k.STATE_FAMILY == family] + [ContactTerms] * bool(cterms):
            schema.update(kind.schema_of(B, lidar_points))
    for launch in launches or ():
        schema.update(launch.state_schema(B))
    return schema


def check_env_state(state, schema, expect):
    """Go2SimError unless `state` has every key of `schema` with its type, dtype and shape, and its scalars equal `expect` (a dict: version, family,
    num_envs, num_obs, num_critic_obs).  Nothing is written anywhere: load_state_dict calls this before it touches the env."""
    if not isinstance(state, dict):
        raise Go2SimError(f"an env state is a dictionary, got {type(state).__name__}")
    missing = sorted(k for k in schema if k not in state)
    if missing:
        raise Go2SimError(f"the env state lacks the key(s) {missing}")
    for key, want in expect.items():
        if state[key] != want:
            raise Go2SimError(f"the env state was saved with {key} = {state[key]!r}, this env has {key} = {want!r}")
    for key, kind in schema.items():
        v = state[key]
        if isinstance(kind, type):
            if not isinstance(v, kind) or isinstance(v, bool):
                raise Go2SimError(f"the env state's {key!r} must be a plain {kind.__name__}, got {type(v).__name__}")
            continue
        dtype, shape = kind
        if not torch.is_tensor(v) or v.dtype != dtype:
            raise Go2SimError(f"the env state's {key!r} must be a {dtype} tensor, got {getattr(v, 'dtype', type(v).__name__)}")
        if v.dim() != len(shape) or any(w is not None and int(n) != int(w) for n, w in zip(v.shape, shape)):
            raise Go2SimError(f"the env state's {key!r} has shape {tuple(v.shape)}, this env's is {tuple('*' if w is None else w for w in shape)}")


class Go2Env:
    def __init__(self, num_envs, env_cfg, obs_cfg, reward_cfg, command_cfg, show_viewer=False, *, seed=None, device=None,
                 freeze_curriculum=False, log_extras=True, errno_poll_every=5, shared_globals=False):
        if show_viewer:
            raise Go2SimError("the viewer is outside the accelerated path (SURVEY.md section 8f)")
        check_one_exteroceptive_layout(env_cfg)
        base = is_base_env_cfg(env_cfg, obs_cfg)
        use_wells = is_well_terrain_cfg(env_cfg.get("terrain")) and not base
        if use_wells and (env_cfg.get("lidar") or env_cfg.get("stair_info")):
            raise Go2SimError("the stairwell terrain has its own 11 x 11 scan: it does not combine with env_cfg['lidar'] or env_cfg['stair_info']")
        # The layout launch: the step kernels write inner rows without a height scan (49 / 105, 45 / 101 with pls_enable=False), one more launch writes
        # the wider rows -- the stair info (go2_env_stair_lidar_2.py; include/go2sim_stairinfo.h), the LIDAR scans (go2_env_stair_lidar.py;
        # include/go2sim_lidar.h), or the stairwell's scan with its alive term (go2_env_stair6_Omni.py; include/go2sim_wells.h)
        layout = None if base else StairInfo if stair_info_enabled(env_cfg) else LidarScan if lidar_enabled(env_cfg) else WellScan if use_wells else None
        inner_obs_cfg = obs_cfg
        if layout is not None:                                              # obs_cfg must carry the layout's widths (before anything touches the device)
            inner_widths = layout.inner_widths(env_cfg, obs_cfg)
            inner_obs_cfg = dict(obs_cfg, num_obs=inner_widths[0], num_privileged_obs=inner_widths[1])
        cterm_scales = (0.0, 0.0) if base else contact_term_scales(reward_cfg)
        if any(cterm_scales):                                               # an unknown link name is refused; the reference warns and drops the term
            cterm_body_links = resolve_body_links(env_cfg.get("body_contact_names", list(DEFAULT_BODY_CONTACT_NAMES)))
        self.device = device if device is not None else (_DEVICE if _DEVICE is not None else init())
        self.num_envs = num_envs
        self.num_obs = obs_cfg["num_obs"]
        self.num_privileged_obs = obs_cfg.get("num_privileged_obs", None)
        self.num_actions = env_cfg["num_actions"]
        self.num_pos_actions = env_cfg.get("num_pos_actions", 12)
        self.num_commands = command_cfg["num_commands"]
        self.simulate_action_latency = env_cfg.get("simulate_action_latency", True)
        self.dt = 0.02
        self.max_episode_length = math.ceil(env_cfg["episode_length_s"] / self.dt)
        self.env_cfg, self.obs_cfg, self.reward_cfg, self.command_cfg = env_cfg, obs_cfg, reward_cfg, command_cfg
        self.obs_scales = obs_cfg["obs_scales"]
        self.reward_scales = dict(reward_cfg["reward_scales"])

        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._sim = Go2Sim(load_hip_lib(), pack_model(), num_envs, dev_index, _SEED if seed is None else int(seed))
        # the two env families of the reference: walk / stairs (go2_env_walk.py / go2_env_stair.py: 16 actions and 49 / 104 / 182 obs with per-leg
        # stiffness, 12 and 45 / 100 / 178 without) and base (go2_env_base.py: 12 / 45).  The walk family's train scripts set `pls_enable` and
        # `num_privileged_obs`, the base env's set neither (go2_train_crouch.py / go2_train_jump.py)
        self.is_base_env = base
        self._lidar = self._stairinfo = self._wells = self._cterms = None    # the launch handles by name; self._launches is what the env runs
        self.terrain = None                                                # the TerrainManager of the rough-terrain env
        B, dev, handle_seed = num_envs, self.device, _SEED if seed is None else int(seed)
        if self.is_base_env:
            fcfg, icfg, self._reward_names = flatten_base_cfg(num_envs, env_cfg, obs_cfg, reward_cfg, command_cfg)
            self.num_privileged_obs = None
        else:
            fcfg, icfg, self._reward_names = flatten_walk_cfg(num_envs, env_cfg, inner_obs_cfg, reward_cfg, command_cfg,
                                                              freeze_curriculum=freeze_curriculum, shared_globals=shared_globals)
            layouts = {(16, 49): (None, 104, 182)}
            if not env_cfg.get("pls_enable", False):
                layouts[(12, 45)] = (None, 100, 178)
            if inner_obs_cfg is not obs_cfg:
                icfg[C["GO2SIM_IC_SCAN_N"]] = 0                                  # the scans are the scan launch's
            elif self.num_privileged_obs not in layouts.get((self.num_actions, self.num_obs), ()):
                raise Go2SimError("go2sim implements the walk layout (16 actions, 49 / 104 obs; go2_train_walk.py:300-320), the stair layout "
                                  "(49 / 182 obs; go2_train_stair.py:282-300), both with pls_enable=False (12 actions, 45 / 100 and 45 / 178 obs) "
                                  "and the base layout (12 actions, 45 obs; go2_train_crouch.py / "
                                  "go2_train_jump.py)")
            terrain_cfg = env_cfg.get("terrain", None)
            if is_tile_terrain_cfg(terrain_cfg):
                # the rough-terrain env (go2_env_Omni_kplearn_varied_terrain.py:  a terrain dictionary with `subterrain_types` or a `height_field`):
                # the manager makes the morph, the library takes its field and runs ground height, boundary and spawn itself (include/go2sim_tiles.h)
                if layout is not None:
                    raise Go2SimError("the LIDAR / stair-info layouts belong to the stair terrain, not to a tile terrain")
                self.terrain = TerrainManager(terrain_cfg, num_envs, device=self.device)
                morph = self.terrain.build_terrain_morph()
                install_terrain(self._sim, morph.height_field, morph.horizontal_scale, morph.vertical_scale, list(morph.pos))
                self.terrain.post_build(morph)
                self.terrain.bind(self)
            elif terrain_cfg is not None and terrain_cfg.get("enabled", False):
                if use_wells:                                                     # go2_env_stair6_Omni.py:371-397: the grid of stairwells
                    hf, info = build_stairwell_terrain(terrain_cfg)
                    info = dict(info, row_centers=well_centers(info), num_difficulty_rows=info["num_difficulty_levels"])
                else:                                                             # go2_env_stair.py:352-433: gs.morphs.Terrain instead of the plane
                    hf, info = build_stair_terrain(terrain_cfg)
                self._terrain_info = info
                self._sim.set_terrain(hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"])
                field = (B, hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"])
                noise = dict(seed=handle_seed, dr_schedule=env_cfg.get("dr_schedule", None),
                             curriculum_enabled=bool((env_cfg.get("curriculum", {}) or {}).get("enabled", False)), device=dev)
                if layout is StairInfo:
                    depths = info.get("step_depths_m", [float(info.get("step_depth_m", 0.30))] * info["num_difficulty_rows"])
                    self._stairinfo = StairInfo(env_cfg["stair_info"], *field, info["step_heights_m"], depths, **noise)
                elif layout is LidarScan:
                    self._lidar = LidarScan(env_cfg["lidar"], *field, **noise)
                elif layout is WellScan:
                    self._wells = WellScan(terrain_cfg, *field, n_levels=info["num_difficulty_levels"], alive_scale=self.reward_scales.get("alive"), dt=self.dt,
                                           device=dev)
        self._sim.env_configure(fcfg, icfg)

        self.body_contact_count = torch.zeros(B, device=dev)               # links of body_contact_names in contact at the last step, per env
        cterm_keys = [] if self.is_base_env else [n for n in CONTACT_TERM_NAMES if n in self.reward_scales]
        if any(cterm_scales):
            # body_contact (go2_env_stair_lidar_2.py) and stumble (go2_env_terrain.py): one launch after the step's own reads the links' contact forces
            # where the solve left them and adds both terms (include/go2sim_cterms.h)
            self._cterms = ContactTerms(B, body_links=cterm_body_links, body_contact_scale=cterm_scales[0], stumble_scale=cterm_scales[1],
                                        body_contact_threshold=float(env_cfg.get("body_contact_threshold", 1.0)),
                                        stumble_threshold=float(reward_cfg.get("stumble_threshold", 5.0)), dt=self.dt, device=dev, report=cterm_keys,
                                        count_out=self.body_contact_count)
        # In the order the rewards are added: at most one layout launch (alive), then the contact terms (body_contact, stumble)
        self._launches = [h for h in (self._stairinfo, self._lidar, self._wells, self._cterms) if h is not None]
        # a zero scale without the launch: the key is accepted, nothing runs, the entry is zero
        self._episode_zeros = {} if self._cterms is not None else dict.fromkeys(["rew_" + n for n in cterm_keys], torch.zeros((), device=dev))
        # what the launches read in place: the base pose buffers, the curriculum level, the terrain rows, the links' contact forces (SoA [link * 3 + comp][B])
        self._base_pose = env_pose_ptrs(self._sim)
        self._level_ptr = self._sim.env_globals_ptr() + EnvGlobals.level.offset
        self._terrain_rows_ptr = env_rows_ptr(self._sim)
        self._contact_force_ptr = self._sim.field_ptr(C["GO2SIM_F_CONTACT_FORCE"])
        # the step kernels' inner rows, rewritten every step (None: the step kernels write the env's own row)
        self._inner_obs = torch.zeros(B, inner_widths[0], device=dev) if layout is not None and layout.WIDENS_OBS else None
        self._inner_priv = torch.zeros(B, inner_widths[1], device=dev) if layout is not None else None
        # names the env tests read: the inner rows' proprioceptive width (only with a layout launch) and the contact terms' per-env episode records
        if layout is not None:
            self._lidar_n_in = inner_widths[0]
        if self._cterms is not None:
            self._cterms_ep = self._cterms.ep
        self.obs_buf = torch.zeros(B, self.num_obs, device=dev)
        self.privileged_obs_buf = torch.zeros(B, 45 if self.is_base_env else (self.num_privileged_obs or self.num_obs + 55), device=dev)
        self.rew_buf = torch.zeros(B, device=dev)
        self.reset_buf = torch.zeros(B, dtype=torch.uint8, device=dev)
        self._time_outs = torch.zeros(B, device=dev)
        self._actions = torch.zeros(B, self.num_actions, device=dev)
        self.extras = {"observations": {}}
        # live device view of the curriculum / DR globals and the last reset's episode log
        gptr = self._sim.env_globals_ptr()
        self._glob_f32 = _as_device_tensor(gptr, (ctypes.sizeof(EnvGlobals) // 4,), torch.float32, dev)
        self._ep_off = EnvGlobals.last_episode_rew.offset // 4
        self._glob_f64 = self._glob_f32.view(torch.float64)     # the python-float state of the reference is kept in double (include/go2sim.h)
        self._level_off = EnvGlobals.level.offset // 8
        self._goff = {name: getattr(EnvGlobals, name).offset // (8 if ct is ctypes.c_double else 4) for name, ct in EnvGlobals._fields_}
        self._episode_keys = ["rew_" + n for n in self._reward_names]
        self._use_terrain = hasattr(self, "_terrain_info")
        self._terrain_rows_locked = False
        self.log_extras = bool(log_extras)            # per-step snapshot of the episode / curriculum / DR logs (one small device copy)
        self.errno_poll_every = int(errno_poll_every)  # env steps between errno polls (simulator.py:267: every 10 substeps)
        self.freeze_curriculum = bool(freeze_curriculum)  # what evaluation.Evaluator asks for
        self._steps_since_poll = 0
        self._views = {}
        self._extras_snapshot = self._extras_full_snapshot = None
        self._shared_globals = bool(shared_globals) and not self.is_base_env
        if self._shared_globals:
            # one batch sharded over ranks: the first sync (before the constructor's reset) puts every shard at the single-process starting point -- rank 0's
            # t_sample at level_init and first global draws; without it the shard's first episodes would sample the easy end of every DR range
            self.sync_globals(initial=True)
        self.reset()

    # ---- reference API -------------------------------------------------------------------------
    def step(self, actions):
        """go2_env_walk.py:985-1109.  ``actions`` [num_envs, num_actions] float32 on ``self.device``.

        Like the reference (``self.obs_buf = torch.cat(...)``, go2_env_walk.py:1084 / go2_env_base.py:175), every step returns NEW
        observation tensors: rsl_rl's PPO keeps ``transition.observations = obs`` by reference across ``env.step`` and copies it afterwards,
        so an observation buffer overwritten in place would pair o_{t+1} with a_t in the rollout storage."""
        if actions.shape != (self.num_envs, self.num_actions):
            raise Go2SimError(f"actions must have shape {(self.num_envs, self.num_actions)}, got {tuple(actions.shape)}")
        a = actions
        if a.dtype != torch.float32 or not a.is_contiguous() or a.device != self.device:
            a = self._actions.copy_(actions)
        self._raise_on_errno(self._sim.errno_poll_result())               # result of the poll enqueued after an earlier step
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.obs_buf = torch.empty_like(self.obs_buf)                      # caching allocator: host-side only, no kernel
        self.privileged_obs_buf = torch.empty_like(self.privileged_obs_buf)
        self._sim.env_step(a, self.obs_buf if self._inner_obs is None else self._inner_obs,
                           self.privileged_obs_buf if self._inner_priv is None else self._inner_priv, self.rew_buf, self.reset_buf, self._time_outs, stream)
        for launch in self._launches:                                      # one more launch each, straight into the fresh tensors and onto the reward
            launch.launch(self, self._inner_obs, self._inner_priv)
            if self.log_extras:
                launch.log(self.reset_buf)
        self._steps_since_poll += 1
        poll = self._steps_since_poll >= self.errno_poll_every             # RATE_CHECK_ERRNO = 10 substeps, simulator.py:45,267
        if poll:
            self._steps_since_poll = 0
            self._raise_on_errno(self._sim.errno_poll_wait())              # the previous poll is a whole cadence old: this practically never blocks,
            self._sim.errno_poll_begin(stream)                             # and an error surfaces at most 2 x errno_poll_every steps after it happened
        self.extras["time_outs"] = self._time_outs
        self.extras["observations"]["critic"] = self.privileged_obs_buf if self.num_privileged_obs else self.obs_buf
        if self.log_extras:
            self._refresh_extras(full=poll)
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras

    def _refresh_extras(self, full=True):
        """extras["episode"] (go2_env_walk.py:1228-1235) every step, extras["curriculum"] (:674-686) and extras["domain_randomization"]
        (:756,813) every ``errno_poll_every`` steps, from ONE snapshot of the device globals: a single small device copy, no synchronisation;
        the values are 0-dim views of that snapshot (the reference stores python floats obtained with ``.item()``)."""
        self._set_extras(self._glob_f32.clone(), full)

    def _set_extras(self, snap, full):
        """the extras of one snapshot of the device globals (kept: state_dict() saves the last one and the last full one)"""
        self._extras_snapshot = snap
        n = len(self._reward_names)
        self.extras["episode"] = dict(zip(self._episode_keys, snap[self._ep_off:self._ep_off + n].unbind(0)))
        for launch in self._launches:
            self.extras["episode"].update(launch.episode_entries())
        self.extras["episode"].update(self._episode_zeros)
        if self._use_terrain:
            rows = snap.view(torch.int32)
            self.extras["episode"]["terrain_mean_row"] = rows[self._goff["terrain_row_sum"]].float() / rows[self._goff["last_reset_count"]].clamp(min=1).float()
        if self.is_base_env or not full:
            return
        self._extras_full_snapshot = snap
        f, i, d = snap, snap.view(torch.int32), snap.view(torch.float64)
        g = self._goff
        self.extras["curriculum"] = {
            "level": d[g["level"]], "timeout_rate_ema": d[g["timeout_rate_ema"]], "tracking_ema": d[g["tracking_ema"]],
            "fall_rate_ema": d[g["fall_rate_ema"]], "ready_streak": i[g["ready_streak"]], "hard_streak": i[g["hard_streak"]],
            "cooldown": i[g["cooldown"]], "obs_noise_level_cur": d[g["obs_noise_level_cur"]], "action_noise_std_cur": d[g["action_noise_std_cur"]],
            "push_enable": i[g["push_enable"]], "push_force_range_cur": d[g["push_force_lo"]:g["push_force_lo"] + 2],
            "push_interval_steps": i[g["push_interval"]], "delay_max_cur": i[g["delay_max_cur"]],
            "cmd_ranges": {"lin_vel_x_range": d[g["cmd_x_lo"]:g["cmd_x_lo"] + 2], "lin_vel_y_range": d[g["cmd_y_lo"]:g["cmd_y_lo"] + 2],
                           "ang_vel_range": d[g["cmd_yaw_lo"]:g["cmd_yaw_lo"] + 2]},
        }
        for launch in self._launches:
            self.extras["curriculum"].update(launch.curriculum_entries(d[g["level"]]))
        self.extras["domain_randomization"] = {"friction": f[g["friction"]], "mass_shift": f[g["mass_shift"]],
                                               "com_shift": f[g["com_shift"]:g["com_shift"] + 3],
                                               "leg_mass_shift": f[g["leg_mass_shift"]:g["leg_mass_shift"] + 4]}

    def _raise_on_errno(self, v):
        """rigid_solver.py:1189-1213: the exceptions scene.step raises from its errno poll."""
        if not v:
            return
        if v & C["GO2SIM_ERR_INVALID_FORCE_NAN"]:
            raise Go2SimError("Invalid constraint forces causing 'nan'. Some environments were not advanced.")
        if v & C["GO2SIM_ERR_INVALID_ACC_NAN"]:
            raise Go2SimError("Invalid accelerations causing 'nan'. Some environments were not advanced.")
        if v & (C["GO2SIM_ERR_OVERFLOW_CANDIDATE_CONTACTS"] | C["GO2SIM_ERR_OVERFLOW_COLLISION_PAIRS"]):
            raise Go2SimError("Exceeding max number of broad phase candidate contact pairs / contacts.")

    def get_observations(self):
        self.extras["observations"]["critic"] = self.privileged_obs_buf if self.num_privileged_obs else self.obs_buf
        return self.obs_buf, self.extras

    def mirror_tables(self):
        """The left-right mirror of this env's observation and action layout (module function ``mirror_tables``), for
        ``PPO(symmetry_cfg={"mirror_tables": env.mirror_tables(), ...})``."""
        return mirror_tables(self.env_cfg, self.obs_cfg)

    def get_privileged_observations(self):
        return self.privileged_obs_buf if self.num_privileged_obs is not None else None

    def reset(self):
        """go2_env_walk.py:1242-1245 (reset_idx over all envs; obs_buf is not recomputed, as in the reference)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._sim.env_reset(stream)
        self.reset_buf.fill_(1)
        self._clear_launches()
        if self.log_extras:
            self._refresh_extras()
        return self.obs_buf, None

    def _clear_launches(self, idx=None):
        """the launches' share of a reset of the envs `idx` (None: all): stored rows := 0, episode terms handed over and their records logged"""
        mask = self.reset_buf
        if idx is not None and self.log_extras and any(launch.logs for launch in self._launches):
            mask = torch.zeros(self.num_envs, device=self.device)
            mask[idx.long()] = 1.0
        for launch in self._launches:
            launch.clear(idx)
            if self.log_extras:
                launch.log(mask)

    def reset_idx(self, envs_idx):
        """go2_env_walk.py:1156-1240: curriculum bookkeeping, "global" DR draws and per-env reset of ``envs_idx`` (index tensor / list)."""
        idx = torch.as_tensor(envs_idx, device=self.device).to(torch.int32).contiguous()
        if idx.numel() == 0:
            return
        self._sim.env_reset_idx(idx, idx.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        self.reset_buf[idx.long()] = 1
        self._clear_launches(idx)
        if self.log_extras:
            self._refresh_extras()

    _cterms_log = property(lambda self: self._cterms.ep_log)               # the contact terms' logged means, under the name the env tests read

    # ---- snapshots (include/go2sim_state.h, ENV_STATE.md) ---------------------------------
    @property
    def state_family(self):
        if self.is_base_env:
            return "base"
        for launch in self._launches:
            if launch.STATE_FAMILY:
                return launch.STATE_FAMILY
        if self.terrain is not None:
            return "rough"
        return "stairs" if self._use_terrain else "walk"

    def _state_schema(self):
        schema = env_state_schema(self.state_family, self.num_envs, self.num_obs, self.privileged_obs_buf.shape[1], self._sim.state_size(),
                                  launches=self._launches)
        expect = {"version": ENV_STATE_VERSION, "family": self.state_family, "num_envs": self.num_envs, "num_obs": self.num_obs,
                  "num_critic_obs": int(self.privileged_obs_buf.shape[1])}
        return schema, expect

    def state_dict(self):
        """Everything of this env that outlives a step, as CPU tensors and plain numbers (eval_io.read_checkpoint reads them without executing
        anything): the core's record (go2sim_state_save), the LIDAR / stair-info / wells handles' state, and the env's own tensors -- the rows
        get_observations() returns, the reset flags and time-outs, the terrain-row lock, the poll cadence and the snapshots behind ``extras``.
        Static inputs (heightfield, tiles, well centres, model, cfgs, seed) are not state: the caller builds the env from them.  Waits for the stream."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rec = torch.empty(self._sim.state_size(), dtype=torch.uint8, device=self.device)
        self._sim.state_save(rec, stream=stream)
        _, sd = self._state_schema()
        sd = dict(sd, terrain_rows_locked=int(self._terrain_rows_locked), steps_since_poll=int(self._steps_since_poll), core=rec.cpu())
        for key, t in (("obs_buf", self.obs_buf), ("privileged_obs_buf", self.privileged_obs_buf), ("rew_buf", self.rew_buf), ("reset_buf", self.reset_buf),
                       ("time_outs", self._time_outs), ("extras_snapshot", self._extras_snapshot), ("extras_full_snapshot", self._extras_full_snapshot)):
            sd[key] = torch.zeros(0) if t is None else t.detach().cpu().clone()
        for launch in self._launches:
            sd.update(launch.state_dict())
        return sd

    def load_state_dict(self, state):
        """Put a ``state_dict()`` back into an env built from the same cfgs, num_envs and seed: ``get_observations()`` then returns the saved rows and
        the next ``step(a)`` returns what the saved env's next ``step(a)`` returned, bit for bit.  The dictionary is validated before anything is
        written (keys, family, widths, num_envs), and the core compares the record's header with its own (seed, model and configuration digests)
        before it writes: a Go2SimError names the mismatch and leaves the env as it was."""
        schema, expect = self._state_schema()
        check_env_state(state, schema, expect)
        dev, stream = self.device, torch.cuda.current_stream(self.device).cuda_stream
        rec = state["core"].to(dev)
        if self._sim.state_load(rec, stream=stream) != C["GO2SIM_E_OK"]:
            mine = torch.empty_like(rec)
            self._sim.state_save(mine, stream=stream)
            n = 4 * C["GO2SIM_STATE_HDR_WORDS"]
            names = state_header_mismatch(rec[:n].cpu().view(torch.int32).tolist(), mine[:n].cpu().view(torch.int32).tolist())
            raise Go2SimError(f"go2sim_state_load refused the record: its {' and '.join(names) or 'header'} differ(s) from this env's "
                              "(build the env from the cfgs, num_envs and seed the state was saved with)")
        self.obs_buf, self.privileged_obs_buf = state["obs_buf"].to(dev), state["privileged_obs_buf"].to(dev)
        self.rew_buf.copy_(state["rew_buf"]); self.reset_buf.copy_(state["reset_buf"]); self._time_outs.copy_(state["time_outs"])
        self._terrain_rows_locked, self._steps_since_poll = bool(state["terrain_rows_locked"]), int(state["steps_since_poll"])
        for launch in self._launches:
            launch.load_state_dict(state)
        self.extras = {"observations": {"critic": self.privileged_obs_buf if self.num_privileged_obs else self.obs_buf}, "time_outs": self._time_outs}
        self._extras_snapshot = self._extras_full_snapshot = None
        n_glob = self._glob_f32.numel()
        for key, full in (("extras_full_snapshot", True), ("extras_snapshot", False)):      # the last full one first: the per-step entries come from the later one
            if state[key].numel() == n_glob:
                self._set_extras(state[key].to(dev), full)
        torch.cuda.current_stream(self.device).synchronize()                   # the handles' setters read host copies of the state's tensors

    # ---- eval / teleop surface (go2_eval_walk.py, go2_eval_stairs.py) ------------------------------
    @property
    def _lock_terrain_rows(self):
        return self._terrain_rows_locked

    @_lock_terrain_rows.setter
    def _lock_terrain_rows(self, value):
        """go2_env_stair.py:399,1513; go2_eval_stairs.py:657 sets it after the first reset."""
        self._terrain_rows_locked = bool(value)
        self._sim.env_lock_terrain_rows(self._terrain_rows_locked, torch.cuda.current_stream(self.device).cuda_stream)

    def set_terrain_rows(self, rows):
        """``env._env_terrain_row[:] = rows`` of the eval scripts."""
        r = torch.as_tensor(rows, device=self.device).to(torch.int32).expand(self.num_envs).contiguous()
        self._sim.env_set_terrain_rows(r, torch.cuda.current_stream(self.device).cuda_stream)

    def respawn(self, envs_idx, pos, quat=None, clear_buffers=True):
        """Teleport ``envs_idx`` to ``pos`` [n, 3] (``quat`` [n, 4] wxyz, default base_init_quat) in the default joint pose with zero velocity:
        respawn_at_start (go2_eval_stairs.py:314-361, clear_buffers=True) / respawn_on_tile (go2_eval_walk.py:399-480, clear_buffers=False)."""
        idx = torch.as_tensor(envs_idx, device=self.device).to(torch.int32).contiguous()
        p = torch.as_tensor(pos, device=self.device, dtype=torch.float32).reshape(idx.numel(), 3).contiguous()
        q = None if quat is None else torch.as_tensor(quat, device=self.device, dtype=torch.float32).reshape(idx.numel(), 4).contiguous()
        self._sim.env_respawn(idx, p, q, clear_buffers, idx.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        if clear_buffers and idx.numel():
            for launch in self._launches:
                launch.clear(idx)

    def respawn_at_start(self, envs_idx=(0,)):
        """go2_eval_stairs.py:314-361: back to the spawn point of the env's terrain row (or base_init_pos on flat ground)."""
        idx = torch.as_tensor(envs_idx, device=self.device).long()
        if self._use_terrain:
            rows = self._env_view("TERRAIN_ROW", 1, torch.int32)[idx].long()
            centers = torch.tensor(self._terrain_info["row_centers"], device=self.device, dtype=torch.float32)
            pos = centers[rows].clone()
            pos[:, 2] += float(self.env_cfg["base_init_pos"][2])
        else:
            pos = torch.tensor(self.env_cfg["base_init_pos"], device=self.device, dtype=torch.float32).expand(idx.numel(), 3)
        self.respawn(idx, pos, None, True)

    # ---- state the reference exposes as attributes ----------------------------------------------
    def _env_view(self, name, k, dtype=torch.float32):
        key = (name, k)
        if key not in self._views:
            self._views[key] = torch.zeros(self.num_envs, k, dtype=dtype, device=self.device)
        buf = self._views[key]   # env_get delivers the reference's [n_envs, k] layout
        self._sim.env_get(C["GO2SIM_EB_" + name], buf, torch.cuda.current_stream(self.device).cuda_stream)
        return buf if k > 1 else buf[:, 0]

    @property
    def episode_length_buf(self):
        return self._env_view("EPISODE_LENGTH", 1, torch.int32)

    @episode_length_buf.setter
    def episode_length_buf(self, value):
        """rsl_rl ``init_at_random_ep_len`` assigns a fresh tensor here (on_policy_runner)."""
        v = value.to(device=self.device, dtype=torch.int32).contiguous()
        self._sim.env_set_episode_length(v, torch.cuda.current_stream(self.device).cuda_stream)

    commands = property(lambda self: self._env_view("COMMANDS", 3))
    base_lin_vel = property(lambda self: self._env_view("BASE_LIN_VEL", 3))
    base_ang_vel = property(lambda self: self._env_view("BASE_ANG_VEL", 3))
    projected_gravity = property(lambda self: self._env_view("PROJECTED_GRAVITY", 3))
    dof_pos = property(lambda self: self._env_view("DOF_POS", 12))
    dof_vel = property(lambda self: self._env_view("DOF_VEL", 12))
    base_pos = property(lambda self: self._env_view("BASE_POS", 3))
    base_quat = property(lambda self: self._env_view("BASE_QUAT", 4))
    base_euler = property(lambda self: self._env_view("BASE_EULER", 3))
    # rough-terrain env (go2_env_Omni_kplearn_varied_terrain.py `_ground_height`): the bilinear ground height under the base at the last step
    _ground_height = property(lambda self: self._env_view("GROUND_HEIGHT", 1))

    @property
    def episode_sums(self):
        sums = self._env_view("EPISODE_SUMS", 32)
        return {n: sums[:, i] for i, n in enumerate(self._reward_names)}

    def set_commands(self, commands):
        """Eval scripts overwrite ``env.commands`` (go2_eval_walk.py); here through the setter of the C ABI."""
        v = commands.to(device=self.device, dtype=torch.float32).contiguous()
        self._sim.env_set_commands(v, torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def base_gains(self):
        """(kp_val, kd_val) [num_envs] float32 drawn at each env's last reset (pls_enable=False with kp_range; go2_env_walk.py:776-781)."""
        out = torch.zeros(2, self.num_envs, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._sim.get_field(C["GO2SIM_F_BASE_KP"], out[0], stream)
        self._sim.get_field(C["GO2SIM_F_BASE_KD"], out[1], stream)
        return out[0], out[1]

    @property
    def engine_gains(self):
        """(kp, kv) the motor dofs' engine PD runs with after the last reset call when the batch gain is on (pls_enable=False, kp_range set, no
        kp_factor_range: the mean effective gains, go2_env_walk.py:797-801); float32 scalars on the device, no synchronisation."""
        return self._glob_f32[self._goff["engine_kp"]], self._glob_f32[self._goff["engine_kd"]]

    @property
    def curriculum_level(self):
        return self._glob_f64[self._level_off]

    def curriculum_state(self):
        """extras["curriculum"] of the reference (go2_env_walk.py:674-690); this call synchronises the stream."""
        return self._sim.env_globals(torch.cuda.current_stream(self.device).cuda_stream).as_dict()

    def sync_globals(self, group=None, initial=False):
        """One batch sharded over ranks (``shared_globals=True``): all-reduce of the curriculum counters, the shared state machine, broadcast of
        rank 0's global DR draws (distributed.sync_env_globals).  Call on every rank once per rollout."""
        from .distributed import sync_env_globals

        return sync_env_globals(self._sim, group, torch.cuda.current_stream(self.device).cuda_stream, initial=initial)

    def check_errno(self):
        """rigid_solver.py:1208-1211: blocking form of the poll (``step`` runs the asynchronous one every ``errno_poll_every`` steps)."""
        v = self._sim.check_errno(torch.cuda.current_stream(self.device).cuda_stream)
        self._raise_on_errno(v)
        return v

    def graph_status(self):
        """(step graph in use, number of times the library fell back to plain launches)."""
        return self._sim.graph_status()
