"""Batched policy evaluation: a grid of commands (and terrain rows) over the envs of one Go2Env, the per-step bookkeeping one launch behind the env
step (include/go2sim_evalstats.h states its law), the derived metrics on the host in float64.

    env = Go2Env(4096, *cfgs, freeze_curriculum=True)                         # cfgs[0]["resampling_time_s"] longer than the episode
    grid = command_grid(4096, vx=(0.0, 0.5, 1.0), vy=(0.0,), yaw=(-0.5, 0.0, 0.5))
    report = Evaluator(env, policy, commands=grid).run(max_steps=4000)        # one dictionary per bin: report["bins"][k]["lin_vel_rmse"], ...

``command_grid``, ``bin_metrics`` and the Evaluator's refusals need no GPU.  This stands in for the reference's keyboard teleop scripts
(examples/locomotion/go2_eval_*.py), which answer "how well does it track, how often does it fall, what does it ask of the motors" one robot at a
time in a viewer."""
import ctypes
import itertools
import math

import numpy as np
import torch

from .capi import C, EnvLaunch, Go2SimError, _as_device_tensor, _ptr
from .contact_terms import FOOT_LINK_NAMES, link_mask
from .model_blob import load_model_json

METRICS = ("episodes", "falls", "fall_rate", "mean_episode_s", "lin_vel_rmse", "yaw_rate_rmse", "mean_vx", "mean_vy", "mean_wz", "mean_abs_power_W",
           "cost_of_transport", "torque_rms", "peak_torque", "peak_dof_vel", "frac_steps_over_torque", "frac_steps_over_dof_vel", "tilt_rms",
           "peak_foot_force", "n_samples", "complete")
ENV_BUFFERS = ("COMMANDS", "BASE_LIN_VEL", "BASE_ANG_VEL", "PROJECTED_GRAVITY", "DOF_VEL", "TORQUE")      # what go2sim_env_buffer_dev hands out, in the step's order


class EvalStatsCfg(ctypes.Structure):
    """go2sim_evalstats_cfg_t"""
    DOUBLES = ("dt", "torque_limit", "dof_vel_limit")
    INTS = ("n_envs", "n_bins", "settle_steps", "max_episodes", "n_links")
    _fields_ = [(n, ctypes.c_double) for n in DOUBLES] + [(n, ctypes.c_int) for n in INTS] + [("foot_mask", ctypes.c_uint32)]


class EvalStatsView(ctypes.Structure):
    """go2sim_evalstats_view_t"""
    _fields_ = [("p", ctypes.c_void_p), ("comp_stride", ctypes.c_longlong), ("env_stride", ctypes.c_longlong)]


class EvalStatsIn(ctypes.Structure):
    """go2sim_evalstats_in_t"""
    VIEWS = ("commands", "base_lin_vel", "base_ang_vel", "projected_gravity", "dof_vel", "torque")
    _fields_ = [(n, EvalStatsView) for n in VIEWS] + [("cf", ctypes.c_void_p)] + [(n, ctypes.c_longlong) for n in ("cf_comp_stride", "cf_link_stride", "cf_env_stride")] + \
               [("reset", ctypes.c_void_p), ("time_out", ctypes.c_void_p)]


def _address(x):
    return _ptr(x, True).value or 0


def eval_inputs(views, cf, cf_strides, reset, time_out):
    """A go2sim_evalstats_in_t of device tensors or raw device addresses: ``views`` maps each of EvalStatsIn.VIEWS to (memory, component stride, env
    stride), ``cf_strides`` is (component, link, env), all in elements.  The caller keeps the tensors alive."""
    x = EvalStatsIn()
    for name in EvalStatsIn.VIEWS:
        mem, cs, es = views[name]
        setattr(x, name, EvalStatsView(_address(mem), int(cs), int(es)))
    x.cf, (x.cf_comp_stride, x.cf_link_stride, x.cf_env_stride) = _address(cf), (int(s) for s in cf_strides)
    x.reset, x.time_out = _address(reset), _address(time_out)
    return x


def foot_links(model=None):
    """The model's indices of the four feet (the calf links)."""
    model = load_model_json() if model is None else model
    return [i for i, l in enumerate(model["links"]) if l["name"] in FOOT_LINK_NAMES]


def robot_weight(model=None):
    """(mass of the robot's links in kg, |g| in m / s^2) of the model file: the m g of the cost of transport."""
    model = load_model_json() if model is None else model
    return float(sum(l["inertial_mass"] for l in model["links"][1:])), abs(float(model["gravity"][2]))


class EvalStats(EnvLaunch):
    """The handle of go2sim_evalstats_create.  An evaluation's own: it is no part of Go2Env.state_dict() and the env does not run it."""
    NAME = "evalstats"

    def __init__(self, n_envs, *, n_bins=1, bins=None, dt=0.02, settle_steps=25, max_episodes=4, torque_limit=23.7, dof_vel_limit=30.0, n_links=None,
                 foot_mask=None, device=None):
        EnvLaunch.__init__(self, n_envs, device)
        c = EvalStatsCfg()
        c.dt, c.torque_limit, c.dof_vel_limit = float(dt), float(torque_limit), float(dof_vel_limit)
        c.n_envs, c.n_bins, c.settle_steps, c.max_episodes = self.n_envs, int(n_bins), int(settle_steps), int(max_episodes)
        c.n_links = int(C["GO2SIM_NL"] if n_links is None else n_links)
        c.foot_mask = link_mask(foot_links()) if foot_mask is None else int(foot_mask)
        self.cfg, self.n_bins, self.max_episodes = c, int(n_bins), int(max_episodes)
        host_bins = self._host_bins(bins)                                   # alive across the call
        self._create(c, _ptr(host_bins))
        ep = ctypes.c_void_p()
        self._call("episodes", ctypes.byref(ep))
        self.episodes = _as_device_tensor(ep.value, (self.n_envs,), torch.int32, self.device)      # closed episodes per env, a live device view

    def _host_bins(self, bins):
        if bins is None:
            return None
        b = np.ascontiguousarray(torch.as_tensor(bins).detach().cpu().numpy(), np.int32)
        if b.shape != (self.n_envs,):
            raise Go2SimError(f"bins has shape ({self.n_envs},), got {b.shape}")
        return b

    def set_bins(self, bins):
        host_bins = self._host_bins(bins)
        if host_bins is None:
            raise Go2SimError("set_bins needs int32 [n_envs] values")
        self._call("set_bins", _ptr(host_bins), self._stream())

    def step(self, inputs):
        """go2sim_evalstats_step on an ``eval_inputs(...)`` structure: one launch."""
        self._step(ctypes.c_int(self.n_envs), ctypes.byref(inputs))

    def reduce(self):
        self._call("reduce", self._stream())

    def done(self):
        """0-dim bool device tensor: every env has max_episodes closed episodes (no synchronisation)."""
        return (self.episodes >= self.max_episodes).all()

    def state(self):
        """(run_f float64 [M, n], run_i int32 [K, n], tot_f, tot_i, bin_f float64 [n_bins, M], bin_i int64 [n_bins, KB]) numpy arrays; the bin arrays
        are the last reduce()'s.  Waits for the stream."""
        n, M, K = self.n_envs, C["GO2SIM_ES_M"], C["GO2SIM_EI_K"]
        out = [np.zeros((M, n)), np.zeros((K, n), np.int32), np.zeros((M, n)), np.zeros((K, n), np.int32), np.zeros((self.n_bins, M)),
               np.zeros((self.n_bins, C["GO2SIM_EBIN_K"]), np.int64)]
        self._call("get_state", *(_ptr(a) for a in out), self._stream())
        return tuple(out)

    def env_inputs(self, env):
        """The inputs of a Go2Env, read in place: the core's own buffers (go2sim_env_buffer_dev), the links' contact forces where the solve left them,
        the env's reset flags and time-outs."""
        sim, views = env._sim, {}
        for name, buf in zip(EvalStatsIn.VIEWS, ENV_BUFFERS):
            p, cs, es = ctypes.c_void_p(), ctypes.c_longlong(), ctypes.c_longlong()
            sim.L.check(sim.L.fn("env_buffer_dev")(sim.h, ctypes.c_int(C["GO2SIM_EB_" + buf]), ctypes.byref(p), ctypes.byref(cs), ctypes.byref(es)), "env_buffer_dev")
            views[name] = (p.value, cs.value, es.value)
        n = self.n_envs
        return eval_inputs(views, env._contact_force_ptr, (n, 3 * n, 1), env.reset_buf, env._time_outs)


class CommandGrid:
    """``commands`` float32 [num_envs, 3], ``bins`` int32 [num_envs] and ``cells`` float32 [n_cells, 3] (vx, vy, yaw) of command_grid()."""

    def __init__(self, commands, bins, cells):
        self.commands, self.bins, self.cells = commands, bins, cells


def command_grid(num_envs, vx=(0.0,), vy=(0.0,), yaw=(0.0,)):
    """The cells are the products of the three lists, vx slowest and yaw fastest; env b evaluates cell b % n_cells, which is its bin.  With num_envs no
    multiple of n_cells the first num_envs % n_cells cells have one env more.  More cells than envs are refused."""
    cells = np.array(list(itertools.product([float(v) for v in vx], [float(v) for v in vy], [float(v) for v in yaw])), np.float32).reshape(-1, 3)
    if len(cells) < 1:
        raise Go2SimError("command_grid needs at least one value of each of vx, vy and yaw")
    if len(cells) > int(num_envs):
        raise Go2SimError(f"command_grid: {len(cells)} cells do not fit into {int(num_envs)} envs (an env evaluates one cell)")
    bins = (np.arange(int(num_envs)) % len(cells)).astype(np.int32)
    return CommandGrid(cells[bins].copy(), bins, cells)


def _ratio(a, b):
    return float(a) / float(b) if b else None


def _root(x):
    return None if x is None else (math.sqrt(x) if x >= 0.0 else float("nan"))


def bin_metrics(bin_f, bin_i, dt, mass, gravity):
    """The report of one bin from its reduced totals (float64 [GO2SIM_ES_M], int64 [GO2SIM_EBIN_K]), in Python floats, i.e. float64.  A ratio whose
    denominator is zero (no episode closed, no sample taken, no distance covered) is None."""
    f = {k[len("GO2SIM_ES_"):]: float(bin_f[v]) for k, v in C.items() if k.startswith("GO2SIM_ES_") and k not in ("GO2SIM_ES_M", "GO2SIM_ES_NSUMS")}
    i = {k[len("GO2SIM_EI_"):]: int(bin_i[v]) for k, v in C.items() if k.startswith("GO2SIM_EI_") and k != "GO2SIM_EI_K"}
    envs, complete = int(bin_i[C["GO2SIM_EBIN_ENVS"]]), int(bin_i[C["GO2SIM_EBIN_COMPLETE"]])
    n = f["N"]
    return {
        "episodes": i["EPISODES"], "falls": i["FALLS"], "fall_rate": _ratio(i["FALLS"], i["EPISODES"]),
        "mean_episode_s": _ratio(i["LENGTH_STEPS"] * float(dt), i["EPISODES"]),
        "lin_vel_rmse": _root(_ratio(f["LIN_ERR2"], n)), "yaw_rate_rmse": _root(_ratio(f["YAW_ERR2"], n)),
        "mean_vx": _ratio(f["VX"], n), "mean_vy": _ratio(f["VY"], n), "mean_wz": _ratio(f["WZ"], n),
        "mean_abs_power_W": _ratio(f["ABS_POWER"], n), "cost_of_transport": _ratio(f["ABS_POWER"], float(mass) * float(gravity) * f["SPEED"]),
        "torque_rms": _root(_ratio(f["TORQUE2"], C["GO2SIM_EVALSTATS_NDOF"] * n)), "peak_torque": f["PEAK_TORQUE"], "peak_dof_vel": f["PEAK_DOF_VEL"],
        "frac_steps_over_torque": _ratio(i["OVER_TORQUE"], n), "frac_steps_over_dof_vel": _ratio(i["OVER_DOF_VEL"], n),
        "tilt_rms": _root(_ratio(f["TILT2"], n)), "peak_foot_force": f["PEAK_FOOT_FORCE"], "n_samples": int(n) if math.isfinite(n) else None,
        "complete": envs > 0 and complete == envs, "envs": envs,
    }


class Evaluator:
    """Runs ``policy`` over the envs of ``env`` under scripted commands and reports per bin.

    ``commands``: a CommandGrid (its cells are the bins unless ``bins`` is given) or [num_envs, 3] values with ``bins`` int [num_envs] (default: one
    bin).  ``terrain_rows``: the difficulty rows of a stair-terrain env to evaluate on -- one row per env, or a shorter list that env b walks through
    once per pass over the command cells (row ``terrain_rows[(b // n_cells) % len(terrain_rows)]``); the rows go into the bins (bin = command bin *
    number of distinct rows + index of the row among the sorted distinct rows), are written with ``env.set_terrain_rows`` and locked.
    ``policy``: a module with ``act_inference`` or the callable of ``runner.get_inference_policy()``; ``memory``: the recurrent module whose
    ``reset(dones)`` follows every env step (default: the policy itself, or the module its bound ``act_inference`` belongs to)."""

    def __init__(self, env, policy, *, commands, bins=None, terrain_rows=None, settle_steps=25, max_episodes=4, torque_limit=23.7, dof_vel_limit=30.0,
                 memory=None):
        if getattr(env, "is_base_env", False):
            raise Go2SimError("Evaluator: the base env (crouch / jump) has no velocity commands to track; it evaluates the walk, stair and rough-terrain envs")
        env_cfg, B = env.env_cfg, int(env.num_envs)
        curriculum = bool((env_cfg.get("curriculum", {}) or {}).get("enabled", False))
        if curriculum and not getattr(env, "freeze_curriculum", False):
            raise Go2SimError("Evaluator: build the env with Go2Env(..., freeze_curriculum=True): an evaluation must not move the curriculum level it measures at")
        if not float(env_cfg["resampling_time_s"]) > float(env_cfg["episode_length_s"]):
            raise Go2SimError(f"Evaluator: env_cfg['resampling_time_s'] = {env_cfg['resampling_time_s']} must be longer than the episode "
                              f"(episode_length_s = {env_cfg['episode_length_s']}): a command resampled inside an episode would replace the scripted one for a step")
        if int(settle_steps) < 1:
            raise Go2SimError("Evaluator: settle_steps >= 1 -- the first observation after a reset still carries the command the reset drew")
        if isinstance(commands, CommandGrid):
            cmd, n_cells = commands.commands, len(commands.cells)
            cells = commands.cells if bins is None else None                # the bins are the cells: the report names each bin's command
            bins = commands.bins if bins is None else bins
        else:
            cmd, cells, n_cells = commands, None, 1
        cmd = np.ascontiguousarray(torch.as_tensor(cmd).detach().cpu().numpy(), np.float32)
        if cmd.shape != (B, 3):
            raise Go2SimError(f"Evaluator: commands has shape ({B}, 3) -- (vx, vy, yaw rate) per env -- got {cmd.shape}")
        if not np.isfinite(cmd).all():
            raise Go2SimError("Evaluator: commands must be finite")
        bins = np.zeros(B, np.int32) if bins is None else np.ascontiguousarray(torch.as_tensor(bins).detach().cpu().numpy()).astype(np.int64)
        if bins.shape != (B,) or bins.min() < 0:
            raise Go2SimError(f"Evaluator: bins has shape ({B},) and no negative entry")
        n_bins, rows, self.bin_rows = int(bins.max()) + 1, None, None
        if terrain_rows is not None:
            if not getattr(env, "_use_terrain", False):
                raise Go2SimError("Evaluator: terrain_rows needs an env with the stair terrain enabled (env_cfg['terrain']['enabled'])")
            n_rows = int(env._terrain_info["num_difficulty_rows"])
            given = np.asarray(terrain_rows, np.int64).reshape(-1)
            if len(given) < 1 or given.min() < 0 or given.max() >= n_rows:
                raise Go2SimError(f"Evaluator: terrain_rows lie in [0, {n_rows}), got {given.tolist()[:16]}")
            rows = given if len(given) == B else given[(np.arange(B) // n_cells) % len(given)]
            distinct = sorted(set(rows.tolist()))
            bins = bins * len(distinct) + np.searchsorted(distinct, rows)
            self.bin_rows = [distinct[k % len(distinct)] for k in range(n_bins * len(distinct))]
            n_bins *= len(distinct)
        self.env, self.num_envs, self.n_bins = env, B, n_bins
        self.commands_host, self.bins, self.rows, self.cells = cmd, bins.astype(np.int32), rows, cells
        self._act = policy.act_inference if hasattr(policy, "act_inference") else policy
        if not callable(self._act):
            raise Go2SimError("Evaluator: policy is a module with act_inference or a callable (runner.get_inference_policy())")
        owner = memory if memory is not None else policy if hasattr(policy, "act_inference") else getattr(policy, "__self__", None)
        self._memory = owner if getattr(owner, "is_recurrent", False) else None
        self.mass, self.gravity = robot_weight()
        # from here on the device
        self.stats = EvalStats(B, n_bins=n_bins, bins=self.bins, dt=env.dt, settle_steps=settle_steps, max_episodes=max_episodes, torque_limit=torque_limit,
                               dof_vel_limit=dof_vel_limit, device=env.device)
        self.commands = torch.from_numpy(cmd).to(env.device)
        self._inputs = self.stats.env_inputs(env)
        if rows is not None:
            env.set_terrain_rows(torch.from_numpy(rows))
            env._lock_terrain_rows = True
        self.steps = 0

    def step(self):
        """set_commands, act_inference, env.step, one stats launch; -> what env.step returned and the actions"""
        env = self.env
        env.set_commands(self.commands)
        actions = self._act(self._obs)
        out = env.step(actions)
        self.stats.step(self._inputs)
        self._obs = out[0]
        if self._memory is not None:
            self._memory.reset(out[2])
        self.steps += 1
        return out, actions

    def begin(self):
        """Every env into a fresh episode (on its terrain row), empty records, an empty memory."""
        self.env.reset()
        self.stats.clear()
        if self._memory is not None:
            self._memory.reset()
        self._obs, self.steps = self.env.get_observations()[0], 0

    def run(self, max_steps):
        """-> {"bins": [one dictionary per bin], "steps", "complete", ...}.  Stops when every env has max_episodes closed episodes (tested on the device
        view every env.errno_poll_every steps: one small copy, no wait per step) or after max_steps."""
        self.begin()
        every, pending = max(1, int(self.env.errno_poll_every)), None
        while self.steps < int(max_steps):
            self.step()
            if self.steps % every:
                continue
            if pending is not None:                                         # the answer of the poll before this one: a cadence old, it practically never blocks
                pending[1].synchronize()
                if bool(pending[0][0]):
                    break
            flag, event = torch.empty(1, dtype=torch.bool).pin_memory(), torch.cuda.Event()
            flag.copy_(self.stats.done().reshape(1), non_blocking=True)
            event.record(torch.cuda.current_stream(self.env.device))
            pending = (flag, event)
        return self.report()

    def report(self):
        """Reduce and read back (waits for the stream)."""
        self.stats.reduce()
        bin_f, bin_i = self.stats.state()[4:]
        dt = float(self.env.dt)
        out = []
        for k in range(self.n_bins):
            entry = bin_metrics(bin_f[k], bin_i[k], dt, self.mass, self.gravity)
            if self.cells is not None:
                per = 1 if self.bin_rows is None else len(set(self.bin_rows))
                entry["command"] = [float(v) for v in self.cells[(k // per) % len(self.cells)]]
            if self.bin_rows is not None:
                entry["terrain_row"] = int(self.bin_rows[k])
            out.append(entry)
        return {"bins": out, "steps": self.steps, "num_envs": self.num_envs, "complete": all(e["complete"] for e in out if e["envs"] > 0),
                "settle_steps": int(self.stats.cfg.settle_steps), "max_episodes": int(self.stats.cfg.max_episodes), "dt": dt,
                "mass_kg": self.mass, "gravity": self.gravity}
