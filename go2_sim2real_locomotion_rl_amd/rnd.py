"""Random network distillation -- host-side mirror of ``rsl_rl.modules.RandomNetworkDistillation`` and of what ``rsl_rl.algorithms.PPO`` does with
``rnd_cfg``, on the entry points of include/go2sim_rnd.h (which states the law).  A fixed random target network and a trained predictor embed the
``rnd_state`` rows; their distance is a curiosity bonus that is added to the env's reward before the rollout storage sees it, and the predictor is
regressed onto the target on the mini-batches of the PPO update.

    rnd = RandomNetworkDistillation(num_states=49, num_outputs=8, predictor_hidden_dims=[-1], target_hidden_dims=[-1], weight=0.1 * env.dt,
                                    reward_normalization=True, state_normalization=True, device=dev, seed=1)
    rnd.attach(max_rows)                                   # the largest step or mini-batch, in rows
    intrinsic, rewards_total = rnd.get_intrinsic_reward(rnd_state, rewards)      # counter += 1, two launches (+ the state normaliser's two)
    rnd.last_state                                         # the rows the update reads later (normalised when state_normalization is on)
    rnd_loss = rnd.update(states, idx, n_rows_total, n_epochs, n_mini_batches)   # float64 device scalar; no synchronisation

``PPO(policy, rnd_cfg={...})`` builds and drives one (ppo.py); the runner fills ``num_states`` and scales ``weight`` by ``env.dt`` (runner.py).

State-dict keys: ``predictor.{0,2,..}.{weight,bias}``, ``target.{0,2,..}.{weight,bias}``, ``state_normalizer.{_mean,_var,_std,count}``,
``reward_normalizer.emp_norm.{_mean,_var,_std,count}`` (rsl_rl's names) and ``reward_normalizer.disc_avg.avg`` (the discounted sums, which rsl_rl does not save).
"""
import ctypes

import numpy as np
import torch

from .capi import Go2SimError, RndCfg, _ptr, load_hip_lib
from .module_core import linear_init, mlp_keys, unflatten_keys
from .trainer import OptimizerState, TrainerHandle

RND_CFG_DEFAULTS = {"weight": 0.0, "weight_schedule": None, "reward_normalization": False, "state_normalization": False, "num_outputs": 1,
                    "predictor_hidden_dims": [-1], "target_hidden_dims": [-1], "activation": "elu", "learning_rate": 1e-3}
SCHEDULE_KEYS = {"constant": set(), "step": {"final_step", "final_value"}, "linear": {"initial_step", "final_step", "final_value"}}
TARGET_SEED_PURPOSE = 0x7a26e7                              # the target's draws come from seed + this: predictor and target differ
GAMMA, UNTIL, STATE_EPS = 0.99, 1.0e8, 1.0e-2


# ---- pure functions (no GPU) ---------------------------------------------------------------------------------------------------------------------
def check_rnd_cfg(cfg):
    """rsl_rl's rnd_cfg -> a dict with every entry of the law (defaults filled) plus ``num_states`` when given, or None for None / {}.  Entries the law
    does not name, a schedule mode it does not know or a schedule without its entries are refused."""
    if not cfg:
        return None
    unknown = sorted(set(cfg) - set(RND_CFG_DEFAULTS) - {"num_states"})
    if unknown:
        raise Go2SimError(f"rnd_cfg: unknown entries {unknown}; the entries are {sorted(RND_CFG_DEFAULTS)} (and num_states, which the runner fills)")
    out = {k: cfg.get(k, v) for k, v in RND_CFG_DEFAULTS.items()}
    if "num_states" in cfg and cfg["num_states"] is not None:
        out["num_states"] = int(cfg["num_states"])
    out["weight"] = float(out["weight"])
    out["num_outputs"] = int(out["num_outputs"])
    if out["num_outputs"] < 1:
        raise Go2SimError(f"rnd_cfg: num_outputs must be >= 1, got {out['num_outputs']}")
    if not float(out["learning_rate"]) > 0.0:
        raise Go2SimError(f"rnd_cfg: learning_rate must be > 0, got {out['learning_rate']}")
    out["weight_schedule"] = check_schedule(out["weight_schedule"])
    return out


def check_schedule(schedule):
    if schedule is None:
        return None
    mode = schedule.get("mode")
    if mode not in SCHEDULE_KEYS:
        raise Go2SimError(f"rnd_cfg: unknown weight_schedule mode {mode!r}; the modes are {sorted(SCHEDULE_KEYS)}")
    missing = sorted(SCHEDULE_KEYS[mode] - set(schedule))
    extra = sorted(set(schedule) - SCHEDULE_KEYS[mode] - {"mode"})
    if missing or extra:
        raise Go2SimError(f"rnd_cfg: weight_schedule mode {mode!r} takes {sorted(SCHEDULE_KEYS[mode])}; missing {missing}, unexpected {extra}")
    if mode == "linear" and not schedule["final_step"] > schedule["initial_step"]:
        raise Go2SimError("rnd_cfg: a linear weight_schedule needs final_step > initial_step")
    return dict(schedule)


def rnd_weight(w0, schedule, counter):
    """w(counter) of the law, in float64"""
    w0 = float(w0)
    mode = "constant" if schedule is None else schedule["mode"]
    if mode == "constant":
        return w0
    v = float(schedule["final_value"])
    if mode == "step":
        return v if counter >= schedule["final_step"] else w0
    a, b = schedule["initial_step"], schedule["final_step"]
    if counter < a:
        return w0
    if counter > b:
        return v
    return w0 + (v - w0) * (counter - a) / (b - a)


def rnd_dims(num_states, hidden_dims, num_outputs):
    """layer sizes of one network: a hidden width of -1 means num_states"""
    return [int(num_states), *[int(num_states) if int(d) == -1 else int(d) for d in hidden_dims], int(num_outputs)]


def rnd_init(pdims, tdims, seed):
    """the two networks' initial tensors: nn.Linear's default init, the predictor from `seed`, the target from a purpose of its own"""
    sd = linear_init(torch.Generator().manual_seed(int(seed)), "predictor", pdims)
    sd.update(linear_init(torch.Generator().manual_seed(int(seed) + TARGET_SEED_PURPOSE), "target", tdims))
    return sd


# ---- the trainer handle --------------------------------------------------------------------------------------------------------------------------
class RndHandle(TrainerHandle):
    """One go2sim_rnd handle: pointers only.  `predictor` / `target` are policy.Mlp objects of the product library."""

    def __init__(self, lib, predictor, target, max_rows, *, learning_rate=1e-3, reward_normalization=False, betas=(0.9, 0.999), eps=1e-8, device=None):
        TrainerHandle.__init__(self, lib, "rnd", device)
        self.predictor, self.target, self.max_rows = predictor, target, int(max_rows)
        cfg = RndCfg(float(learning_rate), betas[0], betas[1], eps, int(bool(reward_normalization)))
        h = ctypes.c_void_p()
        lib.check(lib.fn("rnd_create")(predictor.h, target.h, ctypes.byref(cfg), ctypes.c_int(self.max_rows), ctypes.byref(h)), "rnd_create")
        self._created(h)
        self.n_outputs = predictor.dims[-1]

    def step(self, s, rewards, weight, intrinsic, rewards_total, n_rows=None):
        n = s.shape[0] if n_rows is None else n_rows
        self._call("step", _ptr(s), _ptr(rewards), ctypes.c_int(n), ctypes.c_double(float(weight)), _ptr(intrinsic), _ptr(rewards_total))

    def last_step(self, n_rows):
        """(target embedding, predictor embedding, r before the reward normaliser) of the last step: device copies"""
        t, p = (torch.empty(n_rows, self.n_outputs, device=self.device) for _ in range(2))
        r = torch.empty(n_rows, device=self.device)
        self._call("last_step", _ptr(t), _ptr(p), _ptr(r), ctypes.c_int(n_rows))
        return t, p, r

    def minibatch_grad(self, s, idx, n_rows=None):
        self._call("minibatch_grad", _ptr(s), _ptr(idx), ctypes.c_int(idx.numel() if n_rows is None else n_rows))

    def apply(self):
        self._call("apply")

    def update(self, s, idx, n_rows_total, n_epochs, n_mini_batches):
        self._call("update", _ptr(s), _ptr(idx), ctypes.c_int(n_rows_total), ctypes.c_int(n_epochs), ctypes.c_int(n_mini_batches))

    def stats(self):
        """float64 device tensor [mean rnd loss, learning rate, grad norm, step, mini-batches, Adam steps]; no synchronisation"""
        return TrainerHandle.stats(self)

    def get_reward_state(self, n_avg):
        """-> (mean, var, std as numpy float32 scalars, count, avg[n_avg] as a numpy array); waits for the stream"""
        m, v, s = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        cnt = ctypes.c_int64()
        avg = np.zeros(int(n_avg), np.float32)
        self._call("get_reward_state", ctypes.byref(m), ctypes.byref(v), ctypes.byref(s), ctypes.byref(cnt), avg.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(int(n_avg)))
        return np.float32(m.value), np.float32(v.value), np.float32(s.value), int(cnt.value), avg

    def set_reward_state(self, mean, var, std, count, avg):
        avg = np.ascontiguousarray(avg, dtype=np.float32).reshape(-1)
        self._call("set_reward_state", ctypes.c_float(float(mean)), ctypes.c_float(float(var)), ctypes.c_float(float(std)), ctypes.c_int64(int(count)),
                   avg.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(avg.size))


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------
class RandomNetworkDistillation(OptimizerState):
    def __init__(self, num_states, num_outputs=1, predictor_hidden_dims=(-1,), target_hidden_dims=(-1,), activation="elu", weight=0.0, state_normalization=False,
                 reward_normalization=False, weight_schedule=None, learning_rate=1e-3, *, device=None, seed=1):
        from .normalization import EmpiricalNormalization
        from .policy import Mlp, flatten_sequential, resolve_activation       # policy.py imports ppo.py, which imports this module

        self.activation = resolve_activation(activation)                          # refused before the device is touched
        self.weight_schedule = check_schedule(weight_schedule)
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_states, self.num_outputs = int(num_states), int(num_outputs)
        self.pdims = rnd_dims(num_states, predictor_hidden_dims, num_outputs)
        self.tdims = rnd_dims(num_states, target_hidden_dims, num_outputs)
        self.initial_weight = float(weight)
        self.reward_normalization, self.state_normalization = bool(reward_normalization), bool(state_normalization)
        self.learning_rate = float(learning_rate)
        self.update_counter, self.weight = 0, float(weight)
        self._L = load_hip_lib()
        sd = rnd_init(self.pdims, self.tdims, seed)
        dev_index = self.device.index or 0
        self._predictor = Mlp(self._L, self.pdims, flatten_sequential(sd, "predictor", len(self.pdims) - 1)[0], dev_index, self.activation)
        self._target = Mlp(self._L, self.tdims, flatten_sequential(sd, "target", len(self.tdims) - 1)[0], dev_index, self.activation)
        self._target_host = {k: sd[k].clone() for k, _ in mlp_keys("target", self.tdims)}
        self._initial_predictor = {k: sd[k].clone() for k, _ in mlp_keys("predictor", self.pdims)}
        self.state_normalizer = EmpiricalNormalization([self.num_states], eps=STATE_EPS, until=UNTIL, device=self.device) if self.state_normalization else None
        self._h = None
        self._bufs = {}
        self.last_state = self.intrinsic = self.rewards_total = None
        self._n_avg = 0

    def attach(self, max_rows):
        """The go2sim_rnd handle, sized for steps and mini-batches of up to max_rows rows; the optimizer state and the reward normaliser live in it."""
        if self._h is not None:
            raise Go2SimError("RandomNetworkDistillation.attach: the handle exists already")
        self._h = RndHandle(self._L, self._predictor, self._target, max_rows, learning_rate=self.learning_rate, reward_normalization=self.reward_normalization,
                            device=self.device)
        return self._h

    def _buf(self, name, n):
        t = self._bufs.get(name)
        if t is None or t.shape[0] != n:
            t = self._bufs[name] = torch.empty(n, device=self.device, dtype=torch.float32)
        return t

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the env step --------------------------------------------------------------------------------
    def get_intrinsic_reward(self, rnd_state, rewards):
        """Items 1 to 7 of the law: -> (intrinsic, rewards_total), buffers of the module's own that the next call overwrites; `rewards` is not written.
        ``last_state`` holds the rows the update reads."""
        from .normalization import norm_step

        if self._h is None:
            raise Go2SimError("get_intrinsic_reward: attach(max_rows) first (PPO.init_storage does)")
        self.update_counter += 1
        s = rnd_state.to(device=self.device, dtype=torch.float32)
        if s.dim() != 2 or s.shape[1] != self.num_states:
            raise Go2SimError(f"rnd_state has shape {tuple(s.shape)}, the networks read [.][{self.num_states}]")
        s = norm_step(self.state_normalizer, s, update=True)[0] if self.state_normalizer is not None else s.contiguous()
        n = s.shape[0]
        rew = rewards.reshape(n).to(device=self.device, dtype=torch.float32).contiguous()
        self.weight = rnd_weight(self.initial_weight, self.weight_schedule, self.update_counter)
        self.intrinsic, self.rewards_total = self._buf("intrinsic", n), self._buf("rewards_total", n)
        self._h.step(s, rew, self.weight, self.intrinsic, self.rewards_total, n)
        self.last_state, self._n_avg = s, n
        return self.intrinsic, self.rewards_total

    # ---- the update ----------------------------------------------------------------------------------
    def update(self, states, idx, n_rows_total, n_epochs, n_mini_batches):
        """The predictor's loop over the mini-batches idx[i mbs .. (i + 1) mbs) of every epoch; -> the handle's statistics (device, float64)"""
        self._h.update(states, idx, int(n_rows_total), int(n_epochs), int(n_mini_batches))
        return self._h.stats()

    # ---- state -------------------------------------------------------------------------------------------
    def state_dict(self):
        out = {k: v.clone() for k, v in self._initial_predictor.items()}
        if self._h is not None:
            out = unflatten_keys(self._h.export("PARAMS").cpu(), mlp_keys("predictor", self.pdims))
        out.update({k: v.clone() for k, v in self._target_host.items()})
        if self.state_normalizer is not None:
            out.update({"state_normalizer." + k: v for k, v in self.state_normalizer.state_dict().items()})
        if self.reward_normalization and self._h is not None:
            m, v, s, cnt, avg = self._h.get_reward_state(self._n_avg)
            f = lambda x: torch.tensor([[x]], dtype=torch.float32)
            out.update({"reward_normalizer.emp_norm._mean": f(m), "reward_normalizer.emp_norm._var": f(v), "reward_normalizer.emp_norm._std": f(s),
                        "reward_normalizer.emp_norm.count": torch.tensor(cnt, dtype=torch.long), "reward_normalizer.disc_avg.avg": torch.from_numpy(avg.copy())})
        return out

    def load_state_dict(self, sd, strict=True):
        from .policy import flatten_sequential

        if self._h is None:
            raise Go2SimError("load_state_dict: attach(max_rows) first (PPO.init_storage does)")
        for prefix, dims in (("predictor", self.pdims), ("target", self.tdims)):
            missing = [k for k, _ in mlp_keys(prefix, dims) if k not in sd]
            if missing:
                raise Go2SimError(f"rnd state dict lacks {missing}")
            flat, got = flatten_sequential(sd, prefix, len(dims) - 1)
            if list(got) != list(dims):
                raise Go2SimError(f"rnd state dict has {prefix} layer sizes {got}, this module's are {dims}")
            if prefix == "predictor":
                self._h.import_("PARAMS", torch.from_numpy(flat))
            else:
                self._target.set_params(flat)
                torch.cuda.synchronize(self.device)
                self._target_host = {k: sd[k].detach().cpu().clone() for k, _ in mlp_keys("target", dims)}
        has_state = any(k.startswith("state_normalizer.") for k in sd)
        has_reward = any(k.startswith("reward_normalizer.") for k in sd)
        if has_state != (self.state_normalizer is not None) or has_reward != self.reward_normalization:
            raise Go2SimError(f"rnd state dict: state_normalizer keys {'present' if has_state else 'absent'}, reward_normalizer keys {'present' if has_reward else 'absent'}; "
                              f"this module has state_normalization={self.state_normalization}, reward_normalization={self.reward_normalization}")
        if has_state:
            self.state_normalizer.load_state_dict({k[len("state_normalizer."):]: v for k, v in sd.items() if k.startswith("state_normalizer.")})
        if has_reward:
            g = lambda k: float(sd["reward_normalizer.emp_norm." + k].reshape(-1)[0])
            avg = sd["reward_normalizer.disc_avg.avg"].detach().cpu().to(torch.float32).numpy()
            self._h.set_reward_state(g("_mean"), g("_var"), g("_std"), int(sd["reward_normalizer.emp_norm.count"]), avg)
            self._n_avg = avg.size
        return True

    def optimizer_state_dict(self):
        return dict(OptimizerState.optimizer_state_dict(self), update_counter=int(self.update_counter))

    def load_optimizer_state_dict(self, sd):
        OptimizerState.load_optimizer_state_dict(self, sd)
        self.update_counter = int(sd.get("update_counter", 0))
        self.weight = rnd_weight(self.initial_weight, self.weight_schedule, self.update_counter)
