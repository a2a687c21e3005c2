"""What the update handles and algorithms of ppo.py and distillation.py share on the host: the handle surface that include/go2sim_train.h and
include/go2sim_distill.h spell alike (sizes, flat and padded exports, the step count, the statistics) and the optimizer-state checkpoint entries.  The
state-dict key lists of the flat vectors are module_core.py's.  The device side of the same sharing is csrc/go2sim_trainer_host.h."""
import ctypes

import torch

from .capi import C, Go2SimError, Handle, _ptr


class TrainerHandle(Handle):
    """The common part of a go2sim_ppo / go2sim_distill handle.  `prefix` ("ppo" / "distill") names the entry points go2sim_<prefix>_* and the constants
    GO2SIM_<PREFIX>_*.  A subclass creates the handle and passes it to _created."""

    def __init__(self, lib, prefix, device):
        Handle.__init__(self, lib, prefix + "_destroy")
        self.L, self._prefix = lib, prefix
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())

    def _const(self, name):
        return C[f"GO2SIM_{self._prefix.upper()}_{name}"]

    def _created(self, h):
        self.h = h
        n = ctypes.c_size_t()
        for what in ("n_params", "n_padded"):
            self.L.check(self.L.fn(f"{self._prefix}_{what}")(self.h, ctypes.byref(n)), f"{self._prefix}_{what}")
            setattr(self, what, n.value)
        self._stats = torch.zeros(self._const("N_STATS"), dtype=torch.float64, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """go2sim_<prefix>_<name>(handle, *args, stream)"""
        self.L.check(self.L.fn(f"{self._prefix}_{name}")(self.h, *args, self._stream()), f"{self._prefix}_{name}")

    def export(self, which, *std):
        out = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        self._call("export", ctypes.c_int(self._const(which)), _ptr(out), *[_ptr(s) for s in std])
        return out

    def import_(self, which, flat, *std):
        flat = flat.to(device=self.device, dtype=torch.float32).contiguous()
        if flat.numel() != self.n_params:
            raise Go2SimError(f"flat vector has {flat.numel()} entries, expected {self.n_params}")
        self._call("import", ctypes.c_int(self._const(which)), _ptr(flat), *[_ptr(s) for s in std])
        torch.cuda.current_stream(self.device).synchronize()          # `flat` may be a temporary

    def export_padded(self, which):
        out = torch.empty(self.n_padded, dtype=torch.float32, device=self.device)
        self._call("export_padded", ctypes.c_int(self._const(which)), _ptr(out))
        return out

    def set_step(self, step, learning_rate):
        self._call("set_step", ctypes.c_longlong(int(step)), ctypes.c_double(float(learning_rate)))

    def reset_stats(self):
        self._call("reset_stats")

    def stats(self):
        """float64 device tensor of the handle's statistics (GO2SIM_<PREFIX>_ST_*); no synchronisation"""
        self._call("stats", _ptr(self._stats))
        return self._stats


class OptimizerState:
    """The optimizer part of a runner checkpoint, for an algorithm whose trainer handle is `self._h`."""

    def optimizer_state_dict(self):
        s = self._h.stats().cpu()
        return {"exp_avg": self._h.export("ADAM_M").cpu(), "exp_avg_sq": self._h.export("ADAM_V").cpu(), "step": int(s[self._h._const("ST_STEP")]),
                "lr": float(s[self._h._const("ST_LR")])}

    def load_optimizer_state_dict(self, sd):
        self._h.import_("ADAM_M", sd["exp_avg"]); self._h.import_("ADAM_V", sd["exp_avg_sq"])
        self._h.set_step(int(sd["step"]), float(sd["lr"]))
        self.learning_rate = float(sd["lr"])
