"""EmpiricalNormalization -- ``rsl_rl.modules.EmpiricalNormalization`` (rsl-rl-lib==2.2.4) on the normaliser entry points of the C ABI
(include/go2sim_norm.h): running column mean and variance of the observations, ``y = (x - mean) / (std + eps)``.

    norm = EmpiricalNormalization(49, until=1e8)
    y = norm(obs)                     # training mode: fold the batch into the statistics, then normalise (two launches)
    norm.eval(); y = norm(obs)        # normalise only (one launch)
    y_a, y_c = norm_step(norm_a, obs, norm_c, critic_obs)     # both observation sets of an env step in the same two launches

The statistics live on the device; ``state_dict()`` has rsl_rl's keys and shapes (``_mean``, ``_var``, ``_std`` float32 ``[1, d]``, ``count`` an int64
scalar), so a checkpoint's ``obs_norm_state_dict`` loads as it is.  ``forward`` returns a buffer of the normaliser's own that the next call overwrites;
the input is never modified.  With a process group ``norm_step`` is the sharded form: every rank's float64 moments record, one all-gather, the records
folded in rank order -- every rank holds the same bits and ``count`` is the global row count.
"""
import ctypes

import numpy as np
import torch

from .capi import Go2SimError, Handle, _ptr, load_hip_lib
from .distributed import allgather_records, is_multi


class EmpiricalNormalization(Handle):
    def __init__(self, shape, eps=1e-2, until=None, *, device=None):
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        self.d = int(np.prod(self.shape))
        self.eps, self.until = float(eps), until
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.training = True
        self._L = load_hip_lib()
        Handle.__init__(self, self._L, "norm_destroy")
        self._bufs = {}
        h = ctypes.c_void_p()
        self._L.check(self._L.fn("norm_create")(ctypes.c_int(self.device.index or 0), ctypes.c_int(self.d), ctypes.c_double(self.eps),
                                                ctypes.c_double(0.0 if until is None else float(until)), ctypes.byref(h)), "norm_create")
        self.h = h

    # ---- rsl_rl's module surface -----------------------------------------------------------------------
    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _in(self, x):
        x = x.to(device=self.device, dtype=torch.float32)
        if x.dim() < 1 or (x.shape[-1] != self.d and tuple(x.shape[1:]) != self.shape):
            raise Go2SimError(f"expected rows of {self.d} features, got {tuple(x.shape)}")
        return x.reshape(-1, self.d).contiguous()

    def _out(self, n_rows, name="y"):
        t = self._bufs.get(name)
        if t is None or t.shape[0] != n_rows:
            t = self._bufs[name] = torch.empty(n_rows, self.d, device=self.device, dtype=torch.float32)
        return t

    def forward(self, x):
        return norm_step(self, x)[0].view(x.shape)

    __call__ = forward

    def update(self, x):
        """Fold the batch into the statistics (unless ``count >= until``); the normalised rows go to a scratch buffer."""
        x = self._in(x)
        self._L.check(self._L.fn("norm_step")(self.h, _ptr(x), _ptr(self._out(x.shape[0], "scratch")), None, None, None, ctypes.c_int(x.shape[0]), ctypes.c_int(1),
                                              self._stream()), "norm_step")

    def inverse(self, y):
        sd = self.state_dict()
        return y * (sd["_std"].to(y.device) + np.float32(self.eps)) + sd["_mean"].to(y.device)

    @property
    def mean(self):
        return self.state_dict()["_mean"].squeeze(0).to(self.device)

    @property
    def std(self):
        return self.state_dict()["_std"].squeeze(0).to(self.device)

    @property
    def count(self):
        return self.state_dict()["count"]

    # ---- state (waits for the stream) -------------------------------------------------------------------
    def state_dict(self):
        mean, var, std = (np.empty(self.d, np.float32) for _ in range(3))
        cnt = ctypes.c_int64()
        self._L.check(self._L.fn("norm_get_state")(self.h, mean.ctypes.data_as(ctypes.c_void_p), var.ctypes.data_as(ctypes.c_void_p),
                                                   std.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt), self._stream()), "norm_get_state")
        return {"_mean": torch.from_numpy(mean).unsqueeze(0), "_var": torch.from_numpy(var).unsqueeze(0), "_std": torch.from_numpy(std).unsqueeze(0),
                "count": torch.tensor(cnt.value, dtype=torch.long)}

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in ("_mean", "_var", "_std", "count") if k not in state_dict]
        if missing:
            raise Go2SimError(f"normaliser state dict lacks {missing}")
        arrs = []
        for k in ("_mean", "_var", "_std"):
            t = torch.as_tensor(state_dict[k]).detach().cpu()
            if t.numel() != self.d:
                raise Go2SimError(f"normaliser state dict: {k} has {t.numel()} entries, expected {self.d}")
            arrs.append(np.ascontiguousarray(t.to(torch.float32).reshape(-1).numpy()))
        self._L.check(self._L.fn("norm_set_state")(self.h, *(a.ctypes.data_as(ctypes.c_void_p) for a in arrs), ctypes.c_int64(int(state_dict["count"])),
                                                   self._stream()), "norm_set_state")
        return True


def norm_step(norm_a, x_a, norm_b=None, x_b=None, update=None, group=None):
    """One step of one or two normalisers in the same launches: -> (y_a, y_b or None), ``[n_rows][d]`` buffers of the normalisers' own.  ``update=None``
    follows ``norm_a.training``.  With a process group of more than one rank the batch is this rank's shard: moments record, all-gather, merge in rank
    order (include/go2sim_norm.h)."""
    L = norm_a._L
    update = norm_a.training if update is None else bool(update)
    xa = norm_a._in(x_a)
    n = xa.shape[0]
    ya = norm_a._out(n)
    if xa.data_ptr() == ya.data_ptr():                                     # the caller handed the last output back in
        xa = xa.clone()
    xb = yb = None
    if norm_b is not None:
        xb = norm_b._in(x_b)
        if xb.shape[0] != n:
            raise Go2SimError(f"the two observation sets have {n} and {xb.shape[0]} rows")
        yb = norm_b._out(n)
        if xb.data_ptr() == yb.data_ptr():
            xb = xb.clone()
    hb = norm_b.h if norm_b is not None else None
    stream = norm_a._stream()
    if update and group is not None and is_multi(group):
        ln = ctypes.c_int()
        L.check(L.fn("norm_record_len")(norm_a.h, hb, ctypes.byref(ln)), "norm_record_len")
        rec = torch.empty(ln.value, dtype=torch.float64, device=norm_a.device)
        L.check(L.fn("norm_moments")(norm_a.h, _ptr(xa), hb, _ptr(xb), ctypes.c_int(n), _ptr(rec), stream), "norm_moments")
        recs = allgather_records(rec, group).contiguous()
        L.check(L.fn("norm_merge_step")(norm_a.h, _ptr(xa), _ptr(ya), hb, _ptr(xb), _ptr(yb), ctypes.c_int(n), _ptr(recs), ctypes.c_int(recs.shape[0]), ctypes.c_int(1), stream),
                "norm_merge_step")
    else:
        L.check(L.fn("norm_step")(norm_a.h, _ptr(xa), _ptr(ya), hb, _ptr(xb), _ptr(yb), ctypes.c_int(n), ctypes.c_int(int(update)), stream), "norm_step")
    return ya, yb
