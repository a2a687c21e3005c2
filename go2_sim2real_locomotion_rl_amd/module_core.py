"""What the four policy modules (policy.ActorCritic / ActorCriticRecurrent, distillation.StudentTeacher / StudentTeacherRecurrent) share on the host:
the state-dict key lists, the constructors' initial draws as pure functions of (sizes, init_noise_std, seed), the state of one LSTM memory between cell
launches (`MemoryState`) and the base class `PolicyModule`.  The handles themselves (policy.Mlp, policy.Lstm) and the launches stay where they were; what
a new module has to supply is listed in DESIGN.md "Host modules"."""
import torch

from .capi import C, Go2SimError, load_hip_lib


# ---- key lists (state-dict and flat order) -----------------------------------------------------------------------------------------------------------
def mlp_keys(prefix, dims):
    """[(key, shape)] of one network in state-dict (and flat) order"""
    keys = []
    for l in range(len(dims) - 1):
        keys += [(f"{prefix}.{2 * l}.weight", (dims[l + 1], dims[l])), (f"{prefix}.{2 * l}.bias", (dims[l + 1],))]
    return keys


def lstm_shapes(n_in, n_hidden):
    """[(key suffix, shape)] of one memory in state-dict (and flat) order"""
    return [("weight_ih_l0", (4 * n_hidden, n_in)), ("weight_hh_l0", (4 * n_hidden, n_hidden)), ("bias_ih_l0", (4 * n_hidden,)), ("bias_hh_l0", (4 * n_hidden,))]


LSTM_KEYS = tuple(k for k, _ in lstm_shapes(1, 1))


def memory_keys(prefix, n_in, n_hidden):
    """[(key, shape)] of one memory in state-dict (and flat) order"""
    return [(f"{prefix}.rnn.{k}", shape) for k, shape in lstm_shapes(n_in, n_hidden)]


def unflatten_keys(flat, keys):
    """a flat vector sliced by a [(key, shape)] list -> {key: tensor}"""
    out, o = {}, 0
    for k, shape in keys:
        n = 1
        for s in shape:
            n *= s
        out[k] = flat[o:o + n].reshape(shape).clone()
        o += n
    return out


# ---- the constructors' initial state (no device) --------------------------------------------------------------------------------------------------------
def linear_init(generator, prefix, dims):
    """nn.Linear's default init (kaiming_uniform(a=sqrt 5)) of ``prefix.{0,2,..}``: per layer the weight, then the bias, uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in))"""
    sd = {}
    for l in range(len(dims) - 1):
        bound = 1.0 / (dims[l] ** 0.5)
        sd[f"{prefix}.{2 * l}.weight"] = (torch.rand(dims[l + 1], dims[l], generator=generator) * 2 - 1) * bound
        sd[f"{prefix}.{2 * l}.bias"] = (torch.rand(dims[l + 1], generator=generator) * 2 - 1) * bound
    return sd


def lstm_init(generator, prefix, n_in, n_hidden):
    """nn.LSTM's default init of ``prefix.rnn.*``: every tensor uniform(-1 / sqrt(H), 1 / sqrt(H))"""
    return {k: (torch.rand(*shape, generator=generator) * 2 - 1) / (n_hidden ** 0.5) for k, shape in memory_keys(prefix, n_in, n_hidden)}


def _initial_state(networks, memories, init_noise_std, seed):
    """networks: [(prefix, dims)] drawn in order from a generator seeded `seed`; memories: [(prefix, (n_in, H) or None)] from one seeded `seed + 0x5eed`"""
    sd, g = {}, torch.Generator().manual_seed(int(seed))
    for prefix, dims in networks:
        sd.update(linear_init(g, prefix, dims))
    g = torch.Generator().manual_seed(int(seed) + 0x5eed)
    for prefix, mem in memories:
        if mem is not None:
            sd.update(lstm_init(g, prefix, *mem))
    sd["std"] = float(init_noise_std) * torch.ones(networks[0][1][-1])
    return sd


def actor_critic_init(adims, cdims, init_noise_std, seed):
    return _initial_state([("actor", adims), ("critic", cdims)], [], init_noise_std, seed)


def actor_critic_recurrent_init(adims, cdims, mdims, init_noise_std, seed):
    return _initial_state([("actor", adims), ("critic", cdims)], [("memory_a", mdims[0]), ("memory_c", mdims[1])], init_noise_std, seed)


def student_teacher_init(sdims, tdims, init_noise_std, seed):
    return _initial_state([("student", sdims), ("teacher", tdims)], [], init_noise_std, seed)


def student_teacher_recurrent_init(sdims, tdims, smem, tmem, init_noise_std, seed):
    """tmem None: a teacher without a memory"""
    return _initial_state([("student", sdims), ("teacher", tdims)], [("memory_s", smem), ("memory_t", tmem)], init_noise_std, seed)


def check_lstm_config(cls, rnn_type, rnn_num_layers, width, key):
    """The one refusal of a memory's config, for the class named `cls`; `key` names the width in the config.  -> the width"""
    if str(rnn_type).lower() != "lstm":
        raise Go2SimError(f"{cls}'s memories are LSTMs; rnn_type {rnn_type!r} is not implemented")
    if int(rnn_num_layers) != 1:
        raise Go2SimError(f"{cls}'s memories have one LSTM layer, got rnn_num_layers = {rnn_num_layers}")
    if int(width) < 1 or int(width) > C["GO2SIM_MLP_MAX_WIDTH"]:
        raise Go2SimError(f"{cls}: {key} must be in 1 .. {C['GO2SIM_MLP_MAX_WIDTH']} (GO2SIM_MLP_MAX_WIDTH), got {width}")
    return int(width)


# ---- one memory's state -----------------------------------------------------------------------------------------------------------------------------------
class MemoryState:
    """[h, c, spare h] of one LSTM memory for B rows, on any torch device.  A cell launch reads (h, c) and writes (spare, c): `advance` hands these out
    and makes the spare buffer the state.  The rows of the done envs are zeroed either at once (`zero`) or by the next cell launch, which takes the mask
    as its `reset` argument (`pending`, `take_pending`); a reader of the state that is not the cell launch sees a pending mask applied."""

    def __init__(self, n_hidden, device):
        self.H, self.device, self.B, self.pending = int(n_hidden), device, 0, None
        self._hcs = None

    def rows(self, B):
        """the state for B rows: another B allocates afresh, zero and with no pending mask"""
        if self.B != B:
            self._hcs = [torch.zeros(B, self.H, device=self.device, dtype=torch.float32) for _ in range(3)]
            self.B, self.pending = B, None
        return self

    @property
    def h(self):
        return self._hcs[0]

    @property
    def c(self):
        return self._hcs[1]

    def advance(self):
        """-> (h_in, c_in, h_out, c_out) of the next cell step (c in place, h_out is never h_in); the step's h' is the state from here on"""
        h, c, spare = self._hcs
        self._hcs = [spare, c, h]
        return h, c, spare, c

    def zero(self, mask=None):
        """h = c = 0 now, in the rows where `mask` ([B], any dtype) is nonzero; without a mask everywhere, and a pending mask is dropped"""
        if self.B == 0:
            return
        for t in self._hcs[:2]:
            if mask is None:
                t.zero_()
            else:
                t.masked_fill_((mask.reshape(-1, 1) != 0).to(t.device), 0.0)
        if mask is None:
            self.pending = None

    def take_pending(self):
        """the pending mask, for the cell launch that applies it"""
        mask, self.pending = self.pending, None
        return mask

    def apply_pending(self):
        """the deferred zeroing done now, for a reader that is not the cell launch"""
        if self.pending is not None:
            self.zero(self.take_pending())

    def defer(self, mask):
        """`mask` zeroes its rows when the next step enters them; a mask still pending (two resets without a step between them) is applied first"""
        self.apply_pending()
        self.pending = mask

    def copy_entering(self, h_out, c_out):
        """the state as the next step enters it (pending mask applied), copied into the caller's arrays; the live state is not written"""
        h_out.copy_(self.h); c_out.copy_(self.c)
        if self.pending is not None:
            for t in (h_out, c_out):
                t.masked_fill_(self.pending.reshape(-1, 1) != 0, 0.0)

    def replace(self, h, c):
        """(h, c) of any shape with B x H entries become the state"""
        self.rows(h.reshape(-1, self.H).shape[0])
        self.h.copy_(h.reshape(self.h.shape)); self.c.copy_(c.reshape(self.c.shape))
        self.pending = None

    def views(self):
        """(h, c), each [1][B][H] as nn.LSTM shapes them: views of the live state, a pending mask applied"""
        self.apply_pending()
        return self.h.unsqueeze(0), self.c.unsqueeze(0)


def hidden_state_views(states):
    """get_hidden_states of a module whose memories' states are `states` (None: no such memory): (None, None) before the first step"""
    if states[0].B == 0:
        return None, None
    return tuple(None if s is None else s.views() for s in states)


# ---- the base class ---------------------------------------------------------------------------------------------------------------------------------------
class PolicyModule:
    """The device set-up, the output buffers, the noise counter and the create-or-set of the parts of a module.  A subclass lists its parts
    for `_set_parts`, refuses what its config cannot be, and launches."""
    is_recurrent = False

    def __init__(self, num_actions, device, seed):
        if not torch.cuda.is_available():
            raise Go2SimError("no ROCm GPU visible: the go2sim product path has no CPU fallback")
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_actions = int(num_actions)
        self._L = load_hip_lib()
        self.std = torch.ones(self.num_actions, device=self.device)         # the device tensor the update kernels write: only ever copied into
        self._seed, self._step = int(seed), 0
        self._bufs, self._host, self._trainer, self._mean = {}, {}, None, None

    @property
    def noise_step(self):
        """the `step` of the Philox stream (seed, row, step) the next sampling launch draws from; a checkpoint carries it"""
        return self._step

    @noise_step.setter
    def noise_step(self, step):
        self._step = int(step)

    def _set_parts(self, parts, sd):
        """Create-or-set of the handles `self.<attr>` from ``sd[prefix.*]``, for `parts` = [(attr, kind, prefix, sizes)]: kind "mlp" is a policy.Mlp with
        the layer sizes `sizes`, kind "lstm" a policy.Lstm with (n_in, H); sizes None (a memory the module does not have) is skipped.  Every part's sizes are
        checked before the first is written, and a host copy of the tensors is kept."""
        from .policy import Lstm, Mlp, flatten_lstm, flatten_sequential         # policy.py imports this module

        todo = []
        for attr, kind, prefix, sizes in parts:
            if sizes is None:
                continue
            is_mlp = kind == "mlp"
            flat, got = flatten_sequential(sd, prefix, len(sizes) - 1) if is_mlp else flatten_lstm(sd, prefix)
            if tuple(got) != tuple(sizes):
                raise Go2SimError(f"state dict has {prefix} {'layer ' if is_mlp else ''}sizes {got}, this model's are {sizes}")
            todo.append((attr, is_mlp, flat, sizes, mlp_keys(prefix, sizes) if is_mlp else memory_keys(prefix, *sizes)))
        for attr, is_mlp, flat, sizes, keys in todo:
            if getattr(self, attr, None) is not None:
                getattr(self, attr).set_params(flat)
            elif is_mlp:
                setattr(self, attr, Mlp(self._L, list(sizes), flat, self.device.index or 0, self.activation))
            else:
                setattr(self, attr, Lstm(self._L, *sizes, flat, self.device.index or 0))
            self._host.update({k: sd[k].detach().clone() for k, _ in keys})

    def _set_std(self, sd):
        self.std.copy_(sd["std"].detach().reshape(self.num_actions))

    def _host_state(self):
        """the host copies of the parts as last loaded, and std as it is on the device"""
        return {**{k: v.clone() for k, v in self._host.items()}, "std": self.std.detach().cpu().clone()}

    def _buf(self, name, shape):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(*shape, device=self.device, dtype=torch.float32)
            self._bufs[name] = t
        return t

    @property
    def action_mean(self):
        return self._mean

    @property
    def action_std(self):
        return self.std.expand_as(self._mean)

    def reset(self, dones=None, hidden_states=None):
        pass
