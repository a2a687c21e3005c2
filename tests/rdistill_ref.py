"""The recurrent branch of rsl_rl's distillation update (algorithms.Distillation + modules.StudentTeacherRecurrent, 2.3) restated literally in torch on the
CPU, as include/go2sim_rdistill.h states it: nn.LSTM, nn.Sequential(Linear, ELU, ...), nn.functional.mse_loss / huber_loss, autograd with the detaches
written out, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam.  In float64 it is the reference of the HIP update; the same functions in float32 are the
yardstick its error is measured with.  It shares no code with the product: the window schedule is the literal loop of the header (cnt % G), not
rdistill_schedule, which tests/test_rdistill_ref.py checks against hand-written lists.

`uncut` (None, "done", "epoch", "first") lets the gradient through one of the three places where the law cuts it; tests/rdistill_cases.py uses it to show
that each cut matters to the gradient by far more than the bound the GPU test applies."""
import torch
from torch import nn

from distill_ref import LOSS, mlp

HP = dict(learning_rate=1e-3, max_grad_norm=None, loss_type="mse")
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


class Memory(nn.Module):
    def __init__(self, n_in, n_hidden):
        super().__init__()
        self.rnn = nn.LSTM(n_in, n_hidden, 1)


class Model(nn.Module):
    """the trained half of rsl_rl.modules.StudentTeacherRecurrent: state-dict keys memory_s.rnn.*, student.{0,2,..}.{weight,bias}"""

    def __init__(self, n_in, sdims):
        super().__init__()
        self.n_in, self.sdims = int(n_in), list(sdims)
        self.memory_s, self.student = Memory(n_in, sdims[0]), mlp(sdims)


def ordered_params(model):
    """[(key, parameter)] in the flat order of go2sim_rdistill_export: student W0, b0, ..., memory_s weight_ih, weight_hh, bias_ih, bias_hh"""
    named = dict(model.named_parameters())
    keys = []
    for l in range(len(model.sdims) - 1):
        keys += [f"student.{2 * l}.weight", f"student.{2 * l}.bias"]
    keys += [f"memory_s.rnn.{k}" for k in LSTM_KEYS]
    return [(k, named[k]) for k in keys]


def make_model(n_in, sdims, state, dtype):
    m = Model(n_in, sdims).to(dtype)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(state[k].to(dtype))
    return m


def cell(model, x, h, c):
    """one step of memory_s on x [N][I] from (h, c) [N][H]"""
    _, (h1, c1) = model.memory_s.rnn(x.unsqueeze(0), (h.unsqueeze(0).contiguous(), c.unsqueeze(0).contiguous()))
    return h1[0], c1[0]


def masked(s, done, through=False):
    """the state entering the next step: 0 for the done envs.  `through`: the same values, with the gradient let through the mask"""
    m = s * (1.0 - done.to(s.dtype)).unsqueeze(1)
    return m.detach() + (s - s.detach()) if through else m


def window_grad(model, obs, ta, dones, S, carried, segs, loss_type, uncut=None, before=None):
    """One window of segments (t0, n).  A segment with t0 = 0 starts from S, the first segment with t0 > 0 from `carried` masked by dones[t0 - 1].
    -> ({key: grad}, [l_t], means [pairs][N][A], (h, c) after the last step with its dones applied).
    uncut = "first": `carried` is ignored and recomputed from S through the steps before t0 with the graph kept."""
    for p in model.parameters():
        p.grad = None
    losses, means = [], []
    h = c = None
    for k, (t0, n) in enumerate(segs):
        if t0 == 0:
            if uncut == "epoch" and k > 0:
                h, c = S[0] + (h - h.detach()), S[1] + (c - c.detach())
            else:
                h, c = S
        else:
            assert k == 0
            if uncut == "first":
                h, c = S
                for t in range(t0):
                    h, c = cell(model, obs[t], h, c)
                    h, c = masked(h, dones[t]), masked(c, dones[t])
            else:
                h, c = masked(carried[0], dones[t0 - 1]), masked(carried[1], dones[t0 - 1])
        for t in range(t0, t0 + n):
            h, c = cell(model, obs[t], h, c)
            mu = model.student(h)
            means.append(mu.detach().clone())
            losses.append(LOSS[loss_type](mu, ta[t]))
            h, c = masked(h, dones[t], uncut == "done"), masked(c, dones[t], uncut == "done")
    sum(losses).backward()
    return {k: p.grad.detach().clone() for k, p in ordered_params(model)}, [float(l.detach()) for l in losses], torch.stack(means), (h.detach().clone(), c.detach().clone())


def update(model, obs, ta, dones, S, n_epochs, gradient_length, hp=HP):
    """Distillation.update, recurrent branch: -> dict(loss, norms of every window before the clip, state (h, c) after the update, margin: the smallest
    distance of a residual from Huber's branch over all pairs).  `model` is updated in place."""
    T = obs.shape[0]
    params = [p for _, p in ordered_params(model)]
    opt = torch.optim.Adam(params, lr=hp["learning_rate"])
    cnt, total, norms, window, margin = 0, 0.0, [], [], float("inf")
    h = c = None
    for _ in range(n_epochs):
        h, c = S                                               # constants: no gradient flows into the first step of an epoch
        for t in range(T):
            h, c = cell(model, obs[t], h, c)
            mu = model.student(h)
            margin = min(margin, float(((mu.detach() - ta[t]).abs() - 1.0).abs().min()))
            window.append(LOSS[hp["loss_type"]](mu, ta[t]))
            cnt += 1
            if cnt % gradient_length == 0:
                opt.zero_grad()
                sum(window).backward()
                norms.append(float(torch.cat([p.grad.reshape(-1) for p in params]).norm()))
                if hp["max_grad_norm"] is not None:
                    nn.utils.clip_grad_norm_(params, hp["max_grad_norm"])
                opt.step()
                total += sum(float(l.detach()) for l in window)
                window = []
                h, c = h.detach(), c.detach()                  # the forward state is carried on, the gradient is not
            h, c = masked(h, dones[t]), masked(c, dones[t])
    total += sum(float(l.detach()) for l in window)            # the dropped tail: reported, no gradient
    return dict(loss=total / (n_epochs * T), norms=norms, state=(h.detach().clone(), c.detach().clone()), margin=margin)
