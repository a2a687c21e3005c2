"""The distillation update of rsl_rl (algorithms.Distillation + modules.StudentTeacher, 2.3 on) restated literally in torch on the CPU: nn.Sequential(Linear,
ELU, ...), nn.functional.mse_loss / huber_loss, autograd, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam.  In float64 it is the reference of the HIP
update (include/go2sim_distill.h); the same functions in float32 are the yardstick its error is measured with.  The window schedule is the product's pure
function distill_windows (the device lists come from the same function); everything else shares no code with the product."""
import torch
from torch import nn

from go2_sim2real_locomotion_rl_amd.distillation import distill_windows

HP = dict(learning_rate=1e-3, max_grad_norm=None, loss_type="mse")
LOSS = {"mse": nn.functional.mse_loss, "huber": nn.functional.huber_loss}


def mlp(dims):
    layers = []
    for l in range(len(dims) - 1):
        layers.append(nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            layers.append(nn.ELU())
    return nn.Sequential(*layers)


class Model(nn.Module):
    """rsl_rl.modules.StudentTeacher: state-dict keys student.{0,2,..}.{weight,bias}, teacher.{0,2,..}.{weight,bias}, std (no gradient)"""

    def __init__(self, sdims, tdims):
        super().__init__()
        self.sdims, self.tdims = list(sdims), list(tdims)
        self.student, self.teacher = mlp(sdims), mlp(tdims)
        self.teacher.requires_grad_(False)
        self.std = nn.Parameter(torch.ones(sdims[-1]), requires_grad=False)


def ordered_params(model):
    """[(key, parameter)] of the student in the flat order of go2sim_distill_export: W0, b0, W1, b1, ..."""
    named = dict(model.named_parameters())
    out = []
    for l in range(len(model.sdims) - 1):
        out += [(f"student.{2 * l}.weight", named[f"student.{2 * l}.weight"]), (f"student.{2 * l}.bias", named[f"student.{2 * l}.bias"])]
    return out


def make_model(sdims, tdims, state, dtype):
    """A Model in `dtype` holding the float32-exact values of `state` (key -> tensor)."""
    m = Model(sdims, tdims).to(dtype)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(state[k].to(dtype))
    return m


def pair_loss(model, obs_t, teacher_actions_t, loss_type):
    """l_t: the mean over envs and actions of rho(student(obs_t) - teacher_actions_t)"""
    return LOSS[loss_type](model.student(obs_t), teacher_actions_t)


def window_grad(model, obs, teacher_actions, steps, loss_type):
    """obs [T][N][Ds], teacher_actions [T][N][A], `steps` the window's step indices (a step may appear twice).  -> ({key: grad}, [l_t])"""
    for p in model.parameters():
        p.grad = None
    losses = [pair_loss(model, obs[t], teacher_actions[t], loss_type) for t in steps]
    sum(losses).backward()
    return {k: p.grad.detach().clone() for k, p in ordered_params(model)}, [float(l.detach()) for l in losses]


def update(model, obs, teacher_actions, n_epochs, gradient_length, hp=HP):
    """Distillation.update: -> (mean_behavior_loss, [total gradient norm of every window before the clip]).  `model` is updated in place."""
    T = obs.shape[0]
    params = [p for _, p in ordered_params(model)]
    opt = torch.optim.Adam(params, lr=hp["learning_rate"])
    windows, tail = distill_windows(T, n_epochs, gradient_length)
    total, norms = 0.0, []
    for w in windows:
        losses = [pair_loss(model, obs[t], teacher_actions[t], hp["loss_type"]) for _, t in w]
        opt.zero_grad()
        sum(losses).backward()
        norms.append(float(torch.cat([p.grad.reshape(-1) for p in params]).norm()))
        if hp["max_grad_norm"] is not None:
            nn.utils.clip_grad_norm_(params, hp["max_grad_norm"])
        opt.step()
        total += sum(float(l.detach()) for l in losses)
    with torch.no_grad():
        for _, t in tail:                                   # the dropped tail is reported, under the final parameters, and gives no gradient
            total += float(pair_loss(model, obs[t], teacher_actions[t], hp["loss_type"]))
    return total / (n_epochs * T), norms
