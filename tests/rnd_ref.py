"""Random network distillation (include/go2sim_rnd.h states the law) restated in torch / numpy on the CPU.  In float64 it is the reference of the HIP
library's step and update; the same update in float32 is the yardstick its error is measured with.  The update is nn.Sequential + nn.functional.mse_loss +
autograd + torch.optim.Adam.  Nothing of the package under test is imported; tests/norm_ref.py supplies the fold of the reward normaliser and its bounds."""
import numpy as np
import torch
from torch import nn

import norm_ref as NR

ACTS = {"elu": nn.ELU, "selu": nn.SELU, "relu": nn.ReLU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "identity": nn.Identity}
GAMMA32 = np.float32(0.99)
UNTIL = 1.0e8
LR = 1e-3
CFG_KEYS = ("weight", "weight_schedule", "reward_normalization", "state_normalization", "num_outputs", "predictor_hidden_dims", "target_hidden_dims",
            "activation", "learning_rate")


def mlp(dims, act):
    layers = []
    for l in range(len(dims) - 1):
        layers.append(nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            layers.append(ACTS[act]())
    return nn.Sequential(*layers)


class Model(nn.Module):
    """state-dict keys predictor.{0,2,..}.{weight,bias}, target.{0,2,..}.{weight,bias}; the target has no gradient"""

    def __init__(self, pdims, tdims, act):
        super().__init__()
        self.pdims, self.tdims = list(pdims), list(tdims)
        self.predictor, self.target = mlp(pdims, act), mlp(tdims, act)
        self.target.requires_grad_(False)


def make_model(pdims, tdims, act, state, dtype):
    """A Model in `dtype` holding the float32-exact values of `state` (key -> tensor)."""
    m = Model(pdims, tdims, act).to(dtype)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(state[k].to(dtype))
    return m


def ordered_params(model):
    """[(key, parameter)] of the predictor in the flat order of go2sim_rnd_export: W0, b0, W1, b1, ..."""
    named = dict(model.named_parameters())
    out = []
    for l in range(len(model.pdims) - 1):
        out += [(f"predictor.{2 * l}.weight", named[f"predictor.{2 * l}.weight"]), (f"predictor.{2 * l}.bias", named[f"predictor.{2 * l}.bias"])]
    return out


def init_state(pdims, tdims, gen):
    """nn.Linear's default init (uniform +- 1 / sqrt(fan_in)) for both networks; float32"""
    sd = {}
    for prefix, dims in (("predictor", pdims), ("target", tdims)):
        for l in range(len(dims) - 1):
            bound = 1.0 / dims[l] ** 0.5
            sd[f"{prefix}.{2 * l}.weight"] = ((torch.rand(dims[l + 1], dims[l], generator=gen) * 2 - 1) * bound).float()
            sd[f"{prefix}.{2 * l}.bias"] = ((torch.rand(dims[l + 1], generator=gen) * 2 - 1) * bound).float()
    return sd


# ---- the update ----------------------------------------------------------------------------------------------------------------------------------------
def minibatch_loss(model, rows):
    """L = mean over rows and outputs of (predictor(s) - target(s))^2; -> (L, p, t)"""
    p = model.predictor(rows)
    with torch.no_grad():
        t = model.target(rows)
    return nn.functional.mse_loss(p, t), p, t


def minibatch_grad(model, s, idx):
    """s [.][D], idx the mini-batch's row list (a row may appear twice).  -> ({key: grad}, L, d L / d p, p, t)"""
    for q in model.parameters():
        q.grad = None
    loss, p, t = minibatch_loss(model, s[idx.long()])
    p.retain_grad()
    loss.backward()
    return {k: q.grad.detach().clone() for k, q in ordered_params(model)}, float(loss.detach()), p.grad.detach().clone(), p.detach(), t


def update(model, s, idx, n_rows_total, n_epochs, n_mini_batches, lr=LR):
    """The predictor's loop: mini-batch i of every epoch is idx[i mbs .. (i + 1) mbs); one Adam step each, no clip.  -> mean of L over the mini-batches"""
    params = [q for _, q in ordered_params(model)]
    opt = torch.optim.Adam(params, lr=lr)
    mbs = n_rows_total // n_mini_batches
    total = 0.0
    for _ in range(n_epochs):
        for i in range(n_mini_batches):
            loss, _, _ = minibatch_loss(model, s[idx[i * mbs:(i + 1) * mbs].long()])
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += float(loss.detach())
    return total / (n_epochs * n_mini_batches)


# ---- the env step --------------------------------------------------------------------------------------------------------------------------------------
def distance64(t, p):
    """item 4 in float64 from float32 embeddings [n][E] (numpy); NOT rounded"""
    d = np.asarray(t, np.float64) - np.asarray(p, np.float64)
    return np.sqrt((d * d).sum(axis=1))


def weight(w0, schedule, counter):
    """item 6: w(counter) in float64"""
    mode = "constant" if schedule is None else schedule["mode"]
    if mode == "constant":
        return float(w0)
    v = float(schedule["final_value"])
    if mode == "step":
        return v if counter >= schedule["final_step"] else float(w0)
    if mode != "linear":
        raise ValueError(mode)
    a, b = schedule["initial_step"], schedule["final_step"]
    if counter < a:
        return float(w0)
    if counter > b:
        return v
    return float(w0) + (v - float(w0)) * (counter - a) / (b - a)


def advance_avg(avg, r):
    """avg' = 0.99f * avg + r in float32: one multiply and one add, each rounded"""
    return (GAMMA32 * np.asarray(avg, np.float32)).astype(np.float32) + np.asarray(r, np.float32)


def reward_fold(state, avg):
    """the one-column fold of the N values of avg into `state` (norm_ref's float32 state with d = 1): -> (new state in float64, per-entry bounds on the
    device's float32 state)"""
    x = np.asarray(avg, np.float64).reshape(-1, 1)
    new64 = NR.update(state, x, until=UNTIL)
    return new64, NR.state_bounds(state, x, new64)


def finish(r, std, w, rewards):
    """items 5 (division) to 7 in float32 from r [n], the state's std (a float32 scalar) and the weight (float64): -> (intrinsic, rewards_total)"""
    r = np.asarray(r, np.float32)
    std = np.float32(std)
    if std > 0:
        r = (r / std).astype(np.float32)
    intrinsic = (np.float32(w) * r).astype(np.float32)
    return intrinsic, (np.asarray(rewards, np.float32) + intrinsic).astype(np.float32)


class RewardNormalizer:
    """The whole reward normaliser as a reference of its own (tests/test_rnd_ref.py): float32 avg, float32 state, float64 fold."""

    def __init__(self, n):
        self.avg = np.zeros(n, np.float32)
        self.state = NR.initial_state(1)

    def __call__(self, r):
        self.avg = advance_avg(self.avg, r)
        if self.state["count"] < UNTIL:
            self.state = NR.rounded(reward_fold(self.state, self.avg)[0])
        std = self.state["std"][0]
        r = np.asarray(r, np.float32)
        return (r / std).astype(np.float32) if std > 0 else r
