"""The mirror-symmetry law of include/go2sim_train.h (rsl_rl 2.2.4's symmetry_cfg with the mirror given as tables) restated in torch autograd on
the CPU, on top of tests/ppo_ref.py: the 2 n-row batch is built explicitly with index_select and signs, the losses are the plain reference's
expressions over it.  In float64 it is the reference of the HIP update with a mirror set; the same functions in float32 are the yardstick.
Shares no code with the product."""
import torch
from torch import nn

import ppo_ref as R

SCALARS = ("surrogate", "value_loss", "entropy", "kl_mean", "symmetry")


def apply_table(x, table):
    """(M x)[..., j] = sign[j] * x[..., src[j]]"""
    src, sign = table
    return x.index_select(-1, torch.as_tensor(src).long()) * torch.as_tensor(sign).to(x.dtype)


def mirrored_rows(mb, tables):
    """The n mirrored rows of a mini-batch: obs, critic obs and actions through their tables, the scalars of the row unchanged.  old_mu and
    old_sigma are only read by kl, which is taken over the original rows: they are copied so that the row dictionary stays complete."""
    out = dict(mb)
    out["obs"], out["critic_obs"], out["actions"] = apply_table(mb["obs"], tables["policy"]), apply_table(mb["critic_obs"], tables["critic"]), \
        apply_table(mb["actions"], tables["actions"])
    return out


def doubled(mb, tables):
    m = mirrored_rows(mb, tables)
    return {k: torch.cat([mb[k], m[k]]) for k in mb}


def loss_terms(model, mb, tables, aug, mloss, coeff, hp=R.HP):
    """-> loss, dict of its terms.  mb: the n original rows."""
    n = mb["obs"].shape[0]
    mb2 = doubled(mb, tables)
    mu2, v2 = model.actor(mb2["obs"]), model.critic(mb2["critic_obs"]).squeeze(-1)
    target = apply_table(mu2[:n].detach(), tables["actions"])
    sym = (mu2[n:] - target).pow(2).mean()
    _, t_orig = R.head_terms(mu2[:n], model.std, v2[:n], mb, hp)                  # kl_mean: the original rows
    if aug:
        loss, t = R.head_terms(mu2, model.std, v2, mb2, hp)
    else:
        loss, t = R.head_terms(mu2[:n], model.std, v2[:n], mb, hp)
    if mloss:
        loss = loss + coeff * sym
    t = dict(t, kl_mean=t_orig["kl_mean"], symmetry=sym, mu2=mu2, v2=v2)
    return loss, t


def minibatch_grad(model, mb, tables, aug, mloss, coeff, hp=R.HP):
    """-> ({key: grad}, {name: float})"""
    for p in model.parameters():
        p.grad = None
    loss, t = loss_terms(model, mb, tables, aug, mloss, coeff, hp)
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in R.ordered_params(model)}
    return grads, {k: float(t[k].detach()) for k in SCALARS}


def update(model, rollout, perm, n_epochs, n_mini_batches, tables, aug, mloss, coeff, hp=R.HP):
    """ppo_ref.update with the mirror: -> (mean value loss, surrogate, entropy, mirror loss), final learning rate.  `model` is updated in place."""
    dtype = next(model.parameters()).dtype
    params = [p for _, p in R.ordered_params(model)]
    lr = hp["learning_rate"]
    opt = torch.optim.Adam(params, lr=lr)
    mbs = rollout["obs"].shape[0] // n_mini_batches
    sums = [0.0, 0.0, 0.0, 0.0]
    for _ in range(n_epochs):
        for i in range(n_mini_batches):
            mb = R.rows_of(rollout, perm[i * mbs:(i + 1) * mbs].long(), dtype)
            loss, t = loss_terms(model, mb, tables, aug, mloss, coeff, hp)
            if hp["schedule"] == "adaptive":
                lr = R.lr_rule(lr, float(t["kl_mean"].detach()), hp["desired_kl"])
                for g in opt.param_groups:
                    g["lr"] = lr
            opt.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(params, hp["max_grad_norm"])
            opt.step()
            for j, k in enumerate(("value_loss", "surrogate", "entropy", "symmetry")):
                sums[j] += float(t[k].detach())
    return tuple(s / (n_epochs * n_mini_batches) for s in sums), lr
