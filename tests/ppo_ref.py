"""The PPO update of rsl-rl-lib 2.2.4 as the train scripts configure it, restated literally in torch on the CPU: nn.Sequential(Linear, ELU, ...),
torch.distributions.Normal, autograd, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam.  In float64 it is the reference of the HIP update
(include/go2sim_train.h); the same functions in float32 are the yardstick its error is measured with.  Shares no code with the product."""
import torch
from torch import nn

HP = dict(clip_param=0.2, desired_kl=0.01, entropy_coef=0.003, learning_rate=1e-3, max_grad_norm=1.0, value_loss_coef=1.0,
          use_clipped_value_loss=True, schedule="adaptive")
ROW_KEYS = ("obs", "critic_obs", "actions", "target_values", "returns", "advantages", "old_log_prob", "old_mu", "old_sigma")


def mlp(dims):
    layers = []
    for l in range(len(dims) - 1):
        layers.append(nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            layers.append(nn.ELU())
    return nn.Sequential(*layers)


class Model(nn.Module):
    """rsl_rl.modules.ActorCritic: state-dict keys actor.{0,2,..}.{weight,bias}, critic.{0,2,..}.{weight,bias}, std"""

    def __init__(self, adims, cdims):
        super().__init__()
        self.adims, self.cdims = list(adims), list(cdims)
        self.actor, self.critic = mlp(adims), mlp(cdims)
        self.std = nn.Parameter(torch.ones(adims[-1]))


def ordered_params(model):
    """[(key, parameter)] in the flat order of go2sim_ppo_export: actor W0, b0, ..., critic W0, b0, ..., std"""
    named = dict(model.named_parameters())
    out = []
    for prefix, dims in (("actor", model.adims), ("critic", model.cdims)):
        for l in range(len(dims) - 1):
            out += [(f"{prefix}.{2 * l}.weight", named[f"{prefix}.{2 * l}.weight"]), (f"{prefix}.{2 * l}.bias", named[f"{prefix}.{2 * l}.bias"])]
    out.append(("std", named["std"]))
    return out


def make_model(adims, cdims, state, dtype):
    """A Model in `dtype` holding the float32-exact values of `state` (key -> tensor)."""
    m = Model(adims, cdims).to(dtype)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(state[k].to(dtype))
    return m


def flat(tensors_by_key, model):
    return torch.cat([tensors_by_key[k].reshape(-1) for k, _ in ordered_params(model)])


def head_terms(mu, std, v, mb, hp=HP):
    """The issue's law from the networks' outputs: mu [n][A], the learned std [A], v [n].  -> loss, dict of its terms (tensors)"""
    sigma = mu * 0.0 + std
    dist = torch.distributions.Normal(mu, sigma)
    logp = dist.log_prob(mb["actions"]).sum(-1)
    entropy = dist.entropy().sum(-1)
    kl = torch.sum(torch.log(sigma / mb["old_sigma"] + 1.0e-5) + (mb["old_sigma"] ** 2 + (mb["old_mu"] - mu) ** 2) / (2.0 * sigma ** 2) - 0.5, dim=-1)
    ratio = torch.exp(logp - mb["old_log_prob"])
    adv, clip = mb["advantages"], hp["clip_param"]
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    if hp["use_clipped_value_loss"]:
        v_clipped = mb["target_values"] + (v - mb["target_values"]).clamp(-clip, clip)
        value_loss = torch.max((v - mb["returns"]).pow(2), (v_clipped - mb["returns"]).pow(2)).mean()
    else:
        value_loss = (mb["returns"] - v).pow(2).mean()
    loss = surrogate + hp["value_loss_coef"] * value_loss - hp["entropy_coef"] * entropy.mean()
    return loss, dict(surrogate=surrogate, value_loss=value_loss, entropy=entropy.mean(), kl_mean=kl.mean(), mu=mu, v=v, logp=logp, ratio=ratio)


def loss_terms(model, mb, hp=HP):
    """One mini-batch `mb` (key -> rows) under the model's current parameters"""
    return head_terms(model.actor(mb["obs"]), model.std, model.critic(mb["critic_obs"]).squeeze(-1), mb, hp)


def lr_rule(lr, kl_mean, desired_kl):
    if kl_mean > desired_kl * 2.0:
        return max(1e-5, lr / 1.5)
    if kl_mean < desired_kl / 2.0 and kl_mean > 0.0:
        return min(1e-2, lr * 1.5)
    return lr


def rows_of(rollout, idx, dtype):
    return {k: rollout[k][idx].to(dtype) for k in ROW_KEYS}


def minibatch_grad(model, mb, hp=HP):
    """-> ({key: grad}, {name: float})"""
    for p in model.parameters():
        p.grad = None
    loss, t = loss_terms(model, mb, hp)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in ordered_params(model)}
    return grads, {k: float(t[k].detach()) for k in ("surrogate", "value_loss", "entropy", "kl_mean")}


def adam_step(model, grads, exp_avg, exp_avg_sq, steps_done, lr, max_grad_norm):
    """clip_grad_norm_ + one torch.optim.Adam step from the given optimizer state (tensors by key, `steps_done` earlier steps).  -> total_norm"""
    params = [p for _, p in ordered_params(model)]
    opt = torch.optim.Adam(params, lr=lr)
    for k, p in ordered_params(model):
        p.grad = grads[k].detach().clone().to(p.dtype)
        opt.state[p] = {"step": torch.tensor(float(steps_done)), "exp_avg": exp_avg[k].detach().clone().to(p.dtype),
                        "exp_avg_sq": exp_avg_sq[k].detach().clone().to(p.dtype)}
    total_norm = float(nn.utils.clip_grad_norm_(params, max_grad_norm))
    opt.step()
    for k, p in ordered_params(model):
        exp_avg[k], exp_avg_sq[k] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    return total_norm


def update(model, rollout, perm, n_epochs, n_mini_batches, hp=HP):
    """PPO.update: -> (mean value loss, mean surrogate loss, mean entropy), final learning rate, per-mini-batch kl_mean list.  `model` is updated in place."""
    dtype = next(model.parameters()).dtype
    params = [p for _, p in ordered_params(model)]
    lr = hp["learning_rate"]
    opt = torch.optim.Adam(params, lr=lr)
    n_rows = rollout["obs"].shape[0]
    mbs = n_rows // n_mini_batches
    sums, kls = [0.0, 0.0, 0.0], []
    for _ in range(n_epochs):
        for i in range(n_mini_batches):
            mb = rows_of(rollout, perm[i * mbs:(i + 1) * mbs].long(), dtype)
            loss, t = loss_terms(model, mb, hp)
            if hp["schedule"] == "adaptive":
                lr = lr_rule(lr, float(t["kl_mean"].detach()), hp["desired_kl"])
                for g in opt.param_groups:
                    g["lr"] = lr
            opt.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(params, hp["max_grad_norm"])
            opt.step()
            sums = [sums[0] + float(t["value_loss"].detach()), sums[1] + float(t["surrogate"].detach()), sums[2] + float(t["entropy"].detach())]
            kls.append(float(t["kl_mean"].detach()))
    n = n_epochs * n_mini_batches
    return tuple(s / n for s in sums), lr, kls
