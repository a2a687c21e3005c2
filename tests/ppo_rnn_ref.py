"""The recurrent PPO update of rsl-rl-lib 2.2.4 (ActorCriticRecurrent, rnn_type "lstm", one layer) restated in torch on the CPU: two nn.LSTM memories
in front of the two MLPs of tests/ppo_ref.py, autograd through time, the losses of ppo_ref.head_terms, clip_grad_norm_ and torch.optim.Adam.  In
float64 it is the reference of the HIP update (include/go2sim_rnn.h); the same functions in float32 are the yardstick.  Shares no code with the product.

The law: the recurrent generator does not shuffle, mini-batch m is the env block [m B / nmb, (m + 1) B / nmb) with all T steps; the memories run over the
[T][block] grid from the state saved at the rollout's first act, with h, c <- 0 entering step t + 1 wherever dones[t] is set; every loss is a mean over
all T x block rows (row t * block + j)."""
import torch
from torch import nn

import ppo_ref as R

LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


class Memory(nn.Module):
    """rsl_rl.modules.actor_critic_recurrent.Memory: state-dict keys rnn.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}"""

    def __init__(self, n_in, n_hidden):
        super().__init__()
        self.rnn = nn.LSTM(input_size=n_in, hidden_size=n_hidden, num_layers=1)


class Model(nn.Module):
    """ActorCriticRecurrent: memory_a = LSTM(I_a -> H) feeds the actor MLP (adims[0] == H), memory_c = LSTM(I_c -> H) the critic MLP"""

    def __init__(self, n_obs, n_cobs, adims, cdims):
        super().__init__()
        assert adims[0] == cdims[0]
        self.n_obs, self.n_cobs, self.H = n_obs, n_cobs, adims[0]
        self.adims, self.cdims = list(adims), list(cdims)
        self.actor, self.critic = R.mlp(adims), R.mlp(cdims)
        self.std = nn.Parameter(torch.ones(adims[-1]))
        self.memory_a, self.memory_c = Memory(n_obs, self.H), Memory(n_cobs, self.H)


def ordered_params(model):
    """[(key, parameter)] in the flat order of go2sim_ppo_export with memories: actor W0, b0, ..., critic W0, b0, ..., memory_a weight_ih, weight_hh,
    bias_ih, bias_hh, memory_c the same, std"""
    named = dict(model.named_parameters())
    out = []
    for prefix, dims in (("actor", model.adims), ("critic", model.cdims)):
        for l in range(len(dims) - 1):
            out += [(f"{prefix}.{2 * l}.weight", named[f"{prefix}.{2 * l}.weight"]), (f"{prefix}.{2 * l}.bias", named[f"{prefix}.{2 * l}.bias"])]
    for prefix in ("memory_a", "memory_c"):
        out += [(f"{prefix}.rnn.{k}", named[f"{prefix}.rnn.{k}"]) for k in LSTM_KEYS]
    out.append(("std", named["std"]))
    return out


def make_model(n_obs, n_cobs, adims, cdims, state, dtype):
    m = Model(n_obs, n_cobs, adims, cdims).to(dtype)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(state[k].to(dtype))
    return m


def unroll(lstm, x, h0, c0, dones):
    """nn.LSTM over x [T][n][I] from (h0, c0) [n][H], the state zeroed entering step t + 1 where dones[t] [T][n] is set.  -> h' [T][n][H], (h, c) after
    the last step (not masked by the last dones), the gate pre-activations [T][n][4H] (detached; for the cases' own conditions)"""
    T = x.shape[0]
    h, c = h0, c0
    hs, zs = [], []
    for t in range(T):
        if t > 0:
            keep = (dones[t - 1] == 0).to(x.dtype).unsqueeze(-1)
            h, c = h * keep, c * keep
        with torch.no_grad():
            zs.append(x[t] @ lstm.weight_ih_l0.T + lstm.bias_ih_l0 + h @ lstm.weight_hh_l0.T + lstm.bias_hh_l0)
        out, (hn, cn) = lstm(x[t:t + 1], (h.unsqueeze(0), c.unsqueeze(0)))
        h, c = hn[0], cn[0]
        hs.append(out[0])
    return torch.stack(hs), (h, c), torch.stack(zs)


def block_rows(ro, e0, nb, dtype):
    """The env block's rows in mini-batch order (row t * nb + j) of a rollout whose arrays are [T][B][...]"""
    return {k: ro[k][:, e0:e0 + nb].reshape((-1,) + tuple(ro[k].shape[2:])).to(dtype) for k in R.ROW_KEYS}


def forward(model, ro, init, e0, nb):
    """mu [T nb][A], v [T nb] of the env block under the model's parameters; `init` = dict(h_a, c_a, h_c, c_c) [B][H]"""
    dt = next(model.parameters()).dtype
    d = ro["dones"][:, e0:e0 + nb]
    ha, _, za = unroll(model.memory_a.rnn, ro["obs"][:, e0:e0 + nb].to(dt), init["h_a"][e0:e0 + nb].to(dt), init["c_a"][e0:e0 + nb].to(dt), d)
    hc, _, zc = unroll(model.memory_c.rnn, ro["critic_obs"][:, e0:e0 + nb].to(dt), init["h_c"][e0:e0 + nb].to(dt), init["c_c"][e0:e0 + nb].to(dt), d)
    mu = model.actor(ha.reshape(-1, model.H))
    v = model.critic(hc.reshape(-1, model.H)).squeeze(-1)
    return mu, v, (za, zc)


def loss_terms(model, ro, init, e0, nb, hp=R.HP):
    dt = next(model.parameters()).dtype
    mu, v, _ = forward(model, ro, init, e0, nb)
    return R.head_terms(mu, model.std, v, block_rows(ro, e0, nb, dt), hp)


def minibatch_grad(model, ro, init, e0, nb, hp=R.HP):
    """-> ({key: grad}, {name: float})"""
    for p in model.parameters():
        p.grad = None
    loss, t = loss_terms(model, ro, init, e0, nb, hp)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in ordered_params(model)}
    return grads, {k: float(t[k].detach()) for k in ("surrogate", "value_loss", "entropy", "kl_mean")}


def update(model, ro, init, n_epochs, n_mini_batches, hp=R.HP):
    """PPO.update with the recurrent generator: -> (mean value loss, mean surrogate loss, mean entropy), final learning rate, per-mini-batch kl_mean"""
    params = [p for _, p in ordered_params(model)]
    lr = hp["learning_rate"]
    opt = torch.optim.Adam(params, lr=lr)
    B = ro["obs"].shape[1]
    assert B % n_mini_batches == 0
    nb = B // n_mini_batches
    sums, kls = [0.0, 0.0, 0.0], []
    for _ in range(n_epochs):
        for i in range(n_mini_batches):
            loss, t = loss_terms(model, ro, init, i * nb, nb, hp)
            if hp["schedule"] == "adaptive":
                lr = R.lr_rule(lr, float(t["kl_mean"].detach()), hp["desired_kl"])
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
