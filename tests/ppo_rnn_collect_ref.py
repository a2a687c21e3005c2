"""The collection rules of include/go2sim_rnn.h replayed in torch on the CPU, for tests/test_ppo_rnn_collect_gpu.py: what PPO + ActorCriticRecurrent must have
recorded after one rollout of scripted observations and dones.  In float64 it is the reference, the same code in float32 the yardstick.  Shares no code with
the product; the memories run through ppo_rnn_ref.unroll (nn.LSTM per step).

The rules:  the four state arrays are saved at the rollout's first act (before it);  act steps memory_a and memory_c on the step's observations;
reset(dones[t]) follows every env step, so dones[t] cuts between step t and step t + 1 -- and the reset after the last step acts on the state the next
rollout starts from;  compute_returns evaluates the last critic observation, which advances memory_c (not memory_a) once more."""
import torch

import ppo_rnn_ref as RR

STATE_KEYS = ("h_a", "c_a", "h_c", "c_c")


def scripted_dones(T, B):
    """[2][T][B] uint8 for two consecutive rollouts.  Rollout 0: env 0 done at step 0, env 1 on the two consecutive steps 1 and 2, env 2 (and env 5) at the
    last step, env 3 never (in neither rollout).  Rollout 1: env 0 at the last step, env 4 at step 1, env 5 at step 0."""
    assert T >= 4 and B >= 6
    d = torch.zeros(2, T, B, dtype=torch.uint8)
    d[0, 0, 0] = 1
    d[0, 1, 1] = d[0, 2, 1] = 1
    d[0, T - 1, 2] = d[0, T - 1, 5] = 1
    d[1, T - 1, 0] = 1
    d[1, 1, 4] = 1
    d[1, 0, 5] = 1
    return d


def check_dones_script(d):
    """The script holds every pattern the collection rules distinguish (rollout 0)"""
    d0, T = d[0], d.shape[1]
    assert bool(d0[0].any()), "an env done at step 0"
    assert bool((d0[:-1] & d0[1:]).any()), "an env done on two consecutive steps"
    assert bool(d0[T - 1].any()), "an env done at the last step of the first rollout"
    assert bool((d.sum((0, 1)) == 0).any()), "an env that is never done"
    assert bool((d0[T - 1] == 0).any()) and bool(d[1].any())


def zero_state(B, H, dtype):
    return {k: torch.zeros(B, H, dtype=dtype) for k in STATE_KEYS}


def replay_rollout(model, live, obs, critic_obs, dones, last_critic_obs):
    """One rollout under `model` (ppo_rnn_ref.Model) from the live state `live` ({h_a, c_a, h_c, c_c} [B][H]) entering its first act.
    obs [T][B][Ia], critic_obs [T][B][Ic], dones [T][B], last_critic_obs [B][Ic].
    -> dict(saved = the state entering step 0, mu [T][B][A], v [T][B], last_v [B], live = the state after compute_returns)"""
    dt = next(model.parameters()).dtype
    T, B = dones.shape
    saved = {k: live[k].to(dt).clone() for k in STATE_KEYS}
    with torch.no_grad():
        ha, (h_a, c_a), _ = RR.unroll(model.memory_a.rnn, obs.to(dt), saved["h_a"], saved["c_a"], dones)
        hc, (h_c, c_c), _ = RR.unroll(model.memory_c.rnn, critic_obs.to(dt), saved["h_c"], saved["c_c"], dones)
        mu = model.actor(ha.reshape(T * B, -1)).reshape(T, B, -1)
        v = model.critic(hc.reshape(T * B, -1)).reshape(T, B)
        keep = (dones[T - 1] == 0).to(dt).unsqueeze(-1)                  # reset(dones) after the last env step
        h_a, c_a, h_c, c_c = h_a * keep, c_a * keep, h_c * keep, c_c * keep
        _, (hn, cn) = model.memory_c.rnn(last_critic_obs.to(dt).unsqueeze(0), (h_c.unsqueeze(0), c_c.unsqueeze(0)))      # compute_returns' evaluate
        last_v = model.critic(hn[0]).squeeze(-1)
    return dict(saved=saved, mu=mu, v=v, last_v=last_v, live=dict(h_a=h_a, c_a=c_a, h_c=hn[0], c_c=cn[0]))


def log_prob(mu, std, actions):
    """Normal(mu, std).log_prob(actions).sum(-1) in mu's precision"""
    return torch.distributions.Normal(mu, mu * 0 + std.to(mu.dtype)).log_prob(actions.to(mu.dtype)).sum(-1)
