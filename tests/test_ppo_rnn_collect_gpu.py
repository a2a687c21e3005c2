"""What PPO + ActorCriticRecurrent hand to the recurrent update (the collection rules of include/go2sim_rnn.h), with no simulator: two consecutive rollouts of
scripted observations, critic observations, rewards and dones, replayed in float64 by tests/ppo_rnn_collect_ref.py from policy.state_dict() read before each
rollout; the float32 replay is the yardstick, the bound the cell step's  max|y - y64| <= C_MLP max(max|y32 - y64|, 2^-24 max|y64|).  The sampled
actions are taken from alg.actions (sampling has its own tests).  After each alg.update() a second recurrent handle runs the same update from clones of
the recorded arrays: the class's parameters must equal its parameters bit for bit, so the class passed exactly what it recorded (the update's numerics
are held to float64 by tests/test_ppo_rnn_gpu.py::test_whole_update)."""
import functools

import numpy as np
import pytest
import torch

import ppo_ref as R
import ppo_rnn_cases as RC
import ppo_rnn_collect_ref as CR
import ppo_rnn_ref as RR
from test_ppo_rnn_gpu import C_MLP, DEV, RnnSide, ratio

pytestmark = pytest.mark.gpu

B, T, NMB, H, IA, IC, A, HID = 6, 4, 2, 20, 5, 7, 3, [8]
ADIMS, CDIMS = [H, *HID, A], [H, *HID, 1]


@functools.lru_cache(maxsize=None)
def script():
    g = torch.Generator().manual_seed(2718)
    s = dict(obs=(RC.obs_scale(IA, H) * torch.randn(2, T, B, IA, generator=g)).float(), critic_obs=(RC.obs_scale(IC, H) * torch.randn(2, T, B, IC, generator=g)).float(),
             last=(RC.obs_scale(IC, H) * torch.randn(2, B, IC, generator=g)).float(), rewards=torch.randn(2, T, B, generator=g).float(),
             dones=CR.scripted_dones(T, B))
    CR.check_dones_script(s["dones"])
    return s


def make_alg():
    from go2_sim2real_locomotion_rl_amd import PPO, ActorCriticRecurrent

    policy = ActorCriticRecurrent(IA, IC, A, HID, HID, rnn_hidden_size=H, seed=5)
    alg = PPO(policy, num_learning_epochs=1, num_mini_batches=NMB, schedule="adaptive", entropy_coef=R.HP["entropy_coef"], learning_rate=R.HP["learning_rate"])
    alg.init_storage(B, T, [IA], [IC], [A])
    return policy, alg


def saved_state(alg):
    return dict(zip(CR.STATE_KEYS, (x.cpu().clone() for x in alg._saved)))


def live_state(policy):
    (ha, ca), (hc, cc) = policy.get_hidden_states()
    return dict(h_a=ha[0].cpu().clone(), c_a=ca[0].cpu().clone(), h_c=hc[0].cpu().clone(), c_c=cc[0].cpu().clone())


@functools.lru_cache(maxsize=None)
def drive():
    """The two rollouts and updates, run once: per rollout the state dict before it, everything the class recorded, the state dict after the update and the
    parameters of the second handle after the same update"""
    s = script()
    policy, alg = make_alg()
    side, out = None, []
    for r in range(2):
        sd = {k: v.clone() for k, v in policy.state_dict().items()}
        for t in range(T):
            actions = alg.act(s["obs"][r, t].to(DEV), s["critic_obs"][r, t].to(DEV))
            assert actions.shape == (B, A)
            alg.process_env_step(s["rewards"][r, t].to(DEV), s["dones"][r, t].to(DEV), {})
        alg.compute_returns(s["last"][r].to(DEV))
        st = alg.storage
        rec = dict(obs=alg.obs, critic_obs=alg.critic_obs, actions=alg.actions, target_values=st.values, returns=st.returns, advantages=st.advantages,
                   old_log_prob=alg.old_log_prob, old_mu=alg.old_mu, old_sigma=alg.old_sigma, dones=st.dones)
        rec = {k: v.cpu().clone() for k, v in rec.items()}
        saved, live = saved_state(alg), live_state(policy)
        if side is None:                                    # the second handle lives through both updates: it carries Adam's moments, the step and the learning rate
            side = RnnSide(policy._L, H, IA, IC, ADIMS, CDIMS, sd, rec, saved, T, B // NMB, **alg._hyper)
        else:
            for k, v in rec.items():
                side.ro[k].copy_(v)
            for k, v in saved.items():
                side.init[k].copy_(v)
        alg.update()
        side.h.rnn_update(side.batch, side.rstate, side.std, B, alg.num_learning_epochs, NMB)
        out.append(dict(sd=sd, rec=rec, saved=saved, live=live, after={k: v.clone() for k, v in policy.state_dict().items()},
                        side_after={k: v.float() for k, v in side.split(side.h.export("PARAMS", side.std)).items()}, lr=alg.learning_rate, lr_side=side.stats()[0]["lr"]))
    return out


@functools.lru_cache(maxsize=None)
def replays():
    """{precision: [rollout 0, rollout 1]} of ppo_rnn_collect_ref.replay_rollout under the state dicts the drive read, the live state carried across"""
    s, d = script(), drive()
    out = {}
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        live, out[prec] = CR.zero_state(B, H, dt), []
        for r in range(2):
            m = RR.make_model(IA, IC, ADIMS, CDIMS, d[r]["sd"], dt)
            rp = CR.replay_rollout(m, live, s["obs"][r], s["critic_obs"][r], s["dones"][r], s["last"][r])
            rp["logp"] = CR.log_prob(rp["mu"], d[r]["sd"]["std"], d[r]["rec"]["actions"])
            out[prec].append(rp)
            live = rp["live"]
    return out


@pytest.mark.parametrize("r", [0, 1])
def test_recorded_rollout_against_the_replay(hip_lib, r):
    s, d, rp = script(), drive()[r], replays()
    p64, p32, rec = rp["f64"][r], rp["f32"][r], drive()[r]["rec"]
    # what is copied is exact
    assert torch.equal(rec["dones"], s["dones"][r]) and torch.equal(rec["obs"], s["obs"][r]) and torch.equal(rec["critic_obs"], s["critic_obs"][r])
    assert torch.equal(rec["old_sigma"], d["sd"]["std"].expand(T, B, A))
    assert torch.isfinite(rec["actions"]).all() and not torch.equal(rec["actions"], rec["old_mu"])
    worst = 0.0
    for name, got, k in (("old_mu", rec["old_mu"], "mu"), ("values", rec["target_values"], "v"), ("old_log_prob", rec["old_log_prob"], "logp")):
        q = ratio(got.double(), p64[k], p32[k])
        print(f"RATIO collect rollout{r} {name} {q:.3f}")
        worst = max(worst, q)
    for which, got in (("saved", d["saved"]), ("live", d["live"])):
        for k in CR.STATE_KEYS:
            q = ratio(got[k].double(), p64[which][k], p32[which][k])
            print(f"RATIO collect rollout{r} {which} {k} {q:.3f}")
            worst = max(worst, q)
            zero = ~p64[which][k].ne(0).any(1)              # the rows the law leaves at exactly zero
            assert not got[k][zero].any() and bool(got[k][~zero].ne(0).any(1).all()), (which, k)
    print(f"RATIO worst collect rollout{r} {worst:.3f}")
    assert worst <= C_MLP
    # the rows that tell a correct collection from a wrong one
    done_last = s["dones"][r, T - 1] != 0
    lv = d["live"]
    assert done_last.any() and not lv["h_a"][done_last].any() and not lv["c_a"][done_last].any()
    assert bool(lv["h_c"][done_last].ne(0).any(1).all()) and bool(lv["c_c"][done_last].ne(0).any(1).all()), "compute_returns stepped memory_c from zero"
    if r == 0:
        assert not any(d["saved"][k].any() for k in CR.STATE_KEYS), "the first rollout starts from the zero state: saved before the first act"
    else:
        prev = drive()[0]["live"]
        assert all(torch.equal(d["saved"][k], prev[k]) for k in CR.STATE_KEYS), "the saved state is the live state the last rollout left"
        was_done = s["dones"][0, T - 1] != 0
        assert not d["saved"]["h_a"][was_done].any() and bool(d["saved"]["h_c"][was_done].ne(0).any(1).all())


@pytest.mark.parametrize("r", [0, 1])
def test_update_takes_exactly_what_was_recorded(hip_lib, r):
    d = drive()[r]
    assert list(d["after"]) == list(d["side_after"])
    for k, v in d["after"].items():
        assert np.array_equal(v.numpy().view(np.int32), d["side_after"][k].numpy().view(np.int32)), k
        assert not torch.equal(v, d["sd"][k]), k
    assert d["lr"] == d["lr_side"]


def test_evaluate_only_and_inference_steps(hip_lib):
    """An evaluate-only step between two act steps leaves h_a / c_a untouched bit for bit and advances only memory_c (the three-buffer rotation hands back
    the right buffers afterwards); act_inference advances memory_a only.  The states against the float64 replay of the same calls."""
    s = script()
    policy, alg = make_alg()
    sd = policy.state_dict()
    bits = lambda st: {k: v.numpy().view(np.int32).copy() for k, v in st.items()}
    obs, cobs = s["obs"][0].to(DEV), s["critic_obs"][0].to(DEV)
    policy.act(obs[0], cobs[0])
    s1 = live_state(policy)
    v = policy.evaluate(cobs[1])
    s2 = live_state(policy)
    assert v.shape == (B, 1)
    assert np.array_equal(bits(s1)["h_a"], bits(s2)["h_a"]) and np.array_equal(bits(s1)["c_a"], bits(s2)["c_a"])
    assert not torch.equal(s1["h_c"], s2["h_c"]) and not torch.equal(s1["c_c"], s2["c_c"])
    policy.act(obs[2], cobs[2])
    s3 = live_state(policy)
    mean3, val3 = policy.action_mean.cpu().clone(), policy.values.cpu().clone().squeeze(-1)
    a = policy.act_inference(obs[3])
    s4 = live_state(policy)
    assert torch.equal(a, policy.action_mean)
    assert np.array_equal(bits(s3)["h_c"], bits(s4)["h_c"]) and np.array_equal(bits(s3)["c_c"], bits(s4)["c_c"])
    assert not torch.equal(s3["h_a"], s4["h_a"]) and not torch.equal(s3["c_a"], s4["c_a"])
    mean4 = a.cpu().clone()
    want = {}
    for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = RR.make_model(IA, IC, ADIMS, CDIMS, sd, dt)
        step = lambda lstm, x, h, c: [y[0] for y in lstm(x.to(dt).unsqueeze(0), (h.unsqueeze(0), c.unsqueeze(0)))[1]]
        z = torch.zeros(B, H, dtype=dt)
        with torch.no_grad():
            ha, ca = step(m.memory_a.rnn, s["obs"][0, 0], z, z)
            hc, cc = step(m.memory_c.rnn, s["critic_obs"][0, 0], z, z)
            hc, cc = step(m.memory_c.rnn, s["critic_obs"][0, 1], hc, cc)
            v2 = m.critic(hc).squeeze(-1)
            ha, ca = step(m.memory_a.rnn, s["obs"][0, 2], ha, ca)
            hc, cc = step(m.memory_c.rnn, s["critic_obs"][0, 2], hc, cc)
            w3 = dict(h_a=ha, c_a=ca, h_c=hc, c_c=cc, mean=m.actor(ha), val=m.critic(hc).squeeze(-1))
            ha, ca = step(m.memory_a.rnn, s["obs"][0, 3], ha, ca)
            want[prec] = dict(v2=v2, s3=w3, h_a4=ha, c_a4=ca, mean4=m.actor(ha))
    got = [("evaluate v", v.cpu().squeeze(-1), "v2"), ("act mean", mean3, ("s3", "mean")), ("act values", val3, ("s3", "val")), ("inference mean", mean4, "mean4"),
           ("inference h_a", s4["h_a"], "h_a4"), ("inference c_a", s4["c_a"], "c_a4")] + [(f"act {k}", s3[k], ("s3", k)) for k in CR.STATE_KEYS]
    worst = 0.0
    for name, x, key in got:
        w64, w32 = (want[p][key] if isinstance(key, str) else want[p][key[0]][key[1]] for p in ("f64", "f32"))
        q = ratio(x.double(), w64, w32)
        print(f"RATIO collect steps {name} {q:.3f}")
        worst = max(worst, q)
    print(f"RATIO worst collect steps {worst:.3f}")
    assert worst <= C_MLP
