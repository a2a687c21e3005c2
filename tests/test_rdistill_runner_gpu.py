"""OnPolicyRunner with ``Distillation`` + ``StudentTeacherRecurrent`` over the walk env (64 envs, 8 steps per env, gradient_length 4): a recurrent student under
an MLP teacher and under a teacher loaded from a recurrent PPO checkpoint, the checkpoints, the inference policy and the refusals.  The numerics of the
update are held by tests/test_rdistill_gpu.py; here: what moves and what must not, and that the collection runs the teacher the PPO run trained."""
import numpy as np
import pytest
import torch

from test_distill_runner_gpu import DISTILL_CFG, bits, cfg, same
from test_ppo_gpu import TRAIN_CFG, walk_env

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RNN = {"class_name": "StudentTeacherRecurrent", "rnn_type": "lstm", "rnn_hidden_dim": 16, "rnn_num_layers": 1}
RCFG = cfg(DISTILL_CFG, policy=RNN)
RCFG_T = cfg(DISTILL_CFG, policy=dict(RNN, teacher_recurrent=True, teacher_rnn_hidden_dim=32))
MEM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


@pytest.fixture(scope="module")
def teacher_ckpts(tmp_path_factory):
    """PPO on the privileged rows, 2 iterations each: -> (an ActorCritic's checkpoint, an ActorCriticRecurrent's with 32 hidden units)"""
    from go2_sim2real_locomotion_rl_amd import OnPolicyRunner

    d = tmp_path_factory.mktemp("rteacher")
    paths = []
    for name, policy in (("mlp", {}), ("lstm", dict(class_name="ActorCriticRecurrent", rnn_type="lstm", rnn_hidden_size=32, rnn_num_layers=1))):
        r = OnPolicyRunner(walk_env(), cfg(TRAIN_CFG, obs_groups={"policy": "critic"}, policy=policy))
        log = r.learn(2)
        assert all(np.isfinite(x["value_loss"]) for x in log)
        paths.append(str(d / f"{name}.pt"))
        r.save(paths[-1])
    return paths


def test_recurrent_student_under_an_mlp_teacher(teacher_ckpts, tmp_path):
    from go2_sim2real_locomotion_rl_amd import Go2SimError, OnPolicyRunner, StudentTeacherRecurrent
    from go2_sim2real_locomotion_rl_amd.eval_io import read_checkpoint

    r = OnPolicyRunner(walk_env(), RCFG)
    assert isinstance(r.policy, StudentTeacherRecurrent) and r.alg.recurrent and r.policy.is_recurrent
    assert r.policy._sdims == [16, 48, 32, 16] and r.policy._smem == (49, 16) and r.policy._tdims == [104, 64, 32, 16] and r.policy._tmem is None
    with pytest.raises(Go2SimError, match="no teacher"):
        r.learn(1)
    fresh = r.policy.state_dict()
    assert {f"memory_s.rnn.{k}" for k in MEM_KEYS} <= set(fresh) and not any(k.startswith("memory_t.") for k in fresh)
    with pytest.raises(Go2SimError, match="memory_a.*teacher has no memory"):      # a recurrent checkpoint onto a teacher without a memory
        r.load(teacher_ckpts[1])
    r.load(teacher_ckpts[0])
    loaded = r.policy.state_dict()
    teacher = read_checkpoint(teacher_ckpts[0])["model_state_dict"]
    assert all(torch.equal(loaded["teacher." + k[6:]], v) for k, v in teacher.items() if k.startswith("actor."))
    assert same({k: v for k, v in loaded.items() if not k.startswith("teacher.")}, {k: v for k, v in fresh.items() if not k.startswith("teacher.")})
    log = r.learn(2)
    assert len(log) == 2 and all(np.isfinite(x["behavior_loss"]) and x["behavior_loss"] > 0 for x in log)
    after = r.policy.state_dict()
    s = r.alg.last_stats
    assert int(s[3]) == 4 and int(s[4]) == 8 and int(s[5]) == 2                    # 8 pairs in windows of 4: two Adam steps per iteration, no tail
    moved = [k for k in after if not torch.equal(after[k], loaded[k])]
    assert set(moved) == {k for k in after if k.startswith(("student.", "memory_s."))}, moved
    h, c = r.policy.get_hidden_states()[0]
    assert h.shape == (1, 64, 16) and bool(torch.isfinite(h).all()) and bool(h.any()) and r.policy.get_hidden_states()[1] is None
    # save and resume: parameters and optimizer state bit for bit
    path = str(tmp_path / "model.pt")
    r.save(path)
    ck = read_checkpoint(path)
    assert set(ck["model_state_dict"]) == set(after) and ck["iter"] == 2
    r2 = OnPolicyRunner(walk_env(), RCFG)
    r2.load(path)
    assert same(r2.policy.state_dict(), after) and r2.current_learning_iteration == 2 and r2.policy.loaded_teacher
    o1, o2 = r.alg.optimizer_state_dict(), r2.alg.optimizer_state_dict()
    assert o1["step"] == o2["step"] == 4 and o1["lr"] == o2["lr"] and torch.equal(o1["exp_avg"], o2["exp_avg"]) and torch.equal(o1["exp_avg_sq"], o2["exp_avg_sq"])
    assert bool(o1["exp_avg"].any()) and o1["exp_avg"].numel() == sum(v.numel() for k, v in after.items() if k.startswith(("student.", "memory_s.")))
    assert r2.policy._step == r.policy._step
    # the inference policy is the student with its memory: the same observations and dones through both runners' policies
    fn = r.get_inference_policy()
    r.policy.reset(); r2.policy.reset()
    g = torch.Generator().manual_seed(3)
    dones = torch.zeros(64, device=DEV)
    for k in range(3):
        obs = torch.randn(64, 49, generator=g).to(DEV)
        a1, a2 = fn(obs).clone(), r2.policy.act_inference(obs).clone()
        assert np.array_equal(bits({"a": a1})["a"], bits({"a": a2})["a"]) and bool(torch.isfinite(a1).all())
        assert torch.equal(a1, r.policy.action_mean)
        if k < 2:
            dones = (torch.rand(64, generator=g) < 0.3).to(DEV).float()
            r.policy.reset(dones); r2.policy.reset(dones)
    r2.policy.reset()                                                            # a zero memory on the last observations: what a done env must have given
    fresh_out = r2.policy.act_inference(obs)
    d = dones.bool()
    assert d.any() and not d.all()
    assert torch.equal(a1[d], fresh_out[d]) and not torch.equal(a1[~d], fresh_out[~d]), "the memory is carried, and reset(dones) zeroes it for the done envs"


def test_teacher_from_a_recurrent_ppo_checkpoint(teacher_ckpts):
    from go2_sim2real_locomotion_rl_amd import ActorCriticRecurrent, Go2SimError, OnPolicyRunner
    from go2_sim2real_locomotion_rl_amd.eval_io import read_checkpoint

    r = OnPolicyRunner(walk_env(), RCFG_T)
    assert r.policy._tmem == (104, 32) and r.policy._tdims == [32, 64, 32, 16] and r.policy._smem == (49, 16)
    with pytest.raises(Go2SimError, match="no memory_a"):                          # an ActorCritic's checkpoint onto a recurrent teacher
        r.load(teacher_ckpts[0])
    fresh = r.policy.state_dict()
    r.load(teacher_ckpts[1])
    msd = read_checkpoint(teacher_ckpts[1])["model_state_dict"]
    loaded = r.policy.state_dict()
    assert all(torch.equal(loaded["teacher." + k[6:]], v) for k, v in msd.items() if k.startswith("actor."))
    assert all(torch.equal(loaded["memory_t." + k[9:]], v) for k, v in msd.items() if k.startswith("memory_a."))
    assert same({k: v for k, v in loaded.items() if k.startswith(("student.", "memory_s.", "std"))}, {k: v for k, v in fresh.items() if k.startswith(("student.", "memory_s.", "std"))})
    # record what the collection hands to the teacher and what it answers
    rec, alg = {"tobs": [], "ta": [], "dones": []}, r.alg
    act0, step0 = alg.act, alg.process_env_step

    def act(s_obs, t_obs):
        a = act0(s_obs, t_obs)
        rec["tobs"].append(t_obs.clone()); rec["ta"].append(r.policy.teacher_actions.clone())
        return a

    def process_env_step(rewards, dones, infos):
        rec["dones"].append(dones.clone())
        return step0(rewards, dones, infos)

    alg.act, alg.process_env_step = act, process_env_step
    buf = r.env.episode_length_buf.clone()                                       # twelve envs run into their time-out at different steps of the two rollouts
    buf[:12] = int(r.env.max_episode_length) - 2 - torch.arange(12, device=buf.device).to(buf.dtype)
    r.env.episode_length_buf = buf
    log = r.learn(2)
    assert len(log) == 2 and all(np.isfinite(x["behavior_loss"]) and x["behavior_loss"] > 0 for x in log)
    after = r.policy.state_dict()
    assert all(torch.equal(after[k], loaded[k]) for k in after if k.startswith(("teacher.", "memory_t.")))
    assert all(not torch.equal(after[k], loaded[k]) for k in after if k.startswith(("student.", "memory_s.")))
    # the PPO policy itself over the same rows and dones: the update in between left the teacher's memory alone
    ppo = ActorCriticRecurrent(104, 104, 16, [64, 32], [64, 32], rnn_hidden_size=32, seed=9)
    ppo.load_state_dict(msd)
    assert len(rec["tobs"]) == 16 and any(bool(d.any()) for d in rec["dones"])
    for k, (tobs, ta, dones) in enumerate(zip(rec["tobs"], rec["ta"], rec["dones"])):
        want = ppo.act_inference(tobs)
        assert np.array_equal(bits({"a": ta})["a"], bits({"a": want})["a"]), f"step {k}"
        ppo.reset(dones)


def test_refusals_name_the_class_and_the_key():
    from go2_sim2real_locomotion_rl_amd import Distillation, Go2SimError, OnPolicyRunner, StudentTeacherRecurrent

    env = walk_env()
    with pytest.raises(Go2SimError, match="StudentTeacherRecurrent.*rnn_hidden_dim"):
        OnPolicyRunner(env, cfg(DISTILL_CFG, policy={"class_name": "StudentTeacherRecurrent"}))
    with pytest.raises(Go2SimError, match="'PPO' with policy 'StudentTeacherRecurrent'"):
        OnPolicyRunner(env, cfg(TRAIN_CFG, policy=dict(RCFG["policy"])))
    r = OnPolicyRunner(env, cfg(DISTILL_CFG, policy={"class_name": "StudentTeacherRecurrent", "rnn_hidden_size": 20}))      # the alias
    assert r.policy.rnn_hidden_dim == 20 and r.policy._sdims[0] == 20
    policy = StudentTeacherRecurrent(49, 104, 16, [32], [32], rnn_hidden_dim=16)
    alg = Distillation(policy, gradient_length=3)
    assert alg.recurrent
    policy.detach_hidden_states()
    assert policy.get_hidden_states() == (None, None)
