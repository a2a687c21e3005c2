"""OnPolicyRunner with ``train_cfg["empirical_normalization"]`` on: 64 walk envs, 8 steps per env, the small nets of test_ppo_gpu.TRAIN_CFG.  The policy sees
the normalised rows (checked against tests/norm_ref.py under the normaliser's own prior state), the env's tensors stay as they are, the checkpoint carries
rsl_rl's two state dicts, resumption is bit for bit, both load mismatches are refused, the inference policy normalises without counting; the recurrent policy,
symmetry and an env without critic observations run through the same loop."""
import copy

import numpy as np
import pytest
import torch

import norm_cases as NC
import norm_ref as R
from test_ppo_gpu import TRAIN_CFG, walk_env

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NORM_CFG = dict(TRAIN_CFG, empirical_normalization=True)
NORM_KEYS = {"_mean": (1,), "_var": (1,), "_std": (1,), "count": ()}


def np_state(norm):
    sd = norm.state_dict()
    return {"mean": sd["_mean"].reshape(-1).numpy().copy(), "var": sd["_var"].reshape(-1).numpy().copy(), "std": sd["_std"].reshape(-1).numpy().copy(),
            "count": int(sd["count"])}


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).contiguous().cpu().numpy().view(np.uint8), b.reshape(-1).contiguous().cpu().numpy().view(np.uint8))


def norm_dicts_equal(a, b):
    return set(a) == set(b) and all(bits_equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """a runner after learn(2) with every _normalize call recorded: raw inputs, prior and posterior states, outputs; and what alg.act received"""
    from go2_sim2real_locomotion_rl_amd import OnPolicyRunner

    runner = OnPolicyRunner(walk_env(), NORM_CFG)                      # accepted: the parent raised "out of scope" here
    calls, acts = [], []
    normalize, act = runner._normalize, runner.alg.act

    def spy_normalize(obs, critic, update):
        rec = {"update": update, "obs": obs.clone(), "critic": critic.clone(), "obs_ptr": obs.data_ptr(), "prior": (np_state(runner.obs_normalizer), np_state(runner.critic_obs_normalizer))}
        y, yc = normalize(obs, critic, update)
        rec.update(y=y.clone(), yc=yc.clone(), post=(np_state(runner.obs_normalizer), np_state(runner.critic_obs_normalizer)),
                   obs_after=obs.clone(), critic_after=critic.clone())
        calls.append(rec)
        return y, yc

    def spy_act(obs, critic_obs):
        acts.append((obs.clone(), critic_obs.clone()))
        return act(obs, critic_obs)

    runner._normalize, runner.alg.act = spy_normalize, spy_act
    log = runner.learn(2)
    runner._normalize, runner.alg.act = normalize, act
    path = str(tmp_path_factory.mktemp("norm") / "model_2.pt")
    runner.save(path)
    return runner, calls, acts, log, path


def test_switch_is_accepted_and_counts_every_env_step(trained):
    runner, calls, acts, log, _ = trained
    assert len(log) == 2 and all(np.isfinite(v) for d in log for v in (d["value_loss"], d["surrogate_loss"], d["entropy"]))
    assert int(runner.obs_normalizer.count) == int(runner.critic_obs_normalizer.count) == 2 * 8 * 64
    assert runner.obs_normalizer.until == runner.critic_obs_normalizer.until == 1e8
    assert len(calls) == 1 + 2 * 8 and not calls[0]["update"] and all(c["update"] for c in calls[1:])
    assert calls[0]["post"][0]["count"] == 0                           # the starting observations are not counted
    assert runner.env.check_errno() == 0


def test_policy_sees_the_reference_normalisation_and_the_env_keeps_its_tensors(trained):
    runner, calls, acts, _, _ = trained
    assert len(acts) == 2 * 8
    worst = {}
    for i, c in enumerate(calls):
        assert bits_equal(c["obs"], c["obs_after"]) and bits_equal(c["critic"], c["critic_after"])       # the raw tensors are not written
        for raw, y, k in ((c["obs"], c["y"], 0), (c["critic"], c["yc"], 1)):
            x = raw.cpu().numpy()
            w = NC.check_step(c["prior"][k], x, c["post"][k], y.cpu().numpy(), until=1e8 if c["update"] else -1.0,
                              ref64=None if c["update"] else {q: (v.astype(np.float64) if q != "count" else v) for q, v in c["prior"][k].items()})
            for key, v in w.items():
                worst[key] = max(worst.get(key, 0.0), v)
        if i < len(acts):                                              # call i's outputs are what act i received (the last call's go to compute_returns)
            assert bits_equal(acts[i][0], c["y"]) and bits_equal(acts[i][1], c["yc"])
    print(f"runner: worst ratio to the kernel bounds over {len(calls)} steps: {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst
    obs, extras = runner.env.get_observations()
    assert obs.data_ptr() == calls[-1]["obs_ptr"] and bits_equal(obs, calls[-1]["obs"])                 # handed out again, still raw
    assert not bits_equal(runner.alg.obs[7], obs)                      # the storage holds normalised rows


def test_checkpoint_carries_rsl_rl_state_dicts(trained):
    from go2_sim2real_locomotion_rl_amd.eval_io import read_checkpoint

    runner, _, _, _, path = trained
    ck = read_checkpoint(path)
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "obs_norm_state_dict", "critic_obs_norm_state_dict"}
    for key, d in (("obs_norm_state_dict", 49), ("critic_obs_norm_state_dict", 104)):
        sd = ck[key]
        assert set(sd) == set(NORM_KEYS)
        for k in ("_mean", "_var", "_std"):
            assert sd[k].shape == (1, d) and sd[k].dtype == torch.float32
        assert sd["count"].shape == () and sd["count"].dtype == torch.int64 and int(sd["count"]) == 2 * 8 * 64
    assert norm_dicts_equal(ck["obs_norm_state_dict"], runner.obs_normalizer.state_dict())


def test_inference_policy_normalises_without_counting(trained):
    runner = trained[0]
    before = runner.obs_normalizer.state_dict()
    x = torch.randn(64, 49, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * 2 + 1
    x0 = x.clone()
    a = runner.get_inference_policy()(x).clone()
    assert norm_dicts_equal(before, runner.obs_normalizer.state_dict()) and bits_equal(x, x0)
    runner.obs_normalizer.eval()
    y = runner.obs_normalizer(x).clone()
    runner.obs_normalizer.train()
    assert norm_dicts_equal(before, runner.obs_normalizer.state_dict())
    assert bits_equal(a, runner.policy.act_inference(y)) and a.shape == (64, 16)
    inv = runner.obs_normalizer.inverse(y)
    # three float32 roundings forward and two back, each at most 2^-24 of |x| + |mean| + |y| (std + eps): 5 x 6e-8 x that, far inside 1e-5 (1 + |x|)
    assert torch.allclose(inv, x, rtol=1e-5, atol=1e-5)


def test_switch_off_keeps_the_old_checkpoint_and_both_mismatches_are_refused(trained, tmp_path):
    from go2_sim2real_locomotion_rl_amd import Go2SimError, OnPolicyRunner
    from go2_sim2real_locomotion_rl_amd.eval_io import read_checkpoint

    runner, _, _, _, with_norm = trained
    plain = OnPolicyRunner(walk_env(), TRAIN_CFG)
    assert plain.obs_normalizer is None and plain.critic_obs_normalizer is None
    without = str(tmp_path / "plain.pt")
    plain.save(without)
    assert set(read_checkpoint(without)) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    before = runner.obs_normalizer.state_dict()
    with pytest.raises(Go2SimError, match="obs_norm_state_dict"):
        runner.load(without)
    assert norm_dicts_equal(before, runner.obs_normalizer.state_dict())
    params = plain.policy.state_dict()
    with pytest.raises(Go2SimError, match="empirical_normalization"):
        plain.load(with_norm)
    assert all(bits_equal(v, plain.policy.state_dict()[k]) for k, v in params.items())
    assert plain.get_inference_policy() == plain.policy.act_inference


def test_resume_is_bit_for_bit(tmp_path):
    from go2_sim2real_locomotion_rl_amd import OnPolicyRunner

    straight = OnPolicyRunner(walk_env(), NORM_CFG)
    log_a = straight.learn(3)
    resumed = OnPolicyRunner(walk_env(), NORM_CFG)
    log_b = resumed.learn(2)
    path = str(tmp_path / "model_2.pt")
    resumed.save(path)
    saved = resumed.obs_normalizer.state_dict()
    resumed.alg.update()                                               # disturb everything load() has to restore
    resumed.policy._step += 5
    resumed.obs_normalizer.update(torch.full((7, 49), 3.0, device=DEV))
    resumed.critic_obs_normalizer.update(torch.full((7, 104), -2.0, device=DEV))
    assert not norm_dicts_equal(saved, resumed.obs_normalizer.state_dict())
    resumed.load(path)
    assert norm_dicts_equal(saved, resumed.obs_normalizer.state_dict())
    log_b += resumed.learn(1)
    assert log_a == log_b
    sa, sb = straight.policy.state_dict(), resumed.policy.state_dict()
    assert all(bits_equal(sa[k], sb[k]) for k in sa)
    oa, ob = straight.alg.optimizer_state_dict(), resumed.alg.optimizer_state_dict()
    assert bits_equal(oa["exp_avg"], ob["exp_avg"]) and bits_equal(oa["exp_avg_sq"], ob["exp_avg_sq"]) and oa["step"] == ob["step"] == 3 * 2 * 4
    assert norm_dicts_equal(straight.obs_normalizer.state_dict(), resumed.obs_normalizer.state_dict())
    assert norm_dicts_equal(straight.critic_obs_normalizer.state_dict(), resumed.critic_obs_normalizer.state_dict())
    assert int(straight.obs_normalizer.count) == 3 * 8 * 64


@pytest.mark.parametrize("variant", ["recurrent", "symmetry"])
def test_recurrent_policy_and_symmetry_train_on_normalised_rows(variant):
    from go2_sim2real_locomotion_rl_amd import OnPolicyRunner

    cfg = copy.deepcopy(NORM_CFG)
    if variant == "recurrent":
        cfg["policy"].update(class_name="ActorCriticRecurrent", rnn_type="lstm", rnn_hidden_size=32, rnn_num_layers=1)
    else:
        cfg["algorithm"]["symmetry_cfg"] = {"use_data_augmentation": True, "use_mirror_loss": True, "mirror_loss_coeff": 0.5}
    runner = OnPolicyRunner(walk_env(), cfg)
    log = runner.learn(1)
    assert all(np.isfinite(log[0][k]) for k in ("value_loss", "surrogate_loss", "entropy"))
    if variant == "symmetry":
        assert np.isfinite(log[0]["symmetry_loss"])
    assert int(runner.obs_normalizer.count) == int(runner.critic_obs_normalizer.count) == 8 * 64
    assert runner.env.check_errno() == 0


class NoCriticEnv:
    """a crouch env whose extras carry no "critic" entry (Go2Env itself always gives one: for the 45-observation envs it is the actor's tensor)"""

    def __init__(self, env):
        self._env = env

    def __getattr__(self, name):
        return getattr(self._env, name)

    @staticmethod
    def _strip(extras):
        out = dict(extras)
        out["observations"] = {k: v for k, v in extras["observations"].items() if k != "critic"}
        return out

    def get_observations(self):
        obs, extras = self._env.get_observations()
        return obs, self._strip(extras)

    def step(self, actions):
        obs, rew, dones, infos = self._env.step(actions)
        return obs, rew, dones, self._strip(infos)


def test_env_without_critic_observations_leaves_the_critic_normaliser_unused():
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_crouch_cfgs, init

    init(seed=11)
    env = Go2Env(64, *get_crouch_cfgs(), seed=11)
    obs, extras = env.get_observations()
    assert extras["observations"]["critic"].data_ptr() == obs.data_ptr()          # what Go2Env gives for a 45-observation env
    runner = OnPolicyRunner(NoCriticEnv(env), NORM_CFG)
    seen = []
    act = runner.alg.act
    runner.alg.act = lambda o, c: (seen.append(o.data_ptr() == c.data_ptr()), act(o, c))[1]
    log = runner.learn(1)
    assert all(seen) and len(seen) == 8                                           # the critic reads the normalised actor rows
    assert int(runner.obs_normalizer.count) == 8 * 64 and int(runner.critic_obs_normalizer.count) == 0
    assert np.isfinite(log[0]["value_loss"]) and env.check_errno() == 0
    # with Go2Env's own extras the critic entry is there and its normaliser counts, as rsl_rl's loop would
    init(seed=11)
    both = OnPolicyRunner(Go2Env(64, *get_crouch_cfgs(), seed=11), NORM_CFG)
    both.learn(1)
    assert int(both.critic_obs_normalizer.count) == 8 * 64
