"""The walk / stair envs with per-leg stiffness off (`pls_enable=False`) on the HIP library.

1. Replay of tests/golden/ref_env_*nopls*.npz, recorded by tools/make_ref_env_fixtures.py from the reference's go2_env_walk.py / go2_env_stair.py on the
   genesis alias over the CPU oracle's physics, with the tolerances of tests/test_ref_env_fixtures.py; the gains the env handed to
   set_dofs_kp / set_dofs_kv are compared bit for bit as well.  The oracle's own env layer has no PLS-off path, so these fixtures are replayed on the
   HIP library only.  The `_rng` cases run on the -DGO2SIM_RNG_CONST build.  Both engine-PD cases (`_engine`) use dyadic gains (easy range = hard
   range), for which torch's float32 mean() -- what the reference hands to set_dofs_kp -- is the correctly rounded mean the C ABI computes; the
   fixture script asserts that at record time, so the comparison is exact.
2. 4096 envs x 300 steps of each mode through Go2Env on the product build: errno 0, finite outputs, and in mode B at every step the batch gains equal
   the correctly rounded float64 mean of the per-env gains of the envs that reset (read back from the device), exactly.
3. One closed loop ActorCritic(45, 100, 12) + Go2Env + RolloutStorage.
"""
import os

import numpy as np
import pytest
import torch

import test_ref_env_fixtures as ref_fix
from test_ref_env_fixtures import load_fixture, replay_and_compare

NOPLS_CASES = ["walk_nopls", "walk_nopls_engine", "walk_nopls_static", "stairs_nopls"]
NOPLS_RNG_CASES = ["walk_nopls_rng", "walk_nopls_engine_rng"]


class GainRecordingEnv(ref_fix.FusedEnv):
    """FusedEnv that keeps (engine_kp, engine_kd) of the env globals after every step."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gains = []

    def step(self, act):
        out = super().step(act)
        g = self.sim.env_globals()
        self.gains.append((np.float32(g.engine_kp), np.float32(g.engine_kd)))
        return out


def replay_with_gains(monkeypatch, lib, blob, case):
    made = []

    def factory(*a, **kw):
        made.append(GainRecordingEnv(*a, **kw))
        return made[-1]

    monkeypatch.setattr(ref_fix, "FusedEnv", factory)
    z, meta = replay_and_compare(lib, blob, case, gpu=True, physics="fast")
    env_cfg = load_fixture(case, "fast")[1][0]
    rec = z["engine_gains"]                                                # [steps, 12, (kp, kv)] handed to set_dofs_kp / kv
    assert np.all(rec == rec[:, :1, :]), "one gain for all 12 motor dofs"
    if "_engine" in case:                                                  # mode B: the batch mean of each reset call
        got = np.array(made[0].gains, np.float32)
        assert np.array_equal(got, rec[:, 0, :]), f"{case}: engine gains, first difference at step {np.flatnonzero((got != rec[:, 0, :]).any(1))[:1]}"
    elif "_static" in case:                                                # mode C: env_cfg kp / kd (go2_env_walk.py:248-249)
        assert np.all(rec[:, 0, 0] == np.float32(env_cfg["kp"])) and np.all(rec[:, 0, 1] == np.float32(env_cfg["kd"]))
    else:                                                                  # mode A: manual PD, engine gains zeroed (:520-522)
        assert np.all(rec == 0.0)
    return z, meta


@pytest.mark.gpu
@pytest.mark.parametrize("case", NOPLS_CASES)
def test_hip_env_matches_the_reference_env_files_pls_off(monkeypatch, hip_lib, blob, case):
    replay_with_gains(monkeypatch, hip_lib, blob, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NOPLS_RNG_CASES)
def test_hip_env_matches_the_reference_env_files_pls_off_with_scheduled_draws(monkeypatch, blob, case):
    from go2_sim2real_locomotion_rl_amd import build
    from go2_sim2real_locomotion_rl_amd.capi import Go2SimLib

    lib = Go2SimLib(os.path.abspath(build.build_hip_variant("rng_const", build.HIP_VARIANTS["rng_const"], verbose=False)), "go2sim_")
    z, meta = replay_with_gains(monkeypatch, lib, blob, case)
    if "_engine" in case:
        assert len(np.unique(z["engine_gains"][:, 0, 0])) >= 3, "the batch gain changed between reset calls"


def mode_cfgs(mode, task="walk"):
    from test_pls_off_cfg import mode_cfgs as cfgs

    return cfgs(task, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_go2env_pls_off_4096_envs(libs_built, mode):
    from go2_sim2real_locomotion_rl_amd import Go2Env, init

    init(precision="32", seed=1)
    B, steps = 4096, 300
    cfgs = mode_cfgs(mode)
    cfgs[0]["episode_length_s"] = 2.0                                      # time-outs inside the run; staggered like rsl_rl's init_at_random_ep_len
    env = Go2Env(B, *cfgs, seed=7)
    assert not env.is_base_env and env.num_actions == 12 and env.num_obs == 45 and env.num_privileged_obs == 100
    gen = torch.Generator(device="cuda").manual_seed(3)
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (B,), device="cuda", generator=gen)
    n_checked, last = 0, None
    for s in range(steps):
        actions = 0.6 * torch.randn(B, 12, device="cuda", generator=gen)
        obs, rew, reset, extras = env.step(actions)
        assert obs.shape == (B, 45) and extras["observations"]["critic"].shape == (B, 100)
        if mode == "B":
            kp, kd = (float(v) for v in env.engine_gains)
            rst = reset.cpu().numpy().astype(bool)
            if rst.any():
                bkp, bkd = (t.cpu().numpy().astype(np.float64) for t in env.base_gains)
                exp = (np.float32(bkp[rst].sum() / rst.sum()), np.float32(bkd[rst].sum() / rst.sum()))
                assert (np.float32(kp), np.float32(kd)) == exp, f"step {s}: batch gains {(kp, kd)} vs mean {exp}"
                n_checked += 1
            elif last is not None:
                assert (kp, kd) == last, f"step {s}: no reset, yet the batch gains moved"
            last = (kp, kd)
        if s % 50 == 49 or s == steps - 1:
            torch.cuda.synchronize()
            assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and torch.isfinite(extras["observations"]["critic"]).all()
    assert env.check_errno() == 0
    if mode == "B":
        assert n_checked >= 250, n_checked
        bkp, _ = env.base_gains
        assert len(torch.unique(bkp)) > 100, "per-env gains are drawn per env"
    if mode == "A":
        bkp, bkd = env.base_gains
        lo, hi = env.env_cfg["kp_range"]
        assert len(torch.unique(bkp)) > 100 and float(bkp.min()) >= min(lo, 0.9 * 60.0) and float(bkp.max()) <= max(hi, 1.1 * 60.0)


@pytest.mark.gpu
def test_closed_loop_pls_off(libs_built):
    from go2_sim2real_locomotion_rl_amd import ActorCritic, Go2Env, RolloutStorage, init

    device = init(precision="32", seed=1)
    B, T = 1024, 24
    env = Go2Env(B, *mode_cfgs("A"), seed=5)
    policy = ActorCritic(45, 100, 12, [512, 256, 128], [512, 256, 128], activation="elu", init_noise_std=0.3, device=device, seed=1)
    storage = RolloutStorage(T, B)
    obs, extras = env.get_observations()
    priv = extras["observations"]["critic"]
    for t in range(T):
        a = policy.act(obs, priv)
        assert a.shape == (B, 12)
        obs, rew, rst, extras = env.step(a)
        priv = extras["observations"]["critic"]
        storage.add_transitions(t, rew, rst, policy.values, extras["time_outs"], gamma=0.99)
    ret, adv = storage.compute_returns(policy.evaluate(priv), 0.99, 0.95)
    torch.cuda.synchronize()
    assert torch.isfinite(ret).all() and torch.isfinite(adv).all() and env.check_errno() == 0
