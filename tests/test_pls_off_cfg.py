"""The walk / stair envs with per-leg stiffness off (`pls_enable=False`, go2_train_walk.py:77, go2_train_stair.py:72): routing, layouts and flags.

Three control modes (go2_env_walk.py:519, 758-801, 1007-1021): A -- kp_factor_range set: manual PD on per-env base x factor gains; B -- no
kp_factor_range, kp_range set: engine PD whose motor gains are the mean effective gain of each reset call; C -- neither: engine PD on env_cfg kp / kd.
CPU only; the GPU side is tests/test_pls_off_gpu.py."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.capi import C, Go2SimError
from go2_sim2real_locomotion_rl_amd.configs import flatten_walk_cfg, get_crouch_cfgs, get_jump_cfgs, get_stair_cfgs, get_walk_cfgs
from go2_sim2real_locomotion_rl_amd.go2_env import is_base_env_cfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOPLS_CASES = ["walk_nopls", "walk_nopls_engine", "walk_nopls_static", "stairs_nopls", "walk_nopls_rng", "walk_nopls_engine_rng"]


def mode_cfgs(task, mode):
    cfgs = copy.deepcopy((get_stair_cfgs if task == "stairs" else get_walk_cfgs)(pls_enable=False))
    env_cfg = cfgs[0]
    if mode in "BC":
        env_cfg.pop("kp_factor_range"); env_cfg.pop("kd_factor_range")
    if mode == "C":
        env_cfg.pop("kp_range"); env_cfg.pop("kd_range")
    return cfgs


@pytest.mark.parametrize("task", ["walk", "stairs"])
@pytest.mark.parametrize("mode", ["A", "B", "C"])
def test_pls_off_cfgs_flatten_with_the_right_flags(task, mode):
    env_cfg, obs_cfg, reward_cfg, command_cfg = mode_cfgs(task, mode)
    assert env_cfg["num_actions"] == 12 and obs_cfg["num_obs"] == 45                       # go2_train_walk.py:83-84, 305
    assert obs_cfg["num_privileged_obs"] == (178 if task == "stairs" else 100)           # :309; go2_train_stair.py:282-299
    assert not is_base_env_cfg(env_cfg, obs_cfg), "a PLS-off walk / stair cfg has the base env's 12 / 45 shape but is the walk family"
    f, i, _ = flatten_walk_cfg(4096, env_cfg, obs_cfg, reward_cfg, command_cfg)
    I = lambda n: int(i[C["GO2SIM_IC_" + n]])
    assert (I("ENV_KIND"), I("PLS_ENABLE"), I("NUM_ACTIONS"), I("NUM_OBS"), I("NUM_PRIV_OBS")) == (0, 0, 12, 45, obs_cfg["num_privileged_obs"])
    assert (I("MANUAL_PD"), I("ENGINE_BATCH_GAIN"), I("HAS_KP_RANGE")) == {"A": (1, 0, 1), "B": (0, 1, 1), "C": (0, 0, 0)}[mode]
    assert I("HAS_KPF_DR") == I("HAS_KDF_DR") == int(mode == "A")


def test_base_cfgs_still_route_to_the_base_env():
    for cfgs in (get_crouch_cfgs(), get_jump_cfgs()):
        assert is_base_env_cfg(cfgs[0], cfgs[1])
    for fn in (get_walk_cfgs, get_stair_cfgs):
        assert not is_base_env_cfg(*fn()[:2])


@pytest.mark.parametrize("task", ["walk", "stairs"])
@pytest.mark.parametrize("num_envs", [4096, 16])
def test_pls_on_cfgs_flatten_as_before(task, num_envs):
    """Byte-identical to what flatten_walk_cfg produced before the PLS-off modes existed (digest recorded then); the int entries appended since
    (GO2SIM_IC_ENGINE_BATCH_GAIN) are zero."""
    ref = json.load(open(os.path.join(GOLDEN, "pls_on_flatten_digest.json")))
    f, i, _ = flatten_walk_cfg(num_envs, *(get_stair_cfgs if task == "stairs" else get_walk_cfgs)())
    assert len(f) == ref["fc_count"] and len(i) >= ref["ic_count"]
    digest = ref[f"{task}_{num_envs}"]
    assert hashlib.sha256(f.astype("<f8").tobytes()).hexdigest() == digest["f_sha256"]
    assert hashlib.sha256(i[:ref["ic_count"]].astype("<i4").tobytes()).hexdigest() == digest["i_sha256"]
    assert not np.any(i[ref["ic_count"]:])


def test_batch_gain_with_shared_globals_raises():
    with pytest.raises(Go2SimError, match="shared_globals"):
        flatten_walk_cfg(64, *mode_cfgs("walk", "B"), shared_globals=True)
    flatten_walk_cfg(64, *mode_cfgs("walk", "A"), shared_globals=True)      # per-env gains shard like every other per-env draw


def test_batch_gain_ranges_are_checked():
    """The exact float64 sum of k_env_engine_gains needs effective gains in [1, 128) and at most 2^23 / 12 envs."""
    cfgs = mode_cfgs("walk", "B")
    cfgs[0]["kd_range"] = [0.5, 5.0]
    with pytest.raises(ValueError, match=r"\[1, 128\)"):
        flatten_walk_cfg(64, *cfgs)
    with pytest.raises(ValueError, match="envs"):
        flatten_walk_cfg((1 << 23) // 12 + 1, *mode_cfgs("walk", "B"))


@pytest.mark.parametrize("case", NOPLS_CASES)
def test_nopls_fixtures_are_what_the_reference_files_produce(case):
    """As test_ref_env_fixtures.test_fixtures_are_what_the_reference_files_produce for the PLS-off cases: the committed script's cfg dicts and action
    tape are the stored ones; with GO2SIM_REFERENCE_DIR set, the reference's env file is re-run for the first 30 steps as well."""
    from test_ref_env_fixtures import check_generator_inputs, fixture_generator, load_fixture

    M = fixture_generator()
    check_generator_inputs(M, case, M.rng_cfgs(case) if case.endswith("_rng") else M.pinned_cfgs(case))
    z, cfgs, meta = load_fixture(case, "fast")
    assert z["actions"].shape[2] == 12 and z["obs"].shape[2] == 45
    if "_engine" in case:
        assert meta["gain_mean_checks"] >= 2 * 4, "the record-time mean check ran on several reset calls"
    if M.REF_DIR is None:
        return
    assert os.path.isdir(M.REF_DIR), f"GO2SIM_REFERENCE_DIR holds no {os.path.relpath(M.REF_DIR, M.REF_ROOT)}"
    out, _ = M.run_case(case, B=meta["n_envs"], T=meta["steps"], seed=meta["seed"], n_run=30, physics="fast")
    for key in ("obs", "priv", "rew", "rew_terms", "done", "time_outs", "ctrl_pos", "ctrl_force", "commands", "base_pos", "episode_length", "engine_gains"):
        assert np.array_equal(out[key], z[key][:30]), key
