"""The LIDAR scan next to the env kernels (64 envs, 30 steps, falls included): (a) on the stair env's own poses and its 11 x 7 grid the scanner's
critic scan IS the env kernel's privileged height scan, bit for bit; (b) the LIDAR env is the stair env plus scan columns -- every proprioceptive and
privileged column, the rewards and the resets are bit-equal, and the scan columns are lidar_ref's on the read-back poses; (c) the runner trains on it,
plain, with the mirror tables and with empirical normalisation."""
import copy

import numpy as np
import pytest
import torch

import lidar_ref as R
from test_ppo_gpu import TRAIN_CFG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, STEPS, SEED = 64, 30, 11


def harsh(cfgs):
    """Both envs of a comparison get the same two keys changed, so that random actions make envs fall inside the 30 steps: the roll and pitch limits."""
    cfgs = copy.deepcopy(cfgs)
    cfgs[0].update({"termination_if_roll_greater_than": 10, "termination_if_pitch_greater_than": 10})
    return cfgs


def actions(t, num_actions=16):
    g = torch.Generator().manual_seed(100 + t)
    return (1.5 * torch.randn(B, num_actions, generator=g)).to(DEV)


def bits(x):
    return x.detach().contiguous().cpu().numpy().view(np.uint32)


def test_critic_scan_is_the_env_kernels_height_scan_bit_for_bit():
    from go2_sim2real_locomotion_rl_amd import Go2Env, LidarScan, get_stair_cfgs, init
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain
    from go2_sim2real_locomotion_rl_amd.lidar import env_pose_ptrs

    init(seed=SEED)
    cfgs = harsh(get_stair_cfgs())
    env = Go2Env(B, *cfgs, seed=SEED)
    hf, info = build_stair_terrain(cfgs[0]["terrain"])
    cfg = {"enabled": True, "actor_scan": {"x_points": [0.0], "y_points": [0.0]}, "critic_scan": dict(cfgs[0]["terrain"]["height_scan"]),
           "height_clip": 1e30, "height_scale": 1.0}                      # the legacy grid, a clip that cannot act, no scaling
    scan = LidarScan(cfg, B, hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"], seed=SEED, device=DEV)
    assert scan.n_critic == 77
    pos, quat, cs = env_pose_ptrs(env._sim)
    assert cs == B
    actor, both = torch.empty(B, 1, device=DEV), torch.empty(B, 78, device=DEV)
    compared = resets = 0
    for t in range(STEPS):
        _, _, reset, _ = env.step(actions(t))
        scan.step(pos, (cs, 1), quat, (cs, 1), None, None, None, None, 0, actor, both)          # the env's own buffers, read in place
        live = (reset == 0).cpu().numpy()
        legacy = env.privileged_obs_buf[:, 105:182]
        assert np.array_equal(bits(both[:, 1:])[live], bits(legacy)[live]), f"step {t}"
        assert np.abs(legacy.cpu().numpy()[live]).max() > 0.1           # the scan sees the robot's height above the terrain, not zeros
        compared, resets = compared + int(live.sum()), resets + int((~live).sum())
    print(f"compared {compared} env steps bit for bit, {resets} resets")
    assert resets > 0 and compared > STEPS * B // 2
    assert env.check_errno() == 0


def test_lidar_env_is_the_stair_env_plus_the_scans():
    """The two cfgs differ in `lidar`, `terrain.height_scan` and the widths only (tests/test_lidar_ref.py holds get_stair_lidar_cfgs to that); both get
    the roll / pitch limits of `harsh`."""
    from go2_sim2real_locomotion_rl_amd import Go2Env, get_stair_cfgs, get_stair_lidar_cfgs, init
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain
    from go2_sim2real_locomotion_rl_amd.lidar import lidar_layout

    init(seed=SEED)
    lcfgs, scfgs = harsh(get_stair_lidar_cfgs()), harsh(get_stair_cfgs())
    lenv, senv = Go2Env(B, *lcfgs, seed=SEED), Go2Env(B, *scfgs, seed=SEED)
    assert (lenv.num_obs, lenv.num_privileged_obs) == (64, 165) and lenv.obs_buf.shape == (B, 64) and lenv.privileged_obs_buf.shape == (B, 165)
    hf, info = build_stair_terrain(lcfgs[0]["terrain"])
    P = {"hf": hf, "origin": info["terrain_origin"], "h_scale": info["horizontal_scale"], "v_scale": info["vertical_scale"]}
    lay = lidar_layout(lcfgs[0]["lidar"])
    N = dict(lcfgs[0]["lidar"]["noise"], height_clip=1.0, height_scale=1.0)
    prev = np.zeros((B, 15), np.float32)
    stats = {"dropout": 0, "latency": 0, "blackout": 0, "reset": 0}
    worst_all = 0.0
    for t in range(STEPS):
        a = actions(t)
        lo, lr, lreset, lex = lenv.step(a)
        so, sr, sreset, sex = senv.step(a)
        lp, sp = lenv.privileged_obs_buf, senv.privileged_obs_buf
        assert lex["observations"]["critic"] is lp and lo is lenv.obs_buf
        assert np.array_equal(bits(lo[:, :49]), bits(so)), f"step {t}: proprioceptive columns"
        assert np.array_equal(bits(lp[:, :49]), bits(sp[:, :49])) and np.array_equal(bits(lp[:, 64:120]), bits(sp[:, 49:105])), f"step {t}: privileged columns"
        assert np.array_equal(bits(lr), bits(sr)) and torch.equal(lreset, sreset) and torch.equal(lex["time_outs"], sex["time_outs"]), f"step {t}"
        assert np.array_equal(bits(lp[:, 49:64]), bits(lo[:, 49:]))
        # the scan columns against lidar_ref on the read-back poses, level and reset flags
        pos, quat, reset = lenv.base_pos.cpu().numpy(), lenv.base_quat.cpu().numpy(), lreset.cpu().numpy()
        L = R.dr_level(float(lenv.curriculum_level), lcfgs[0]["dr_schedule"], True)
        d = R.draws(B, 15, SEED, t)
        v, tol, amb, masks = R.actor_scan(P, N, pos, quat, lay["actor_xy"], L, d, prev, reset)
        ok, worst = R.match(lo[:, 49:].cpu().numpy(), v, tol)
        vc, tolc, ambc = R.critic_scan(P, N, pos, quat, lay["critic_xy"], reset)
        okc, worstc = R.match(lp[:, 120:].cpu().numpy(), vc, tolc)
        print(f"step {t}: L {L:.4f}, actor worst ratio {worst:.3f} (ambiguous {int(amb.sum())}), critic {worstc:.3f} (ambiguous {int(ambc.sum())}), resets {int(reset.sum())}")
        assert ok.all() and okc.all(), f"step {t}"
        for k in stats:
            stats[k] += int(masks[k].sum())
        worst_all = max(worst_all, worst, worstc)
        prev = lo[:, 49:].cpu().numpy()
        assert lenv._lidar.step_count == t + 1
    print(f"fired: {stats}, worst ratio {worst_all:.3f}")
    assert stats["reset"] > 0 and stats["dropout"] > 0 and L > 0
    assert np.array_equal(lenv._lidar.stored_scan().numpy().view(np.uint32), bits(lenv.obs_buf[:, 49:]))
    # reset_idx and reset clear the stored scan of their envs, as the reference's reset_idx zeroes the buffers
    keep = lenv._lidar.stored_scan().numpy().copy()
    lenv.reset_idx([1, 5])
    s = lenv._lidar.stored_scan().numpy()
    assert not s[[1, 5]].any() and np.array_equal(np.delete(s, [1, 5], 0), np.delete(keep, [1, 5], 0))
    lenv.respawn([2], [[1.0, 0.0, 0.5]])
    assert not lenv._lidar.stored_scan().numpy()[2].any()
    lenv.reset()
    assert not lenv._lidar.stored_scan().numpy().any()
    assert lenv.check_errno() == 0 and senv.check_errno() == 0


def test_a_cfg_whose_widths_disagree_is_refused_by_name():
    from go2_sim2real_locomotion_rl_amd import Go2Env, Go2SimError, get_stair_lidar_cfgs, init

    init(seed=SEED)
    env_cfg, obs_cfg, reward_cfg, command_cfg = get_stair_lidar_cfgs()
    obs_cfg["num_privileged_obs"] = 182
    with pytest.raises(Go2SimError, match=r"64 / 182.*64 / 165"):
        Go2Env(B, env_cfg, obs_cfg, reward_cfg, command_cfg, seed=SEED)


@pytest.mark.parametrize("variant", ["plain", "symmetry", "normalization", "pls_off"])
def test_runner_trains_on_the_lidar_env(variant, tmp_path):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_stair_lidar_cfgs, init, read_checkpoint

    init(seed=SEED)
    pls = variant != "pls_off"
    env = Go2Env(B, *get_stair_lidar_cfgs(pls_enable=pls), seed=SEED)
    width = 64 if pls else 60
    cfg = copy.deepcopy(TRAIN_CFG)
    if variant == "symmetry":
        cfg["algorithm"]["symmetry_cfg"] = {"use_data_augmentation": True, "use_mirror_loss": True, "mirror_loss_coeff": 0.5, "mirror_tables": env.mirror_tables()}
    if variant == "normalization":
        cfg["empirical_normalization"] = True
    runner = OnPolicyRunner(env, cfg)
    log = runner.learn(2)
    assert len(log) == 2 and all(np.isfinite(v) for d in log for v in (d["value_loss"], d["surrogate_loss"], d["entropy"]))
    path = str(tmp_path / "model_2.pt")
    runner.save(path)
    ck = read_checkpoint(path)
    assert ck["model_state_dict"]["actor.0.weight"].shape[1] == width and ck["model_state_dict"]["critic.0.weight"].shape[1] == width + 101
    if variant == "normalization":
        assert ck["obs_norm_state_dict"]["_mean"].shape == (1, width) and int(ck["obs_norm_state_dict"]["count"]) == 2 * 8 * B
    again = OnPolicyRunner(Go2Env(B, *get_stair_lidar_cfgs(pls_enable=pls), seed=SEED), cfg)
    again.load(path)
    a, b = runner.policy.state_dict(), again.policy.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)
    assert env.check_errno() == 0
