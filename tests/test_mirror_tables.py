"""Go2Env.mirror_tables (go2_env.mirror_tables): the tables of the four layouts against tables written out entry by entry
(tests/ppo_sym_cases.py), their algebra, and a structural twin check of the env's real observation layout on the strict CPU oracle: two envs in
mirrored states, stepped once with mirrored actions, give mirrored observations -- entry by entry, through the tables."""
import copy

import numpy as np
import pytest
import torch

import go2_sim2real_locomotion_rl_amd.genesis_shim as gs
from go2_sim2real_locomotion_rl_amd.capi import Go2SimError
from go2_sim2real_locomotion_rl_amd.configs import flatten_walk_cfg, get_crouch_cfgs, get_jump_cfgs, get_stair_cfgs, get_walk_cfgs
from go2_sim2real_locomotion_rl_amd.go2_env import Go2Env, mirror_tables

import ppo_sym_cases as SC
from util import gs_on_oracle

LAYOUTS = {"walk": (get_walk_cfgs, 49, 104, 16), "pls_off": (lambda: get_walk_cfgs(pls_enable=False), 45, 100, 12),
           "stairs": (get_stair_cfgs, 49, 182, 16), "base": (get_crouch_cfgs, 45, 45, 12)}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_tables_equal_the_literal_ones(name):
    make, n_obs, n_critic, n_act = LAYOUTS[name]
    env_cfg, obs_cfg = make()[:2]
    got, want = mirror_tables(env_cfg, obs_cfg), SC.ENV_TABLES[name]
    assert set(got) == {"policy", "critic", "actions"}
    for key, width in (("policy", n_obs), ("critic", n_critic), ("actions", n_act)):
        src, sign = got[key]
        assert src.dtype == torch.int32 and sign.dtype == torch.float32 and src.shape == sign.shape == (width,)
        assert torch.equal(src, want[key][0]) and torch.equal(sign, want[key][1]), key
        assert set(sign.tolist()) <= {1.0, -1.0}
        assert torch.equal(src[src.long()].long(), torch.arange(width)) and torch.equal(sign[src.long()] * sign, torch.ones(width)), "an involution"
    assert (n_obs, n_act) == (obs_cfg["num_obs"], env_cfg["num_actions"]) and n_critic == (obs_cfg.get("num_privileged_obs") or n_obs)


def test_other_layouts_and_the_method():
    stairs_off = mirror_tables(*get_stair_cfgs(pls_enable=False)[:2])
    assert [len(stairs_off[k][0]) for k in ("policy", "critic", "actions")] == [45, 178, 12]
    assert torch.equal(stairs_off["critic"][0][101:], SC.ENV_TABLES["stairs"]["critic"][0][105:] - 4)      # the same scan, four entries earlier
    jump = mirror_tables(*get_jump_cfgs()[:2])
    assert all(torch.equal(jump[k][0], SC.ENV_TABLES["base"][k][0]) for k in jump)
    env_cfg, obs_cfg = get_stair_cfgs()[:2]
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg["terrain"]["height_scan"]["y_range"] = [-0.2, 0.3]
    with pytest.raises(Go2SimError, match="y_range"):
        mirror_tables(env_cfg, obs_cfg)
    env = Go2Env.__new__(Go2Env)                               # the method reads the cfg dicts the env was constructed with, nothing of the device
    env.env_cfg, env.obs_cfg = get_walk_cfgs()[:2]
    assert all(torch.equal(env.mirror_tables()[k][0], SC.ENV_TABLES["walk"][k][0]) for k in ("policy", "critic", "actions"))


# ---- the twin check --------------------------------------------------------------------------------------------------------------------------
BLOCKS = {"ang_vel": (0, 3), "gravity": (3, 6), "commands": (6, 9), "dof_pos": (9, 21), "dof_vel": (21, 33), "actions": (33, 49), "lin_vel": (49, 52)}


def _spread(n, lo, hi, g):
    """n values of either sign whose magnitudes are evenly spaced in [lo, hi], in a random order"""
    mags = torch.linspace(lo, hi, n)[torch.randperm(n, generator=g)]
    return mags * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def twin_observations(oracle_lib, seed):
    """Two walk envs on the strict oracle, 1 m above the ground (nothing touches), noise, domain randomisation, pushes and delay off; env 1 holds the
    mirror image of env 0's state, command and action.  -> the privileged observations [2][104] after one env step, the tables"""
    gs_on_oracle(gs, oracle_lib, seed=3)
    cfgs = get_walk_cfgs()
    env_cfg, obs_cfg = cfgs[0], cfgs[1]
    for k in ("friction_range", "kp_factor_range", "kd_factor_range", "kp_range", "kd_range", "mass_shift_range", "com_shift_range", "leg_mass_shift_range",
              "gravity_offset_range", "motor_strength_range", "obs_noise", "push_force_range"):
        env_cfg.pop(k, None)
    env_cfg.update(action_noise_std=0.0, min_delay_steps=0, max_delay_steps=0)
    env_cfg["curriculum"] = dict(env_cfg.get("curriculum", {}), enabled=False, delay_easy_max_steps=0)
    f, i, _ = flatten_walk_cfg(2, *cfgs)
    scene = gs.Scene(sim_options=gs.options.SimOptions(dt=0.02, substeps=2),
                     rigid_options=gs.options.RigidOptions(dt=0.02, constraint_solver=gs.constraint_solver.Newton, enable_collision=True,
                                                           enable_joint_limit=True, max_collision_pairs=30), show_viewer=False)
    scene.add_entity(gs.morphs.URDF(file="urdf/plane/plane.urdf", fixed=True))
    robot = scene.add_entity(gs.morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=np.array(env_cfg["base_init_pos"]), quat=np.array(env_cfg["base_init_quat"])))
    scene.build(n_envs=2)
    sim = scene._sim
    sim.env_configure(f, i)
    sim.env_reset()
    tables = mirror_tables(env_cfg, obs_cfg)
    a_src, a_sign = tables["actions"][0].long(), tables["actions"][1]
    j_src, j_sign = a_src[:12], a_sign[:12]
    motors = [robot.get_joint(n).dof_start for n in env_cfg["joint_names"]]
    default = torch.tensor([env_cfg["default_joint_angles"][n] for n in env_cfg["joint_names"]])
    assert torch.equal(default, j_sign * default[j_src]), "the default pose is its own mirror image"
    g = torch.Generator().manual_seed(seed)
    # The env's PD law reads the joint state it cached at the last reset (the default pose at rest), so an action is a torque held for the whole step:
    # the actions are kept small (their block is judged on its own scale) and the joints coast.  Slow joints and a slowly turning base keep the
    # velocity-product terms small, so the observed positions and velocities keep the separation they are given here.
    act = 1e-3 * _spread(16, 0.15, 1.0, g)
    q_off, q_vel = _spread(12, 0.08, 0.52, g), _spread(12, 0.05, 0.3, g)
    pos, lin, ang, cmd = torch.tensor([0.3, 0.2, 1.0]), torch.tensor([0.4, -0.25, 0.15]), torch.tensor([0.05, -0.09, 0.07]), torch.tensor([0.6, -0.25, 0.45])
    axis, angle = torch.tensor([0.3, -0.5, 0.8]) / torch.tensor([0.3, -0.5, 0.8]).norm(), 0.35
    quat = torch.cat([torch.tensor([np.cos(angle / 2)], dtype=torch.float32), axis * float(np.sin(angle / 2))])
    m = lambda v, s: v * torch.tensor(s)
    robot.set_pos(torch.stack([pos, m(pos, [1.0, -1.0, 1.0])]), zero_velocity=False)
    robot.set_quat(torch.stack([quat, m(quat, [1.0, -1.0, 1.0, -1.0])]), zero_velocity=False)
    robot.set_dofs_position(torch.stack([default + q_off, default + j_sign * q_off[j_src]]), motors, zero_velocity=False)
    v = robot._get("F_VEL")                                    # [18][2]: base linear, base angular, joints
    v[0:3, 0], v[0:3, 1] = lin, m(lin, [1.0, -1.0, 1.0])
    v[3:6, 0], v[3:6, 1] = ang, m(ang, [-1.0, 1.0, -1.0])
    qv_b = j_sign * q_vel[j_src]
    for k, d in enumerate(motors):
        v[d, 0], v[d, 1] = q_vel[k], qv_b[k]
    robot._set("F_VEL", v)
    robot._after_state_write(torch.arange(2))
    sim.env_set_commands(torch.stack([cmd, m(cmd, [1.0, -1.0, -1.0])]).numpy())
    obs, priv = np.zeros((2, 49), np.float32), np.zeros((2, 104), np.float32)
    rew, rst, to = np.zeros(2, np.float32), np.zeros(2, np.uint8), np.zeros(2, np.float32)
    sim.env_step(np.ascontiguousarray(torch.stack([act, a_sign * act[a_src]]).numpy()), obs, priv, rew, rst, to)
    assert not rst.any() and np.array_equal(obs, priv[:, :49])
    return priv, tables


def test_twin_envs_give_mirrored_observations(oracle_strict_lib):
    priv, tables = twin_observations(oracle_strict_lib, TWIN_SEED)
    a, b = priv[0].astype(np.float64), priv[1].astype(np.float64)
    src, sign = tables["critic"][0].numpy(), tables["critic"][1].numpy().astype(np.float64)
    for name, (lo, hi) in BLOCKS.items():
        blk = a[lo:hi]
        scale = np.abs(blk).max()
        cands = np.concatenate([blk, -blk])                    # every +- obs_A[k] of the block
        d = np.abs(cands[:, None] - cands[None, :])[np.triu_indices(len(cands), 1)]
        assert d.min() >= 0.05 * scale, f"{name}: the block's values are not separated ({d.min() / scale:.3f} of its scale)"
        for j in range(lo, hi):
            assert lo <= src[j] < hi
            want = sign[j] * a[src[j]]
            others = np.delete(cands, (src[j] - lo) if sign[j] > 0 else (hi - lo) + (src[j] - lo))
            near, other = abs(b[j] - want), np.abs(b[j] - others).min()
            assert 10.0 * near <= other, f"{name}[{j - lo}]: {near:.3e} from its mirror source, {other:.3e} from another entry"
    # the fixed points and leg swaps of the rest of the critic input (constants here: randomisation is off)
    assert np.array_equal(priv[1, 52:], (sign * a[src])[52:].astype(np.float32))


TWIN_SEED = 2
