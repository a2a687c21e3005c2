"""What Go2Env promises of every launch it runs after the step's own (LIDAR scan, stair info, stairwell scan with alive, contact terms), on 4 envs:
after 3 steps, reset_idx([2]), respawn([1], clear_buffers=True) and respawn([3], clear_buffers=False), each handle's stored state is read back and
held bit for bit -- a cleared env's stored rows are zero, its episode terms are handed over (ep = sum / (f32(max(steps, 1)) * f32(dt)) in float32, then
sum and steps 0), every other env's cells stay, and clear_buffers=False changes nothing.  Before the three calls the episode sums and counts are set to
values that make the law visible (a count of 0 on the env respawned with clear_buffers=True: max(steps, 1)).  One further case: in a stairwell env with
alive and stumble both on, rew_buf is the core's reward, plus the alive increment, plus the stumble term, added in that order in float32."""
import numpy as np
import pytest
import torch

import cterms_ref as R
from test_cterms_env_gpu import robot_forces, same, with_scale

pytestmark = pytest.mark.gpu
B, SEED, DT = 4, 11, np.float32(0.02)
SUMS = np.array([[0.25, -1.5, 3.0, -0.125], [-7.0, 0.375, -0.0625, 11.0]], np.float32)      # per term and env


def make_cfgs(case):
    from go2_sim2real_locomotion_rl_amd import get_rough_cfgs, get_stair_info_cfgs, get_stair_lidar_cfgs, get_stairwell_cfgs

    return {"stairs_lidar": get_stair_lidar_cfgs, "stairs_info": get_stair_info_cfgs, "stairs_info_body_contact": lambda: get_stair_info_cfgs(script_values=True),
            "stairwell_alive": get_stairwell_cfgs, "rough_stumble": lambda: with_scale(get_rough_cfgs("grid"), "stumble", -1.0)}[case]()


def read(env):
    """{name: [arrays]} of every handle's stored state; episode terms as (sum, steps, ep), each [terms, B]"""
    from go2_sim2real_locomotion_rl_amd.go2_env import _as_device_tensor

    out = {}
    if env._lidar is not None:
        out["lidar rows"] = [env._lidar.stored_scan().numpy().copy()]
    if env._stairinfo is not None:
        out["stairinfo rows"] = [env._stairinfo.stored_rows().numpy().copy()]
    if env._wells is not None:
        s, k = env._wells.alive_state()
        ep = _as_device_tensor(env._wells.alive_ep_ptr, (B,), torch.float32, env.device).cpu().numpy()
        out["alive terms"] = [s.numpy()[None].copy(), k.numpy()[None].copy(), ep[None].copy()]
    if env._cterms is not None:
        out["contact terms"] = [x.numpy().copy() for x in env._cterms.state()]
    return out


def check_cleared(before, after, cleared, what):
    """`cleared`: the envs the call cleared (none: nothing may change)"""
    keep = [b for b in range(B) if b not in cleared]
    assert set(before) == set(after)
    for name, arrs in before.items():
        for x, y in zip(arrs, after[name]):
            assert np.array_equal(x[..., keep].view(np.uint32) if name.endswith("terms") else x[keep].view(np.uint32),
                                  y[..., keep].view(np.uint32) if name.endswith("terms") else y[keep].view(np.uint32)), f"{what}: {name} of another env changed"
        for b in cleared:
            if name.endswith("rows"):
                assert x[b].any() and not after[name][0][b].any(), f"{what}: {name} of env {b}"
            else:
                (s0, k0, _), (s1, k1, e1) = arrs, after[name]
                want = s0[:, b] / (np.maximum(k0[:, b], 1).astype(np.float32) * DT)
                assert same(e1[:, b], want) and not s1[:, b].any() and not k1[:, b].any(), f"{what}: {name} of env {b}: {e1[:, b]} vs {want}"


@pytest.mark.parametrize("case", ["stairs_lidar", "stairs_info", "stairs_info_body_contact", "stairwell_alive", "rough_stumble"])
def test_clears_hand_over_and_leave_the_rest(case):
    from go2_sim2real_locomotion_rl_amd import Go2Env, init

    init(seed=SEED)
    np.random.seed(4)                                                        # the grid's tiles are drawn from numpy's global generator
    env = Go2Env(B, *make_cfgs(case), seed=SEED)
    handles = {"stairs_lidar": ["_lidar"], "stairs_info": ["_stairinfo"], "stairs_info_body_contact": ["_stairinfo", "_cterms"],
               "stairwell_alive": ["_wells"], "rough_stumble": ["_cterms"]}[case]
    assert [n for n in ("_lidar", "_stairinfo", "_wells", "_cterms") if getattr(env, n) is not None] == handles
    g = torch.Generator().manual_seed(5)
    for t in range(3):
        before = read(env)
        _, _, reset, _ = env.step((0.3 * torch.randn(B, env.num_actions, generator=g)).to(env.device))
        after, reset = read(env), reset.cpu().numpy()
        for name, arrs in after.items():
            for b in range(B):
                if name.endswith("rows"):
                    assert reset[b] == 0 or not arrs[0][b].any(), f"step {t}: {name} of the reset env {b}"
                else:                                                        # an applied term counts the step; a reset hands the episode over
                    on = np.array(env._cterms.active if name == "contact terms" else [True])
                    want = np.where(on, 0 if reset[b] else before[name][1][:, b] + 1, 0)
                    assert np.array_equal(arrs[1][:, b], want), f"step {t}: {name} of env {b}: steps {arrs[1][:, b]} vs {want}"
    assert env.check_errno() == 0
    if env._wells is not None:
        env._wells.set_alive_state(torch.from_numpy(SUMS[0]), torch.tensor([3, 0, 5, 7], dtype=torch.int32))
    if env._cterms is not None:
        _, _, ep = env._cterms.state()
        env._cterms.set_state(torch.from_numpy(SUMS), torch.tensor([[3, 0, 5, 7], [2, 0, 1, 9]], dtype=torch.int32), ep)
    pos = env.base_pos.clone()
    for what, call, cleared in (("reset_idx([2])", lambda: env.reset_idx([2]), [2]),
                                ("respawn([1], clear_buffers=True)", lambda: env.respawn([1], pos[[1]], clear_buffers=True), [1]),
                                ("respawn([3], clear_buffers=False)", lambda: env.respawn([3], pos[[3]], clear_buffers=False), [])):
        before = read(env)
        call()
        check_cleared(before, read(env), cleared, what)
    assert env.check_errno() == 0


def test_alive_then_stumble_in_a_stairwell_env():
    """`other` is the same env without the two keys: its reward is the core's.  Both are laid on their side just above their wells' floors, with roll and
    pitch limits of 120 degrees, so that links that are no feet press on the ground inside the steps."""
    from go2_sim2real_locomotion_rl_amd import Go2Env, get_stairwell_cfgs, init

    init(seed=SEED)
    cfgs = with_scale(get_stairwell_cfgs(), "stumble", -1.0)
    cfgs[0].update({"termination_if_roll_greater_than": 120, "termination_if_pitch_greater_than": 120})
    assert list(cfgs[2]["reward_scales"])[-2:] == ["alive", "stumble"]
    env, other = Go2Env(B, *cfgs, seed=SEED), Go2Env(B, *with_scale(with_scale(cfgs, "stumble", None), "alive", None), seed=SEED)
    assert env._wells is not None and env._cterms is not None and other._cterms is None and "rew_alive" not in other.extras["episode"]
    levels = torch.arange(B) % 9
    spawn = torch.tensor(env._terrain_info["row_centers"], dtype=torch.float32)[levels] + torch.tensor([0.0, 0.0, 0.15])
    side = torch.tensor([[np.cos(np.pi / 4), np.sin(np.pi / 4), 0.0, 0.0]], dtype=torch.float32).expand(B, 4)       # rolled by 90 degrees
    for e in (env, other):
        e.set_terrain_rows(levels)
        e.respawn(torch.arange(B), spawn, side)
    alive, inc = np.float32(env._wells.inc), R.inc32(-1.0)
    assert alive == R.inc32(cfgs[2]["reward_scales"]["alive"]) and alive != 0
    g, pressed = torch.Generator().manual_seed(6), 0
    for t in range(12):
        a = (0.3 * torch.randn(B, env.num_actions, generator=g)).to(env.device)
        _, r1, d1, _ = env.step(a)
        _, r0, d0, _ = other.step(a)
        F = robot_forces(env)
        assert torch.equal(d1, d0) and np.isfinite(F).all() and same(F, robot_forces(other)), f"step {t}: the two envs part"
        _, pen = R.law32(F, R.THIGHS, R.NON_FEET)
        want = (r0.cpu().numpy() + alive) + pen * inc
        assert same(r1.cpu().numpy(), want), f"step {t}: rew {r1.cpu().numpy()} vs core + alive + stumble {want}"
        pressed += int((pen > 0).sum())
    print(f"stairwell, alive then stumble: {pressed} env-steps with a stumble term")
    assert pressed > 0 and env.check_errno() == 0 and other.check_errno() == 0
