"""The collision broad phase runs at the end of every forward-dynamics pass (tk_broadphase in k_pre_dynamics_team / k_dynamics_team / the dynamics
tail of k_solve_integrate_team and k_integrate_fk_dynamics_team) and k_collide_team starts at the narrow phase on the pair list it left in `broad`.
Everything the broad phase owns -- the persistent sort buffers, the pair count, the cleared contact slots, the normal-cache mask, first_time, the
overflow errno -- and everything the narrow phase makes of its list is compared with the FAST ORDER oracle after EVERY step, tolerance 0.

Lane counts: the candidate ranking walks the candidates in rounds of one team (`for c = tl; c < n_cand; c += T`).  The flagship walk has 4 pairs
per env; random drops reach 12 and more; the stairs env has 27-30 (every robot geom overlaps the heightfield's box).  No state reachable through
the engine exceeds 32, so teams of 32 / 64 lanes run that loop once; more than one round is covered by the stairs case under GO2SIM_DYN_TEAM=16
(k_dynamics_team<16> opens every step there), which asserts n_broad > 16 on the oracle's own I_N_BROAD before anything is compared.

GO2SIM_DYN_TEAM=16 also selects the row-form mass factorisation (the arrow form needs 32 lanes: other last bits, tests/test_rigid_reference.py KNOBS),
so for those runs both libraries are put into their row form (GO2SIM_NO_ARROW=1, read when the model is parsed; HIP == fast oracle bit for bit in that
form: tests/test_parity_gpu.py::test_row_form_factorisation_bit_exact).  The reference stays the fast oracle and the tolerance stays 0."""
import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json, pack_model
from util import Handle, Pair, bench_actions, bits_equal, compare_fields, env_pair, random_poses, step_pair

FIELDS = ["F_SORT_VALUE", "I_SORT_IG", "I_N_BROAD", "I_N_CONTACTS", "I_CONTACT_GEOMS", "F_CONTACT_POS", "F_CONTACT_NORMAL", "F_CONTACT_PEN",
          "F_NORMAL_CACHE", "I_FIRST_TIME", "I_ERRNO"]
SCENE_FIELDS = FIELDS + ["F_QPOS", "F_VEL"]
SORT_FIELDS = ["F_SORT_VALUE", "I_SORT_IG", "I_N_BROAD", "I_FIRST_TIME"]


def _run_env(cpu, gpu, acts, first_step=0, min_broad=None, tag=""):
    seen = 0
    for s, _, _ in step_pair(cpu, gpu, acts, FIELDS, tag, first_step):
        nb = cpu.field("I_N_BROAD")
        if min_broad is not None:                     # the condition on the inputs, on the oracle's own count
            assert nb.min() > min_broad, f"{tag} step {s}: the oracle's n_broad {nb.min()}..{nb.max()} does not exceed {min_broad}"
        seen = max(seen, int(nb.max()))
    assert cpu.sim.check_errno() == gpu.sim.check_errno() == 0
    return seen


# knobs of the dynamics team; 16 lanes: row form on both sides (module docstring)
TEAMS = {"32": None, "16": {"GO2SIM_DYN_TEAM": "16", "GO2SIM_NO_ARROW": "1"}, "64": {"GO2SIM_DYN_TEAM": "64"}}


@pytest.mark.gpu
@pytest.mark.parametrize("team", list(TEAMS))
def test_walk_window_and_steady_gait(oracle_lib, hip_lib, blob, team):
    """The benchmark's walk configuration and action tape from the reset: the landing window (steps 0-25) and on through the steady gait (to step
    150, i.e. 50 steps past the benchmark's 100 warm-up steps), every step compared.  63 envs: the last workgroup of every team kernel is partly empty."""
    n_envs, steps = 63, 150
    cpu, gpu = env_pair(oracle_lib, hip_lib, blob, n_envs, "walk", TEAMS[team], freeze_curriculum=True)
    seen = _run_env(cpu, gpu, bench_actions(steps, n_envs, "walk"), tag=f"walk T={team}")
    assert seen >= 4, seen
    assert gpu.sim.graph_status() == (True, 0), gpu.sim.graph_status()


@pytest.mark.gpu
@pytest.mark.parametrize("team", list(TEAMS))
def test_stairs_env(oracle_lib, hip_lib, blob, team):
    """Stair heightfield: every robot geom overlaps the terrain's box, 27-30 broad-phase pairs per env from the first step -- more than the 16 lanes of
    the smallest dynamics team (asserted on the oracle's own count at every step), so k_dynamics_team<16> ranks its candidates in two rounds; teams of
    32 / 64 lanes run the ranking loop once."""
    n_envs, steps = 64, 20
    cpu, gpu = env_pair(oracle_lib, hip_lib, blob, n_envs, "stairs", TEAMS[team])
    seen = _run_env(cpu, gpu, bench_actions(steps, n_envs, "stairs"), min_broad=16, tag=f"stairs T={team}")
    assert 16 < seen <= 32, seen


@pytest.mark.gpu
def test_resets_in_the_middle_of_a_run(oracle_lib, hip_lib, blob):
    """reset_caches (a subset, then all envs) and env_reset_idx between steps, and first_time raised again for some envs in the middle of the run
    (what a scene reset does; reset_caches and env_reset_idx themselves leave first_time alone, in the oracle as in the HIP library): the next
    dynamics pass rebuilds their sort order from the geom order and hands first_time back."""
    import torch

    n_envs = 64
    cpu, gpu = env_pair(oracle_lib, hip_lib, blob, n_envs, "walk", freeze_curriculum=True)
    acts = bench_actions(50, n_envs, "walk")
    dev = gpu.dev
    assert cpu.field("I_FIRST_TIME").all()                # from the creation of the scene: step 0 takes the first_time path in every env
    _run_env(cpu, gpu, acts[:9], tag="before")
    assert not cpu.field("I_FIRST_TIME").any()
    idx = np.arange(3, n_envs, 5, dtype=np.int32)
    cpu.sim.reset_caches(idx, len(idx)); gpu.sim.reset_caches(torch.from_numpy(idx).to(dev), len(idx))
    compare_fields(cpu, gpu, FIELDS, "after reset_caches(idx)")
    _run_env(cpu, gpu, acts[9:15], first_step=9, tag="after reset_caches(idx)")
    idx = np.arange(1, n_envs, 3, dtype=np.int32)
    cpu.sim.env_reset_idx(idx, len(idx)); gpu.sim.env_reset_idx(torch.from_numpy(idx).to(dev), len(idx))
    compare_fields(cpu, gpu, FIELDS, "after env_reset_idx")
    _run_env(cpu, gpu, acts[15:25], first_step=15, tag="after env_reset_idx")
    cpu.sim.reset_caches(None, 0); gpu.sim.reset_caches(None, 0)
    _run_env(cpu, gpu, acts[25:35], first_step=25, tag="after reset_caches(all)")
    ft = np.zeros((1, n_envs), np.int32); ft[0, ::3] = 1
    cpu.set_field("I_FIRST_TIME", ft); gpu.set_field("I_FIRST_TIME", ft)
    _run_env(cpu, gpu, acts[35:36], first_step=35, tag="first_time raised")
    assert not cpu.field("I_FIRST_TIME").any()
    _run_env(cpu, gpu, acts[36:50], first_step=36, tag="after first_time")


@pytest.mark.gpu
def test_random_drops(oracle_lib, hip_lib, blob):
    """Robots dropped in random orientations: many more pairs than the flagship's four, self collisions, changing sort order."""
    B = 96
    p = Pair(oracle_lib, hip_lib, blob, B)
    p.put("F_QPOS", random_poses(B, 9))
    p.both(lambda s: (s.reset_caches(None, 0), s.forward_kinematics()))
    mx = 0
    for s in range(25):
        p.both(lambda sim: sim.scene_step(1))
        mx = max(mx, int(p.cget("I_N_BROAD").max()))
        p.compare(SCENE_FIELDS, f"step {s}")
    assert mx >= 12, mx                                  # (tests/test_overflow_paths.py clips these states at a cap of 12)
    assert p.cpu.sim.check_errno() == p.gpu.sim.check_errno() == 0


@pytest.mark.gpu
def test_forward_kinematics_leaves_the_sort_state_alone(oracle_lib, hip_lib, blob):
    """set_field(QPOS) + forward_kinematics, twice in a row, then scene_step(1) and scene_step(3): the kinematics alone do not advance the sort buffers
    (they advance once per collision pass); odd substep counts end on a dynamics pass of either kind."""
    B = 64
    p = Pair(oracle_lib, hip_lib, blob, B)
    p.put("F_QPOS", random_poses(B, 5))
    p.both(lambda s: (s.reset_caches(None, 0), s.forward_kinematics()))
    for s in range(4):
        p.both(lambda sim: sim.scene_step(2))
        p.compare(SCENE_FIELDS, f"warm-up {s}")
    for rep in range(3):
        before = {f: p.gget(f) for f in SORT_FIELDS}
        for k in range(2):
            p.put("F_QPOS", random_poses(B, 20 + 2 * rep + k))
            p.both(lambda s: s.forward_kinematics())
            for f in SORT_FIELDS:
                assert bits_equal(before[f], p.gget(f)), f"forward_kinematics changed {f}"
            p.compare(SCENE_FIELDS, f"rep {rep} FK {k}")
        p.both(lambda sim: sim.scene_step(1))
        p.compare(SCENE_FIELDS, f"rep {rep} scene_step(1)")
        assert not bits_equal(before["F_SORT_VALUE"], p.gget("F_SORT_VALUE"))
        p.both(lambda sim: sim.scene_step(3))
        p.compare(SCENE_FIELDS, f"rep {rep} scene_step(3)")
    assert p.cpu.sim.check_errno() == p.gpu.sim.check_errno() == 0


@pytest.mark.gpu
def test_anymal_shape(oracle_lib, hip_lib):
    """ANYmal-C through the same kernels (other geoms, padding spheres that take part in no pair): random position targets every step."""
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go2_sim2real_locomotion_rl_amd", "model", "anymal_c_model.json")
    m = load_model_json(path)
    B = 64

    def make(lib, gpu):
        h = Handle(lib, pack_model(m), B, gpu)
        for k in range(12):
            eff = abs(m["dofs"][6 + k]["force_range"][1])
            h.sim.set_dof_gains(6 + k, 1000.0, 10.0, -eff, eff)
        return h

    p = Pair(oracle_lib, hip_lib, None, B, make)
    mode = np.zeros((18, B), np.int32); mode[6:] = 2
    p.put("I_CTRL_MODE", mode)
    p.both(lambda s: (s.reset_caches(None, 0), s.forward_kinematics()))
    rng = np.random.default_rng(0)
    in_contact = 0
    for s in range(80):
        ctrl = np.zeros((18, B), np.float32); ctrl[6:] = rng.uniform(-0.05, 0.05, (12, B)) * (4.0 if s > 40 else 1.0)
        p.put("F_CTRL_POS", ctrl)
        p.both(lambda sim: sim.scene_step(1 + s % 2))
        p.compare(SCENE_FIELDS, f"step {s}")
        in_contact += int((p.cget("I_N_CONTACTS") > 0).sum())
    assert in_contact > 0, "the robots reached the ground: the narrow phase had pairs to work on"
    assert p.cpu.sim.check_errno() == p.gpu.sim.check_errno() == 0
