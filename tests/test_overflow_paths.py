"""Worst-case contact paths of the constraint solver and the collider (reference sizes: constraint/solver.py:43-48 `len_constraints`,
collider.py:364-372 `max_contact_pairs` / broad pairs): states uploaded through set_field (robots dropped in random orientations with random joint
angles, i.e. on their sides / backs with self collisions; on the stairs lying across the step edges) so that

  * flat ground: more constraint rows than the solver keeps in LDS (32)  -> the per-env global-scratch path of k_constraint_solve_team<32, 32>
  * stair terrain: more than 96 rows                                       -> the same for k_constraint_solve_team<64, 96>
  * a model with small contact / broad-pair caps                           -> the GO2SIM_ERR_OVERFLOW_* flags, identically on both sides

GPU == oracle bit for bit on every step, and each test asserts that the row counts / flags it is about were actually reached."""
import copy

import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.capi import C, Go2Sim
from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json, pack_model
from util import Handle, Pair, install_stairs, random_poses

FIELDS = ["F_QPOS", "F_VEL", "F_ACC", "F_CONTACT_FORCE", "F_QFRC_CONSTRAINT", "F_EFC_FORCE", "F_CONTACT_PEN", "F_CONTACT_POS", "F_CONTACT_NORMAL",
          "I_N_CONTACTS", "I_N_CONSTRAINTS", "I_SOLVER_ITERS", "I_N_BROAD", "I_ERRNO", "I_CONTACT_GEOMS"]


class _Pair(Pair):
    """the scene pair of these tests: optionally on the stairs (`info`: their terrain), states uploaded as qpos, steps counted in rows and contacts"""

    def __init__(self, oracle_lib, hip_lib, blob, B, terrain=False):
        self.info = None

        def make(lib, gpu):
            h = Handle(lib, blob, B, gpu)
            if terrain:
                _, self.info = install_stairs(h.sim)
            return h

        super().__init__(oracle_lib, hip_lib, blob, B, make)

    def upload(self, qpos):
        self.put("F_QPOS", qpos)
        self.both(lambda s: (s.reset_caches(None, 0), s.forward_kinematics()))

    def step_and_compare(self, steps, fields=FIELDS):
        mx_rows = mx_con = 0; errs = 0
        for s in range(steps):
            self.both(lambda sim: sim.scene_step(1))
            self.compare(fields, f"step {s} (rows max {mx_rows})")
            rows = self.cget("I_N_CONSTRAINTS")[0]
            mx_rows = max(mx_rows, int(rows.max())); mx_con = max(mx_con, int(self.cget("I_N_CONTACTS").max()))
            errs |= int(np.bitwise_or.reduce(self.cget("I_ERRNO")[0]))
        assert self.cpu.sim.check_errno() == self.gpu.sim.check_errno()       # (compared with each other: the cap tests mean them to be non-zero)
        return mx_rows, mx_con, errs


@pytest.mark.gpu
def test_flat_ground_more_rows_than_lds(oracle_lib, hip_lib, blob):
    p = _Pair(oracle_lib, hip_lib, blob, 96)
    p.upload(random_poses(96, 5))
    mx_rows, mx_con, errs = p.step_and_compare(25)
    assert mx_rows > 128 and mx_con > 32, (mx_rows, mx_con)        # far beyond the 32 LDS rows of the flat-ground solver
    assert errs == 0


@pytest.mark.gpu
def test_terrain_more_rows_than_lds(oracle_lib, hip_lib, blob):
    p = _Pair(oracle_lib, hip_lib, blob, 96, terrain=True)
    p.upload(random_poses(96, 5, p.info, z_range=(-0.25, 0.3)))
    mx_rows, mx_con, errs = p.step_and_compare(20)
    assert mx_rows > 400 and mx_con > 100, (mx_rows, mx_con)       # > 96 LDS rows of the terrain solver; close to the 150-contact cap
    assert errs == 0


@pytest.mark.gpu
@pytest.mark.parametrize("terrain", [False, True])
def test_contact_cap_overflow_parity(oracle_lib, hip_lib, terrain):
    """max_contact_pairs lowered in the model blob (150 -> 24): contacts beyond the cap are dropped in list order on both sides, the flag
    GO2SIM_ERR_OVERFLOW_COLLISION_PAIRS is raised identically, and the clipped contact lists and everything downstream agree bit for bit."""
    model = copy.deepcopy(load_model_json())
    model["collider"]["max_contact_pairs"] = 24
    p = _Pair(oracle_lib, hip_lib, pack_model(model), 64, terrain=terrain)
    p.upload(random_poses(64, 9, p.info, z_range=(-0.25, 0.3) if terrain else (0.06, 0.2)))
    mx_rows, mx_con, errs = p.step_and_compare(12)
    assert mx_con == 24 and errs == C["GO2SIM_ERR_OVERFLOW_COLLISION_PAIRS"], (mx_con, errs)


@pytest.mark.gpu
def test_broad_pair_cap_overflow_flag_parity(oracle_lib, hip_lib):
    """max_broad_pairs lowered (240 -> 12): GO2SIM_ERR_OVERFLOW_CANDIDATE_CONTACTS is raised for the same envs on both sides, and the broad-phase
    list is clipped to the pairs the serial sweep reaches first.  (What the serial sweep does to the contact-normal cache of the pairs it never
    reaches is an artefact of an error state -- the reference raises at its next errno poll, rigid_solver.py:1189-1213 -- and is not reproduced:
    the state is only compared for this first step.)"""
    model = copy.deepcopy(load_model_json())
    model["collider"]["max_broad_pairs"] = 12
    p = _Pair(oracle_lib, hip_lib, pack_model(model), 64)
    p.upload(random_poses(64, 9))
    p.both(lambda sim: sim.scene_step(1))
    ec, eg = p.cget("I_ERRNO"), p.gget("I_ERRNO")
    assert np.array_equal(ec, eg) and (ec & C["GO2SIM_ERR_OVERFLOW_CANDIDATE_CONTACTS"]).any()
    p.compare(("I_N_BROAD", "I_N_CONTACTS", "I_CONTACT_GEOMS", "F_CONTACT_PEN", "F_QPOS", "F_VEL"), "first step")
    assert p.cget("I_N_BROAD").max() == 12


def test_overflow_states_on_the_oracle(oracle_lib, blob):
    """CPU-side twin of the GPU tests above (no GPU needed): the uploaded states do reach the row counts the GPU tests are about."""
    sim = Go2Sim(oracle_lib, blob, 48, 0, 1)
    sim.set_field_np(C["GO2SIM_F_QPOS"], random_poses(48, 5))
    sim.reset_caches(None, 0); sim.forward_kinematics()
    sim.scene_step(1)
    rows = sim.get_field_np(C["GO2SIM_I_N_CONSTRAINTS"])[0]
    assert rows.max() > 128 and (rows > 32).sum() > 20 and sim.check_errno() == 0
    assert np.isfinite(sim.get_field_np(C["GO2SIM_F_QPOS"])).all()
