"""k_collide_team starts the narrow phase from staged operands: the per-geom constants come from a compact table in LDS (GeomK, derived on the
device with every upload of the model), the pair's normal-cache index travels in the broad-phase word (a | b << 8 | pair index << 16), the env's
records are read in two batches, and the contacts of a round are appended by ballots.  None of it changes a value: every case but the plane
ground (which the oracle does not have: test_plane_ground says what stands in) compares the HIP
library with the FAST ORDER oracle after EVERY step, tolerance 0 -- the fields of tests/test_broad_in_dynamics_gpu.py plus what a contact's friction,
solver parameters and links turn into (the field API has no contact-link field: F_CONTACT_FORCE, F_EFC_FORCE, F_QPOS and F_VEL carry them), the env
outputs, and errno 0 on both sides."""
import os

import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json, pack_model, with_plane_ground
from util import CpuEnv, Handle, Pair, bench_actions, bits_equal, draw_plane_qpos, env_pair, make_actions, random_poses, step_pair, with_knobs

FIELDS = ["F_SORT_VALUE", "I_SORT_IG", "I_N_BROAD", "I_N_CONTACTS", "I_CONTACT_GEOMS", "F_CONTACT_POS", "F_CONTACT_NORMAL", "F_CONTACT_PEN",
          "F_NORMAL_CACHE", "I_FIRST_TIME", "I_ERRNO",
          "F_CONTACT_FORCE", "F_EFC_FORCE", "I_N_CONSTRAINTS", "F_QPOS", "F_VEL"]


def _run_env(cpu, gpu, acts, tag):
    """every step compared; returns (largest n_broad of the oracle, per-env largest n_contacts of the oracle)"""
    nb_max, nc_max = 0, np.zeros(cpu.B, np.int64)
    for _ in step_pair(cpu, gpu, acts, FIELDS, tag):
        nb_max = max(nb_max, int(cpu.field("I_N_BROAD").max()))
        nc_max = np.maximum(nc_max, cpu.field("I_N_CONTACTS")[0])
    assert cpu.sim.check_errno() == gpu.sim.check_errno() == 0
    return nb_max, nc_max


@pytest.mark.gpu
@pytest.mark.parametrize("team", ["16", "32"])
def test_walk_from_the_reset(oracle_lib, hip_lib, blob, team):
    """The benchmark's walk and action tape, steps 0-40 from the reset: the landing steps with their GJK / EPA fallbacks and the first steady steps.
    63 envs: the last workgroup is partly empty (its idle lanes still take part in the copy of the geom table)."""
    n_envs, steps = 63, 41
    cpu, gpu = env_pair(oracle_lib, hip_lib, blob, n_envs, "walk", {"GO2SIM_COLLIDE_TEAM": team}, freeze_curriculum=True)
    acts = bench_actions(steps, n_envs, "walk")
    # the condition on the inputs, on the oracle alone, before anything is compared: every env touches the ground at some step
    probe = CpuEnv(oracle_lib, blob, n_envs, seed=3, task="walk", freeze_curriculum=True)
    probe.reset()
    touched = np.zeros(n_envs, bool)
    for a in acts:
        probe.step(a)
        touched |= probe.field("I_N_CONTACTS")[0] > 0
    assert touched.all(), "some env never has a contact"
    _run_env(cpu, gpu, acts, f"walk T={team}")
    assert gpu.sim.graph_status() == (True, 0), gpu.sim.graph_status()


def _drop(p, seed, steps):
    p.put("F_QPOS", random_poses(p.B, seed))
    p.both(lambda s: (s.reset_caches(None, 0), s.forward_kinematics()))
    nb, nc = 0, 0
    for s in range(steps):
        p.both(lambda sim: sim.scene_step(1))
        nb = max(nb, int(p.cget("I_N_BROAD").max())); nc = max(nc, int(p.cget("I_N_CONTACTS").max()))
        p.compare(FIELDS, f"step {s}")
    assert p.cpu.sim.check_errno() == p.gpu.sim.check_errno() == 0
    return nb, nc


@pytest.mark.gpu
def test_random_drops(oracle_lib, hip_lib, blob):
    """Robots dropped in random orientations: cylinders and boxes, multi-contact perturbed detections, self collisions.  Some env lists more than 16
    pairs (asserted on the oracle): more than one round of pairs per team of 16 -- the append over several rounds, and pair words beyond the first
    round."""
    p = Pair(oracle_lib, hip_lib, blob, 64)
    nb, nc = _drop(p, 9, 15)
    assert nb > 16, nb
    assert nc > 5, nc


PLANE_FIELDS = ["I_N_BROAD", "I_N_CONTACTS", "I_CONTACT_GEOMS", "F_CONTACT_POS", "F_CONTACT_NORMAL", "F_CONTACT_PEN", "F_NORMAL_CACHE", "I_ERRNO",
                "F_CONTACT_FORCE", "F_EFC_FORCE", "F_QPOS", "F_VEL"]


@pytest.mark.gpu
def test_plane_ground(hip_lib):
    """gs.morphs.Plane as the ground (model_blob.with_plane_ground): plane_contact and the plane-box pass on table values.  The CPU oracle has no
    plane geom (oracle/go2sim_cpu.cpp knows sphere, cylinder, box and heightfield), so the reference of this case is the one the plane was built
    against: tests/plane_ref.py (float64), contact lists of one substep on poses read back from the library, at the bound of
    tests/test_plane_gpu.py (1e-5 in position, unit normal and penetration; poses with a keep / drop decision within 1e-4 of its threshold are left
    out, float32 and float64 may decide differently there).  Tolerance 0 holds where a bit-exact counterpart exists: 20 scene steps of dropped
    robots give the same bits with 16, 32 and 64 lanes per env after every step (the team sizes split the pairs into rounds differently: 1, 2 or
    4 appends per 64 pairs, other pair-word loads)."""
    from plane_ref import PlaneRef

    base = load_model_json()
    model = with_plane_ground(base)
    blob, B = pack_model(model), 64
    ref = PlaneRef(model)
    robot_geoms = [i for i in range(1, len(model["geoms"])) if model["collision_pair_idx"][i] >= 0]
    s = Handle(hip_lib, blob, B, True, seed=5)
    worst, accepted = 0.0, 0
    # about one drawn pose in ten has contacts and keeps every decision 1e-4 from its threshold (tests/test_plane_gpu.py: 279 of 2048 on this plane), so
    # rounds of 64 are drawn until 30 poses have been compared; twelve rounds would give about 80
    for rnd in range(12):
        if accepted >= 30:
            break
        s.put("F_QPOS", draw_plane_qpos(base, np.random.default_rng(rnd), B))
        s.put("F_VEL", np.zeros((18, B), np.float32))
        s.sim.reset_caches(None, 0); s.sim.forward_kinematics()
        lp, lq = s.get("F_LINK_POS").reshape(-1, 3, B), s.get("F_LINK_QUAT").reshape(-1, 4, B)
        s.sim.substep()
        nc, cg = s.get("I_N_CONTACTS")[0], s.get("I_CONTACT_GEOMS")
        cpos, cnor, cpen = s.get("F_CONTACT_POS").reshape(-1, 3, B), s.get("F_CONTACT_NORMAL").reshape(-1, 3, B), s.get("F_CONTACT_PEN")
        maxc = cpen.shape[0]
        for b in range(B):
            want = ref.contacts(lp[:, :, b].astype(np.float64), lq[:, :, b].astype(np.float64), robot_geoms)
            if ref.margin < 1e-4 or not want:
                continue
            got = [c for c in range(nc[b]) if cg[c, b] == 0]
            assert nc[b] == len(want) + (nc[b] - len(got)), (rnd, b)
            assert [(int(cg[c, b]), int(cg[maxc + c, b])) for c in got] == [(a, g) for a, g, *_ in want], (rnd, b)
            for c, (_, _, n, p, d) in zip(got, want):
                worst = max(worst, np.abs(cpos[c, :, b] - p).max(), np.abs(cnor[c, :, b] - n).max(), abs(cpen[c, b] - d))
            accepted += 1
    print(f"plane contact lists: {accepted} poses against plane_ref, largest deviation {worst:.2e}")
    assert accepted >= 30, accepted
    assert worst <= 1e-5, worst
    assert s.sim.check_errno() == 0
    scenes = []
    for team in ("16", "32", "64"):
        with with_knobs({"GO2SIM_COLLIDE_TEAM": team}):
            scenes.append(Handle(hip_lib, blob, B, True))
    for sc in scenes:
        sc.put("F_QPOS", random_poses(B, 11))
        sc.sim.reset_caches(None, 0); sc.sim.forward_kinematics()
    touched = 0
    for step in range(20):
        for sc in scenes:
            sc.sim.scene_step(1)
        first = {f: scenes[0].get(f) for f in PLANE_FIELDS}
        touched = max(touched, int(first["I_N_CONTACTS"].max()))
        for sc, team in zip(scenes[1:], ("32", "64")):
            bad = [f for f in PLANE_FIELDS if not bits_equal(first[f], sc.get(f))]
            assert not bad, f"step {step}: {bad} differ between 16 and {team} lanes per env"
    assert touched > 0, "the robots lie on the plane"
    assert all(sc.sim.check_errno() == 0 for sc in scenes)


@pytest.mark.gpu
def test_stairs(oracle_lib, hip_lib, blob):
    """The stair heightfield is installed after the handle exists (set_terrain rewrites geom 0): the geom table has to be rebuilt with the model.
    That geom 0 really is the terrain shows in the oracle's pair count: every robot geom overlaps the heightfield's box, more than 16 pairs."""
    n_envs, steps = 64, 10
    cpu, gpu = env_pair(oracle_lib, hip_lib, blob, n_envs, "stairs")
    probe = CpuEnv(oracle_lib, blob, n_envs, seed=3, task="stairs")
    probe.reset()
    acts = bench_actions(steps, n_envs, "stairs")
    probe.step(acts[0])
    assert int(probe.field("I_N_BROAD").min()) > 16, probe.field("I_N_BROAD").min()
    nb, _ = _run_env(cpu, gpu, acts, "stairs")
    assert nb > 16, nb


@pytest.mark.gpu
def test_jump_with_per_env_friction(oracle_lib, hip_lib, blob):
    """jump_dr: per-env friction (the randomisation lands in geom_friction, asserted on the oracle) -- the friction words of a pair's second batch."""
    n_envs, steps = 64, 30
    cpu, gpu = env_pair(oracle_lib, hip_lib, blob, n_envs, "jump_dr")
    fr = cpu.field("F_GEOM_FRICTION")
    assert np.unique(fr[1]).size > 1, "the envs draw different frictions"
    _, nc = _run_env(cpu, gpu, make_actions(steps, n_envs, seed=5, kind="mixed", n_act=cpu.n_act), "jump_dr")
    assert (nc > 0).any()


@pytest.mark.parametrize("model", ["go2_model.json", "anymal_c_model.json"])
def test_pair_word_fits(model):
    """a | b << 8 | pair index << 16: geoms below 2^8 and pair indices below 2^16 for every valid pair, and pair_list[pair_idx[a][b]] = (a, b) -- the
    index the broad phase carries IS the narrow phase's m.pair_idx[a][b]."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go2_sim2real_locomotion_rl_amd", "model", model)
    m = load_model_json(path)
    ng = len(m["geoms"])
    idx = np.asarray(m["collision_pair_idx"], np.int64).reshape(ng, ng)
    assert ng <= 1 << 8
    pair_list = {}
    for a in range(ng):
        for b in range(a + 1, ng):
            if idx[a, b] >= 0:
                assert idx[a, b] not in pair_list
                pair_list[int(idx[a, b])] = a | (b << 8)
    assert pair_list, "the model has pairs"
    assert sorted(pair_list) == list(range(len(pair_list))), "pair indices are 0 ... n_pairs - 1"
    for p, w in pair_list.items():
        assert p < 1 << 16 and (w >> 8) < 1 << 8 and (w & 0xff) < 1 << 8
        word = w | (p << 16)
        assert (word & 0xff, (word >> 8) & 0xff, word >> 16) == (w & 0xff, w >> 8, p)
        assert word < 1 << 32
