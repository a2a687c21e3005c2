"""k_collide_team compiles its narrow-phase queries per pair class: a wave whose pairs are all a sphere against a box (the walking robot: feet on the
ground box) runs the PC_SPHERE_BOX instantiation of MPR and of the cooperative GJK / EPA fallback, any other wave the generic one.  Both are the
same expressions in the same order, so nothing may change: every comparison here is at tolerance 0.

Scene level: the walk, 130 envs (not a multiple of four: the last wave is partial), 40 steps from the reset under action set C (the benchmark's gait)
and under action set B (0.5 N(0, 1), seed 0 of the benchmark's tape); after EVERY step the default handle against the FAST ORDER oracle and against a handle created under
GO2SIM_COLLIDE_GENERIC=1 (every wave generic: one binary compared with itself).  The field API has no field for a contact's links, friction and
solver parameters nor for the valid bits of the normal cache: as in tests/test_collide_staging_gpu.py, F_CONTACT_FORCE, F_EFC_FORCE, F_QPOS and F_VEL
carry the former (a contact with another link, friction or solver parameter gives other forces and another next state) and F_NORMAL_CACHE reads
through the valid bits.  The per-env count of GJK / EPA fallbacks (pool field gjk_fallback) is compared per env between the two handles and in
total with the oracle's counter.

Conditions on the inputs, asserted on the oracle alone:
  * set C: some step has envs whose MPR answer was replaced by GJK / EPA (the landing; measured: steps 4-10 and 14-30, up to 187 queries a step);
  * the MIXED wave -- a group of four consecutive envs 4 k ... 4 k + 3 (one wave of k_collide_team<16>) whose last collision pass left a sphere-box
    contact in one env and a contact of another convex class in another, none of the four listing more than 16 pairs (one round of pairs): such a
    wave has to take the generic instantiation as a whole.  Under set B the Go2 does not fall within 120 steps at 130 envs: on the oracle, seeds
    0 ... 3 of the benchmark's set-B tape give no such group at any of the 120 steps (every contact is a foot's; I_N_BROAD stays at or below 5).
    The mixed wave is therefore covered with the ANYmal-C model (test_mixed_waves_anymal_c): every second robot starts rolled onto its side, so every
    wave holds standing robots (feet: spheres) next to lying ones (boxes and cylinders on the ground); measured: 20 such groups at step 20, 33 from
    step 29 on, with GJK / EPA fallbacks on the way.

Query level: go2sim_debug_narrowphase which = 7 / 8 (the class instantiations of MPR / of the quad-cooperative GJK + EPA) against which = 0 / 3
(generic) on the sphere-box poses of tests/convex_cases.py -- robot pairs (separated, grazing within the MPR tolerance, shallow, deep, the
sphere's centre inside the box) and feet on the ground slab -- in both operand orders, bit for bit in is_col, penetration, normal and position.  (The poses are the default draw of convex_cases.pair_cases /
slab_cases, computed once per process and shared with tests/test_convex_gpu.py.)"""
import ctypes

import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json
from util import CpuEnv, GpuEnv, bench_actions, bits_equal, compare_fields, make_query, outputs_differing, with_knobs

GEOM_SPHERE, GEOM_BOX = 1, 5
N_ENVS, STEPS = 130, 40
FIELDS = ["I_N_BROAD", "I_N_CONTACTS", "I_CONTACT_GEOMS", "F_CONTACT_POS", "F_CONTACT_NORMAL", "F_CONTACT_PEN", "F_NORMAL_CACHE", "I_FIRST_TIME",
          "I_ERRNO", "F_CONTACT_FORCE", "F_EFC_FORCE", "I_N_CONSTRAINTS", "F_QPOS", "F_VEL"]


def _actions(kind):
    if kind == "C":
        return bench_actions(STEPS, N_ENVS, "walk")
    import torch

    from bench import make_actions
    return make_actions(STEPS, N_ENVS, torch.device("cpu"), workload="walk", kind="B", seed=0).numpy()


def _classes_of_last_pass(env, types):
    """per env: (has a sphere-box contact, has a convex contact of another class) in the contact list the last collision pass left"""
    nc, cg = env.field("I_N_CONTACTS")[0], env.field("I_CONTACT_GEOMS")
    maxc = cg.shape[0] // 2
    sb, other = np.zeros(env.B, bool), np.zeros(env.B, bool)
    for b in range(env.B):
        for c in range(int(nc[b])):
            t = {int(types[cg[c, b]]), int(types[cg[maxc + c, b]])}
            if t == {GEOM_SPHERE, GEOM_BOX}:
                sb[b] = True
            else:
                other[b] = True
    return sb, other


def mixed_wave_groups(env, types):
    """groups of four consecutive envs (one wave at 16 lanes per env) whose last pass held a sphere-box pair and a pair of another class in ONE round"""
    sb, other = _classes_of_last_pass(env, types)
    one_round = env.field("I_N_BROAD")[0] <= 16
    return [k for k in range(0, env.B, 4) if sb[k:k + 4].any() and other[k:k + 4].any() and one_round[k:k + 4].all()]


def _fallbacks(gpu):
    """the pool field gjk_fallback (per env, counted up by every query that GJK / EPA answered) of a HIP handle"""
    import torch

    ptr, k, is_int = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
    assert gpu.sim.L.lib.go2sim_debug_field(gpu.sim.h, b"gjk_fallback", ctypes.byref(ptr), ctypes.byref(k), ctypes.byref(is_int)) == 0
    assert (k.value, is_int.value) == (1, 1)
    torch.cuda.synchronize()
    t = torch.zeros(gpu.B, dtype=torch.int32, device="cuda:0")
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ptr, ctypes.c_size_t(4 * gpu.B), ctypes.c_int(3)) == 0      # device to device
    return t.cpu().numpy()


def _oracle_fallbacks(cpu):
    n = ctypes.c_longlong()
    assert cpu.sim.L.lib.go2sim_cpu_gjk_fallback_count(cpu.sim.h, ctypes.byref(n)) == 0
    return int(n.value)


class _Checker:
    """After every step: the oracle against the default handle, the default handle against the GO2SIM_COLLIDE_GENERIC=1 one, the fallback counts
    (increments since the first call: the counters are never cleared), and the bookkeeping of the conditions on the oracle."""

    def __init__(self, cpu, gpu, gen, types, tag):
        self.cpu, self.gpu, self.gen, self.types, self.tag = cpu, gpu, gen, types, tag
        self.fb0, self.fg0, self.fn0 = _oracle_fallbacks(cpu), _fallbacks(gpu), _fallbacks(gen)
        self.fb_last, self.fb_steps, self.mixed_steps = self.fb0, [], []

    def step(self, s):
        fb = _oracle_fallbacks(self.cpu)
        if fb > self.fb_last:
            self.fb_steps.append(s)
        self.fb_last = fb
        if mixed_wave_groups(self.cpu, self.types):
            self.mixed_steps.append(s)
        compare_fields(self.cpu, self.gpu, FIELDS, f"{self.tag} step {s}, default handle")
        bad = [f for f in FIELDS if not bits_equal(self.gpu.get(f), self.gen.get(f))]
        assert not bad, f"{self.tag} step {s}: {bad} differ between the default handle and GO2SIM_COLLIDE_GENERIC=1"
        fg, fn = _fallbacks(self.gpu) - self.fg0, _fallbacks(self.gen) - self.fn0
        assert np.array_equal(fg, fn), f"{self.tag} step {s}: gjk_fallback differs between the two handles"
        assert int(fg.sum()) == fb - self.fb0, f"{self.tag} step {s}: {int(fg.sum())} fallbacks, the oracle counts {fb - self.fb0}"

    def done(self):
        print(f"{self.tag}: GJK / EPA fallbacks at steps {self.fb_steps}; mixed waves at steps {self.mixed_steps}")
        assert self.cpu.sim.check_errno() == self.gpu.sim.check_errno() == self.gen.sim.check_errno() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["C", "B"])
def test_walk_both_paths_against_the_oracle(oracle_lib, hip_lib, blob, kind):
    types = np.array([g["type"] for g in load_model_json()["geoms"]])
    acts = _actions(kind)
    cpu = CpuEnv(oracle_lib, blob, N_ENVS, seed=3, task="walk", freeze_curriculum=True)
    gpu = GpuEnv(hip_lib, blob, N_ENVS, seed=3, task="walk", freeze_curriculum=True)
    with with_knobs({"GO2SIM_COLLIDE_GENERIC": "1"}):
        gen = GpuEnv(hip_lib, blob, N_ENVS, seed=3, task="walk", freeze_curriculum=True)
    for e in (cpu, gpu, gen):
        e.reset()
    check = _Checker(cpu, gpu, gen, types, f"set {kind}")
    for s, a in enumerate(acts):
        oc, og, on = cpu.step(a), gpu.step(a), gen.step(a)
        check.step(s)
        bad = outputs_differing(oc, og)
        assert not bad, f"set {kind} step {s}: {bad} differ from the fast oracle"
        bad = outputs_differing(og, on)
        assert not bad, f"set {kind} step {s}: {bad} differ between the default handle and GO2SIM_COLLIDE_GENERIC=1"
    check.done()
    assert check.fb_steps, f"no step of the set-{kind} run has a GJK / EPA fallback"


@pytest.mark.gpu
def test_mixed_waves_anymal_c(oracle_lib, hip_lib):
    """ANYmal-C (tests/test_model.py: the `anymal` scene), 130 envs, 40 scene steps: the even envs stand, the odd ones start rolled 1.2 - 1.9 rad
    about x at z = 0.45 and come to lie on their boxes and cylinders."""
    from test_model import _anymal_sim

    cpu, m = _anymal_sim(oracle_lib, N_ENVS)
    gpu, _ = _anymal_sim(hip_lib, N_ENVS, True)
    with with_knobs({"GO2SIM_COLLIDE_GENERIC": "1"}):
        gen, _ = _anymal_sim(hip_lib, N_ENVS, True)
    types = np.array([g["type"] for g in m["geoms"]])
    q = np.tile(np.asarray(m["qpos0"], np.float32)[:, None], (1, N_ENVS))
    odd = np.arange(N_ENVS) % 2 == 1
    ang = np.random.default_rng(5).uniform(1.2, 1.9, N_ENVS)
    q[2, odd] = 0.45
    q[3, odd] = np.cos(0.5 * ang[odd]); q[4, odd] = np.sin(0.5 * ang[odd]); q[5:7, odd] = 0.0
    mode = np.zeros((18, N_ENVS), np.int32); mode[6:] = 2
    for h in (cpu, gpu, gen):
        h.put("F_QPOS", q); h.put("F_CTRL_POS", np.zeros((18, N_ENVS), np.float32)); h.put("I_CTRL_MODE", mode)
        h.sim.reset_caches(); h.sim.forward_kinematics()
    check = _Checker(cpu, gpu, gen, types, "anymal_c")
    for s in range(STEPS):
        for h in (cpu, gpu, gen):
            h.sim.scene_step(1)
        check.step(s)
    check.done()
    assert check.mixed_steps, "no wave holds a sphere-box pair next to a pair of another class"
    assert check.fb_steps, "no GJK / EPA fallback"


def _sphere_box_poses():
    """(tag, ia, ib, pa, qa, pb, qb) from tests/convex_cases.py: the sphere-box class of the robot's own pairs (every depth population and the
    sphere's centre inside the box) and feet / head sphere on the ground slab."""
    from convex_cases import pair_cases, slab_cases

    pc = [c for c in pair_cases() if c["cls"] == "sphere-box"]
    inside = [c for c in pc if c["special"] == "inside"][:6]
    sep = [c for c in pc if c["special"] is None and c["w_min"] < -4e-4][:6]
    graze = [c for c in pc if c["special"] is None and abs(c["w_min"]) <= 2.5e-4][:8]
    shallow = [c for c in pc if c["special"] is None and 2.5e-4 < c["w_min"] < 3e-3][:8]
    deep = [c for c in pc if c["special"] is None and c["w_min"] >= 3e-3][:8]
    slab = [c for c in slab_cases() if c["cls"] == "slab-sphere"][:12]
    out = []
    for tag, cs in (("inside", inside), ("separated", sep), ("grazing", graze), ("shallow", shallow), ("deep", deep), ("slab", slab)):
        assert len(cs) >= 6, (tag, len(cs))
        out += [(tag, c["ia"], c["ib"], c["pa"], c["qa"], c["pb"], c["qb"]) for c in cs]
    return out


@pytest.mark.gpu
def test_single_queries_equal_the_generic_answer(hip_lib, blob):
    types = [g["type"] for g in load_model_json()["geoms"]]
    q = make_query(hip_lib, blob, "go2sim_")
    fn = hip_lib.lib.go2sim_debug_narrowphase

    def run(which, a, b, pa, qa, pb, qb):
        out = np.zeros(8, np.float32)
        arrs = [np.ascontiguousarray(x, np.float32) for x in (pa, qa, pb, qb)]
        rc = fn(q.sim.h, which, a, b, *[x.ctypes.data_as(ctypes.c_void_p) for x in arrs], out.ctypes.data_as(ctypes.c_void_p))
        return rc, out

    n, n_col = 0, {0: 0, 3: 0}
    for tag, ia, ib, pa, qa, pb, qb in _sphere_box_poses():
        assert {types[ia], types[ib]} == {GEOM_SPHERE, GEOM_BOX}
        for order in ((ia, ib, pa, qa, pb, qb), (ib, ia, pb, qb, pa, qa)):                 # both operand orders
            for generic, special in ((0, 7), (3, 8)):
                (rc0, want), (rc1, got) = run(generic, *order), run(special, *order)
                assert rc0 == rc1 == 0
                assert bits_equal(want, got), (tag, order[0], order[1], generic, special, want, got)
                n_col[generic] += int(want[0] != 0.0)
                n += 1
    print(f"{n} query pairs; in contact: MPR {n_col[0]}, GJK / EPA {n_col[3]}")
    assert n_col[0] > 40 and n_col[3] > 40, n_col
    # the class instantiations refuse a pair that is no sphere against a box
    box = [i for i, t in enumerate(types) if t == GEOM_BOX]
    rc, _ = run(7, box[0], box[1], [0, 0, 0], [1, 0, 0, 0], [0, 0, 0], [1, 0, 0, 0])
    assert rc != 0
    assert q.sim.check_errno() == 0
