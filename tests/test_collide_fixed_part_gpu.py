"""The fixed part of k_collide_team<16> -- what a launch spends outside its MPR and GJK / EPA queries -- shortened without changing a value: a wave whose
pairs are all a sphere against a box (the walking Go2: feet and head sphere on the ground box) runs cc_detect0 and cc_rest with the class's constants
(no perturbed detections, no link orientation fetched), any other wave the generic code.  Every case steps the FAST ORDER oracle, the default handle
and a handle created under GO2SIM_COLLIDE_GENERIC=1 (every wave generic: one binary against itself) and compares after EVERY step at tolerance 0: the
oracle against the default handle, the default handle against the generic one, in FIELDS and the five env outputs.

What FIELDS stands for.  The field API (oracle and HIP library alike) has no field for the broad-phase list, for a contact's links, friction and
solver parameters, or for the valid bits of the normal cache, and the oracle keeps them in no other readable place.  As in
tests/test_collide_staging_gpu.py: I_N_BROAD with the sort buffers (F_SORT_VALUE, I_SORT_IG) is the broad phase's state, of which the list is a
function (this kernel only reads it); F_CONTACT_FORCE, F_EFC_FORCE, I_N_CONSTRAINTS, F_QPOS and F_VEL carry a contact's links, friction and solver
parameters (another link, friction or parameter gives other forces and another next state); F_NORMAL_CACHE reads through the valid bits.  The
GJK / EPA fallbacks are compared per env between the two HIP handles (pool field gjk_fallback) and in total with the oracle's counter, which is not
kept per env.  The plane ground is a geom the oracle does not have: that case compares the two HIP handles with each other.

Conditions on the inputs, computed on the oracle alone.  The EXPECTED pairs of a model (expected_pairs) are its valid pairs of a sphere with a box on a
fixed root link: the pairs of the sphere-box class a standing robot lists (the Go2 has five: the head sphere and the four feet).  A sphere pair gives
at most one contact, so an env whose contacts are all of expected pairs and as many as its n_broad lists exactly its contact pairs, in contact order
(= pair order):
  * set C, 130 envs (no multiple of 4 or 64), 40 steps from the reset: the lists go from empty through strict subsets of the expected pairs (with
    a pair on another lane than its index among the expected ones) to four feet with a contact each at the last step; some step has GJK / EPA
    fallbacks; no contact of the run is of another pair, so every wave of the run takes the sphere-box code.
  * set B, 64 envs, 60 steps.  Under set B alone no Go2 falls within 120 steps (tests/test_collide_pair_class_gpu.py), so every third env (one or two
    of every wave of four) is respawned at step 10 rolled 1.2 - 1.9 rad about x, with the roll / pitch terminations off: those robots lie on thighs
    and base next to feet; half of the envs are reset at step 40.  Some env lists a pair that is not expected (a contact of another pair, or more
    pairs than the model expects) while other envs, and the same env, list expected ones: both kinds in one round, the wave goes generic as a whole.
  * stairs: geom 0 is the heightfield, the model expects nothing (generic waves, the terrain pass); plane ground: the same (plane_contact, the
    plane-box pass); jump_dr: the friction words differ between envs and are drawn again at a reset; go2sim_set_friction between steps: the friction
    words change under a handle that has already stepped."""
import ctypes

import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json, pack_model, with_plane_ground
from util import CpuEnv, GpuEnv, bench_actions, bits_equal, compare_fields, make_actions, outputs_differing, with_knobs

GEOM_SPHERE, GEOM_BOX = 1, 5
FIELDS = ["F_SORT_VALUE", "I_SORT_IG", "I_N_BROAD", "I_N_CONTACTS", "I_CONTACT_GEOMS", "F_CONTACT_POS", "F_CONTACT_NORMAL", "F_CONTACT_PEN",
          "F_NORMAL_CACHE", "I_FIRST_TIME", "I_ERRNO", "F_CONTACT_FORCE", "F_EFC_FORCE", "I_N_CONSTRAINTS", "F_QPOS", "F_VEL"]
KNOBS = {"generic": {"GO2SIM_COLLIDE_GENERIC": "1"}}


def expected_pairs(model):
    """[(a, b)] with a < b in the order of the host's scan: valid pairs of a sphere with a box on a fixed root link"""
    g, links = model["geoms"], model["links"]
    ng = len(g)
    idx = np.asarray(model["collision_pair_idx"], np.int64).reshape(ng, ng)
    out = []
    for a in range(ng):
        for b in range(a + 1, ng):
            if idx[a, b] < 0 or {g[a]["type"], g[b]["type"]} != {GEOM_SPHERE, GEOM_BOX}:
                continue
            lb = links[g[a if g[a]["type"] == GEOM_BOX else b]["link"]]
            if lb["parent"] == -1 and lb["is_fixed"]:
                out.append((a, b))
    return out


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


def contact_pairs(env):
    """per env: the (geom a, geom b) of its contacts, a < b, in list order"""
    nc, cg = env.field("I_N_CONTACTS")[0], env.field("I_CONTACT_GEOMS")
    maxc = cg.shape[0] // 2
    return [[tuple(sorted((int(cg[c, b]), int(cg[maxc + c, b])))) for c in range(int(nc[b]))] for b in range(env.B)]


class Sides:
    """The oracle (None where it does not have the scene) next to the default handle and the knob handle(s); make(lib, gpu) builds one side."""

    def __init__(self, make, oracle_lib, hip_lib, tag):
        self.tag = tag
        self.cpu = make(oracle_lib, False) if oracle_lib is not None else None
        self.gpu = make(hip_lib, True)
        self.alt = {}
        for name, knobs in KNOBS.items():
            with with_knobs(knobs):
                self.alt[name] = make(hip_lib, True)
        self.fb_steps, self.fb_last = [], 0

    def all(self):
        return ([self.cpu] if self.cpu is not None else []) + [self.gpu] + list(self.alt.values())

    def start(self):
        """after the resets: the fallback counters are never cleared, the increments count"""
        self.fb0 = _oracle_fallbacks(self.cpu) if self.cpu is not None else 0
        self.fb_last = self.fb0
        self.fg0 = {n: _fallbacks(e) for n, e in [("default", self.gpu)] + list(self.alt.items())}

    def compare(self, s, outs=None):
        where = f"{self.tag} step {s}"
        if self.cpu is not None:
            compare_fields(self.cpu, self.gpu, FIELDS, where + ", default handle")
        got = {f: self.gpu.get(f) for f in FIELDS}
        fg = _fallbacks(self.gpu) - self.fg0["default"]
        for name, e in self.alt.items():
            bad = [f for f in FIELDS if not bits_equal(got[f], e.get(f))]
            assert not bad, f"{where}: {bad} differ between the default handle and {KNOBS[name]}"
            assert np.array_equal(fg, _fallbacks(e) - self.fg0[name]), f"{where}: gjk_fallback differs between the default handle and {KNOBS[name]}"
        if self.cpu is not None:
            fb = _oracle_fallbacks(self.cpu)
            assert int(fg.sum()) == fb - self.fb0, f"{where}: {int(fg.sum())} fallbacks, the oracle counts {fb - self.fb0}"
            if fb > self.fb_last:
                self.fb_steps.append(s)
            self.fb_last = fb
        if outs is not None:
            names = (["oracle"] if self.cpu is not None else []) + ["default"] + list(self.alt)
            ref = outs[names.index("default")]
            for n, o in zip(names, outs):
                bad = outputs_differing(o, ref)
                assert not bad, f"{where}: {bad} differ between {n} and the default handle"

    def step_env(self, s, a):
        self.compare(s, [e.step(a) for e in self.all()])

    def done(self):
        assert all(e.sim.check_errno() == 0 for e in self.all())


def _env_sides(oracle_lib, hip_lib, blob, n_envs, task, tag, seed=3, **kw):
    sd = Sides(lambda lib, gpu: (GpuEnv if gpu else CpuEnv)(lib, blob, n_envs, seed=seed, task=task, **kw), oracle_lib, hip_lib, tag)
    for e in sd.all():
        e.reset()
    sd.start()
    return sd


def _set_b(steps, n_envs):
    import torch

    from bench import make_actions as bench_make_actions
    return bench_make_actions(steps, n_envs, torch.device("cpu"), workload="walk", kind="B", seed=0).numpy()


@pytest.mark.gpu
def test_walk_set_c_from_the_reset(oracle_lib, hip_lib, blob):
    n_envs, steps = 130, 40
    exp = expected_pairs(load_model_json())
    assert 0 < len(exp) <= 8, exp
    sd = _env_sides(oracle_lib, hip_lib, blob, n_envs, "walk", "set C", freeze_curriculum=True)
    subset_other_lane, all_feet_last = [], 0
    for s, a in enumerate(bench_actions(steps, n_envs, "walk")):
        sd.step_env(s, a)
        nb, pairs = sd.cpu.field("I_N_BROAD")[0], contact_pairs(sd.cpu)
        assert all(p in exp for ps in pairs for p in ps), f"step {s}: a contact of a pair the model does not expect"
        for b in range(n_envs):
            if 0 < nb[b] < len(exp) and len(pairs[b]) == nb[b] and any(exp.index(p) != lane for lane, p in enumerate(pairs[b])):
                subset_other_lane.append((s, b))
        all_feet_last = sum(1 for b in range(n_envs) if nb[b] == 4 and len(pairs[b]) == 4)
    sd.done()
    print(f"set C: strict subsets of the expected pairs, a pair on another lane than its index, at {len(subset_other_lane)} (step, env), first {subset_other_lane[:3]}; fallbacks at steps {sd.fb_steps}; "
          f"{all_feet_last} envs on four expected pairs at the last step")
    assert subset_other_lane, "no env lists a strict subset of the expected pairs with a pair on another lane than its own"
    assert sd.fb_steps, "no GJK / EPA fallback"
    assert all_feet_last > 0, "no env lists four expected pairs at the last step"


@pytest.mark.gpu
def test_walk_set_b_with_resets(oracle_lib, hip_lib, blob):
    n_envs, steps = 64, 60
    exp = expected_pairs(load_model_json())
    no_term = lambda env_cfg, *rest: env_cfg.update(termination_if_roll_greater_than=400, termination_if_pitch_greater_than=400)   # noqa: E731
    sd = _env_sides(oracle_lib, hip_lib, blob, n_envs, "walk", "set B", freeze_curriculum=True, mutate=no_term)
    lying = np.arange(1, n_envs, 3, dtype=np.int32)                    # one or two robots of every wave of four envs
    ang = np.random.default_rng(5).uniform(1.2, 1.9, len(lying)).astype(np.float32)
    pos = np.tile(np.array([[0.0, 0.0, 0.25]], np.float32), (len(lying), 1))
    quat = np.stack([np.cos(0.5 * ang), np.sin(0.5 * ang), 0 * ang, 0 * ang], 1).astype(np.float32)
    even = np.arange(0, n_envs, 2, dtype=np.int32)
    dev_of = lambda e, x: x if not e.gpu else e.torch.from_numpy(x).to(e.dev)   # noqa: E731
    unexpected, expected_beside, same_env = [], 0, 0
    for s, a in enumerate(_set_b(steps, n_envs)):
        for e in sd.all():
            if s == 10:
                e.sim.env_respawn(dev_of(e, lying), dev_of(e, pos), dev_of(e, quat), True, len(lying))
            if s == 40:
                e.sim.env_reset_idx(dev_of(e, even), len(even))
        sd.step_env(s, a)
        nb, pairs = sd.cpu.field("I_N_BROAD")[0], contact_pairs(sd.cpu)
        here = [b for b in range(n_envs) if nb[b] > len(exp) or any(p not in exp for p in pairs[b])]
        if here:
            unexpected.append((s, here[0]))
            expected_beside += sum(1 for b in range(n_envs) if b not in here and any(p in exp for p in pairs[b]))
            same_env += sum(1 for b in here if any(p in exp for p in pairs[b]))
    sd.done()
    print(f"set B: a pair that is not expected at {len(unexpected)} steps, first {unexpected[:3]}; at those steps {expected_beside} (step, env) with expected pairs only "
          f"and {same_env} with both kinds in one list")
    assert unexpected, "every listed pair is an expected one"
    assert expected_beside > 0 and same_env > 0, "hits and misses do not meet"


@pytest.mark.gpu
def test_stairs_expect_nothing(oracle_lib, hip_lib, blob):
    n_envs, steps = 16, 20
    sd = _env_sides(oracle_lib, hip_lib, blob, n_envs, "stairs", "stairs")
    nc = 0
    for s, a in enumerate(bench_actions(steps, n_envs, "stairs")):
        sd.step_env(s, a)
        nc = max(nc, int(sd.cpu.field("I_N_CONTACTS").max()))
    sd.done()
    assert nc > 0, "no contact with the stairs"


@pytest.mark.gpu
def test_plane_ground_expects_nothing(hip_lib):
    """(the oracle has no plane geom: the HIP handles against each other)"""
    n_envs, steps = 16, 20
    model = with_plane_ground(load_model_json())
    assert not expected_pairs(model)
    pblob = pack_model(model)
    sd = _env_sides(None, hip_lib, pblob, n_envs, "walk", "plane")
    nc = 0
    for s, a in enumerate(make_actions(steps, n_envs, seed=3, kind="mixed", n_act=sd.gpu.n_act)):
        sd.step_env(s, a)
        nc = max(nc, int(sd.gpu.field("I_N_CONTACTS").max()))
    sd.done()
    assert nc > 0, "no contact with the plane"


@pytest.mark.gpu
def test_jump_dr_friction_redrawn(oracle_lib, hip_lib, blob):
    n_envs, steps = 64, 30
    sd = _env_sides(oracle_lib, hip_lib, blob, n_envs, "jump_dr", "jump_dr")
    fr0 = sd.cpu.field("F_GEOM_FRICTION").copy()
    assert np.unique(fr0[1]).size > 1, "the envs draw different frictions"
    idx = np.arange(0, n_envs, 2, dtype=np.int32)
    nc = 0
    for s, a in enumerate(make_actions(steps, n_envs, seed=5, kind="mixed", n_act=sd.cpu.n_act)):
        if s == 15:
            for e in sd.all():
                e.sim.env_reset_idx(idx if not e.gpu else e.torch.from_numpy(idx).to(e.dev))
            assert not np.array_equal(sd.cpu.field("F_GEOM_FRICTION")[:, idx], fr0[:, idx]), "the reset draws the friction again"
        sd.step_env(s, a)
        if s >= 15:
            nc = max(nc, int(sd.cpu.field("I_N_CONTACTS")[0][idx].max()))
    sd.done()
    assert nc > 0, "no contact after the friction was drawn again"


@pytest.mark.gpu
def test_set_friction_between_steps(oracle_lib, hip_lib, blob):
    n_envs, steps = 4, 24
    sd = _env_sides(oracle_lib, hip_lib, blob, n_envs, "walk", "set_friction", freeze_curriculum=True)
    nc = 0
    for s, a in enumerate(bench_actions(steps, n_envs, "walk")):
        if s >= 8 and s % 4 == 0:
            for e in sd.all():
                e.sim.set_friction(0.4 + 0.1 * (s // 4))
        sd.step_env(s, a)
        if s >= 8:
            nc = max(nc, int(sd.cpu.field("I_N_CONTACTS").max()))
    sd.done()
    assert nc > 0, "no contact after the friction was set"
