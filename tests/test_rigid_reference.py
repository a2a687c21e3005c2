"""The articulated dynamics against an independent float64 reference (tests/rigid_ref.py) at general states.

The HIP kernels are pinned bit for bit to the FAST ORDER oracle, and both translate the same spatial-algebra code; these tests pin that shared
algorithm to physics.  Each batch draws every state from its own seed: base quaternions from the whole sphere (w < 0, near 180 degrees, one
non-unit stored quaternion), joint angles across and slightly outside the limits, realistic and large velocities (base |w| up to about 20 rad/s)
and mass / COM shifts at and beyond the configured DR ranges.  Compared: (a) kinematics and COM-frame velocities, (b) the mass matrix, (c) the
smooth force in force mode, in position mode with saturating PD and with an external wrench, (d) the smooth acceleration (arrow and row form),
(e) the integrator, (f) the constraint phase with contacts (flat ground, stairs, and a batch of sub-millimetre penetrations and limit violations that
reaches both polynomial branches of the impedance curve) and joint limits: the constraint force transpose and the KKT identity, the constraint LAW
(every row's force is D max(0, -(J a - aref)) with aref, impedance, regulariser, friction / solver-parameter mixing and inverse weights rebuilt in
float64 from the reference project's formulas) and the OPTIMUM (the acceleration is the minimiser of the convex constraint problem, found by an
independent float64 Newton solve), cold and warm-started.

The reference is first pinned by closed forms of its own (kinetic energy, a rigidly spinning robot, the double pendulum's Lagrangian, momentum
and energy conservation along an accurate integration, the impedance curve at its knots, a unit mass on one constraint row).

`-m gpu`: the same cases on the HIP library, bit-equal to the FAST ORDER oracle at default settings, and under every launch-shape knob
(GO2SIM_{DYN,FK,COLLIDE,SOLVER}_TEAM, GO2SIM_TERRAIN_SOLVER_TEAM, GO2SIM_NO_LPT, GO2SIM_NO_FUSE, GO2SIM_NO_FUSE_SOLVE, GO2SIM_PAR_PRE).
"""
import os

import numpy as np
import pytest

from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json, pack_model
from rigid_ref import (BRANCH_HIGH, BRANCH_LOW, BRANCH_SAT, RigidRef, constraint_cost, constraint_force, imp_aref, impedance, mat_to_quat,
                       solve_constraints)
from util import GpuEnv, Handle, bits_equal, install_stairs, make_actions, outputs_differing, with_knobs

MODEL_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go2_sim2real_locomotion_rl_amd", "model")
G = 9.81


def _model(name):
    return load_model_json(os.path.join(MODEL_DIR, name + "_model.json"))


# ---------------------------------------------------------------------------------------------------- the reference's own closed forms
def _random_state(ref, rng, big=False):
    q = ref.qpos0.copy()
    q[0:3] = rng.uniform(-1, 1, 3)
    q[3:7] = rng.standard_normal(4)
    q[7:] = rng.uniform(-1.5, 1.5, ref.nq - 7)
    v = rng.standard_normal(ref.nd) * (6.0 if big else 1.0)
    return q, v


@pytest.mark.parametrize("name", ["go2", "anymal_c"])
def test_ref_kinetic_energy_and_jacobian_second_opinion(name):
    """v^T M v = 2 T with T summed from the propagated link velocities, and J v equals a central difference of the FK along qdot."""
    ref = RigidRef(_model(name))
    rng = np.random.default_rng(1)
    for _ in range(4):
        q, v = _random_state(ref, rng, big=True)
        k = ref.fk(q, v)
        M = ref.mass_matrix(k, extras=False)
        T = ref.kinetic_energy(k)
        assert abs(v @ M @ v - 2 * T) <= 1e-10 * T
        h = 1e-6
        kp, km = ref.fk(q + h * ref.qdot(q, v)), ref.fk(q - h * ref.qdot(q, v))
        for l in ref.moving:
            x_dot = (kp["c"][l] - km["c"][l]) / (2 * h)
            Jv, Jw = ref.jac(k, l, k["c"][l])
            assert np.allclose(Jv @ v, x_dot, atol=1e-6 * (1 + np.abs(x_dot).max()))
            assert np.allclose(ref.point_vel(k, l, k["c"][l]), Jv @ v, atol=1e-10)
            assert np.allclose(k["w"][l], Jw @ v, atol=1e-10)


@pytest.mark.parametrize("name", ["go2", "anymal_c"])
def test_ref_rigidly_spinning_robot(name):
    """Joints at rest, base moving with world velocity v0 and angular velocity w: the linear rows of c are m (-g) + m w x (w x r) (r from the base
    origin to the robot COM) and the angular rows, in body axes, R^T (w x I_o w - m r x g) with I_o the composite inertia about the base origin."""
    ref = RigidRef(_model(name))
    rng = np.random.default_rng(2)
    for _ in range(4):
        q, _ = _random_state(ref, rng)
        v = np.zeros(ref.nd)
        v[0:3] = rng.standard_normal(3)
        v[3:6] = rng.standard_normal(3) * 8.0
        k = ref.fk(q, v)
        c = ref.bias(k)
        R, o = k["R"][1], k["p"][1]
        w = R @ v[3:6]
        mv = ref.moving
        mt = k["mass"][mv].sum()
        r = k["com"] - o
        Io = sum(k["I"][l] + k["mass"][l] * ((k["c"][l] - o) @ (k["c"][l] - o) * np.eye(3) - np.outer(k["c"][l] - o, k["c"][l] - o)) for l in mv)
        lin = -mt * ref.gravity + mt * np.cross(w, np.cross(w, r))
        ang = R.T @ (np.cross(w, Io @ w) - mt * np.cross(r, ref.gravity))
        scale = mt * (G + np.linalg.norm(w) ** 2)
        assert np.abs(c[0:3] - lin).max() <= 1e-12 * scale
        assert np.abs(c[3:6] - ang).max() <= 1e-12 * scale


def test_ref_double_pendulum_lagrangian():
    """-M^-1 c of the double pendulum model equals the Lagrangian equations of two point masses on unit rods (tests/test_analytic_shapes.py)."""
    from test_analytic_shapes import double_pendulum_acc

    ref = RigidRef(_model("double_pendulum"))
    rng = np.random.default_rng(3)
    for _ in range(8):
        q, v = rng.uniform(-np.pi, np.pi, 2), rng.standard_normal(2) * 3
        k = ref.fk(q, v)
        acc = -np.linalg.solve(ref.mass_matrix(k, extras=False), ref.bias(k))
        # (inertia 1e-12 of the model's point masses: relative error ~1e-12)
        assert np.allclose(acc, double_pendulum_acc(q, v), rtol=1e-9, atol=1e-9)


def _rk4_flow(ref, q, v, h, gravity_on):
    g = None if gravity_on else np.zeros(3)

    def f(x):
        qq, vv = x[:ref.nq], x[ref.nq:]
        k = ref.fk(qq, vv)
        a = -np.linalg.solve(ref.mass_matrix(k, extras=False), ref.bias(k, gravity=g))
        return np.concatenate([ref.qdot(qq, vv), a])

    x = np.concatenate([q, v])
    k1 = f(x); k2 = f(x + 0.5 * h * k1); k3 = f(x + 0.5 * h * k2); k4 = f(x + h * k3)
    x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x[:ref.nq], x[ref.nq:]


@pytest.mark.parametrize("name", ["go2", "anymal_c"])
def test_ref_free_floating_conservation(name):
    """Free flight (M a = -c, no actuators): with gravity off the linear and angular momentum do not change; with gravity on the energy does not.
    Checked along an RK4 flow of the reference's own M and c (step 1e-3 s: RK4 error ~1e-12 of the scales)."""
    ref = RigidRef(_model(name))
    rng = np.random.default_rng(4)
    for _ in range(2):
        q, v = _random_state(ref, rng, big=True)
        q[3:7] /= np.linalg.norm(q[3:7])
        k0 = ref.fk(q, v)
        P0, L0 = ref.momentum(k0)
        E0 = ref.kinetic_energy(k0)
        q1, v1 = q, v
        for _ in range(5):
            q1, v1 = _rk4_flow(ref, q1, v1, 1e-3, gravity_on=False)
        P1, L1 = ref.momentum(ref.fk(q1, v1))
        pscale = np.sqrt(2 * E0 * k0["mass"][ref.moving].sum())
        assert np.abs(P1 - P0).max() <= 1e-8 * pscale and np.abs(L1 - L0).max() <= 1e-8 * pscale * (1 + np.abs(q1[:3]).max())
        q2, v2 = q, v
        for _ in range(5):
            q2, v2 = _rk4_flow(ref, q2, v2, 1e-3, gravity_on=True)
        k2 = ref.fk(q2, v2)
        E = lambda kk: ref.kinetic_energy(kk) + ref.potential_energy(kk)   # noqa: E731
        assert abs(E(k2) - E(k0)) <= 1e-8 * E0


SOLS = [(0.02, 1.0, 0.9, 0.95, 0.001, 0.5, 2.0), (0.05, 0.7, 0.2, 0.8, 0.01, 0.3, 3.0), (0.01, 1.3, 0.5, 0.99, 0.002, 0.8, 1.0)]


@pytest.mark.parametrize("sol", SOLS)
def test_ref_impedance_closed_forms(sol):
    """The impedance is dmin at 0, dmax at and beyond the width, dmin + mid (dmax - dmin) at mid (the unit curve passes through (mid, mid)); it
    is even in the position, continuous across mid and across the width, and monotone; each stretch reports its branch."""
    _, _, dmin, dmax, width, mid, power = sol
    assert impedance(sol, 0.0) == (dmin, BRANCH_LOW)
    for x in (1.0, 1.0 + 1e-9, 3.0, 1e3):
        imp, br = impedance(sol, -x * width)
        assert imp == pytest.approx(dmax, rel=1e-14) and br == (BRANCH_HIGH if x == 1.0 else BRANCH_SAT)
    imp_mid, br = impedance(sol, mid * width)
    assert imp_mid == pytest.approx(dmin + mid * (dmax - dmin), rel=1e-14) and br == BRANCH_HIGH
    h = 1e-9
    below, above = impedance(sol, (mid - h) * width), impedance(sol, (mid + h) * width)
    assert below[1] == BRANCH_LOW and above[1] == BRANCH_HIGH
    assert abs(below[0] - imp_mid) <= 10 * h and abs(above[0] - imp_mid) <= 10 * h          # (slope of the unit curve at mid: power <= 3)
    xs = np.linspace(0.0, 1.5, 301)
    imps = np.array([impedance(sol, x * width)[0] for x in xs])
    assert (np.diff(imps) >= 0).all() and imps[0] == dmin and imps[-1] == dmax
    assert (np.diff(imps[xs < 1.0]) > 0).all(), "strictly increasing up to the width"
    assert all(impedance(sol, x * width) == impedance(sol, -x * width) for x in xs)
    if power == 2.0:                                                 # the two parabolas written out
        assert impedance(sol, 0.25 * mid * width)[0] == pytest.approx(dmin + (dmax - dmin) * 0.0625 * mid, rel=1e-14)
        x = 0.5 * (1 + mid)
        assert impedance(sol, x * width)[0] == pytest.approx(dmin + (dmax - dmin) * (1 - 0.25 * (1 - mid)), rel=1e-14)


@pytest.mark.parametrize("sol", SOLS)
def test_ref_unit_mass_on_one_row(sol):
    """A unit mass (inverse weight 1) on one limit-type row, diag = (1 - imp) / imp: the reference acceleration is the spring-damper
    aref = -2 v / (dmax T) - imp pos / (dmax T zeta)^2, and where the row is active the minimiser of 1/2 (a - a0)^2 + 1/2 D (a - aref)^2 is
    a = (1 - imp) a0 + imp aref -- the impedance is the fraction of the way from the free to the reference acceleration; where a0 >= aref the
    row is inactive and a = a0."""
    T, zeta, _, dmax = sol[:4]
    rng = np.random.default_rng(5)
    for x in (0.1, 0.45, 0.7, 0.99, 2.5):
        pos, vel, a0 = -x * sol[4], rng.standard_normal() * 0.05, -9.81
        imp, aref, _ = imp_aref(sol, pos, vel)
        assert aref == pytest.approx(-2.0 * vel / (dmax * T) - imp * pos / (dmax * T * zeta) ** 2, rel=1e-14)
        D = imp / (1.0 - imp)
        M, J = np.eye(1), np.ones((1, 1))
        a, cost, active, res = solve_constraints(M, np.array([a0]), J, np.array([aref]), np.array([D]))
        assert aref > a0 and active[0] and res <= 1e-10
        assert a[0] == pytest.approx((1 - imp) * a0 + imp * aref, rel=1e-12)
        assert cost == pytest.approx(0.5 * imp * (aref - a0) ** 2, rel=1e-12)       # 1/2 (1 / (1 + 1 / D)) (aref - a0)^2
        assert constraint_force(J, np.array([aref]), np.array([D]), a)[0] == pytest.approx(a[0] - a0, rel=1e-12)   # M (a - a0) = J^T force
        a, cost, active, _ = solve_constraints(M, np.array([aref + 1.0]), J, np.array([aref]), np.array([D]))
        assert a[0] == aref + 1.0 and cost == 0.0 and not active[0]


def test_ref_contact_params():
    """Friction is the larger of the two geoms' friction x ratio and at least 0.01; the solver parameters are the mean of the two geoms'; the
    inverse weight is the sum of the two links' translational ones, the ground's link having none."""
    import copy

    m = copy.deepcopy(_model("go2"))
    m["geoms"][15]["sol_params"] = [0.04, 0.5, 0.5, 0.75, 0.003, 0.25, 3.0]
    ref = RigidRef(m)
    ng = len(m["geoms"])
    fric, ratio = np.linspace(0.5, 1.5, ng), np.ones(ng)
    ratio[15], ratio[19] = 0.25, 2.0
    w = lambda g: float(np.float32(m["links"][m["geoms"][g]["link"]]["invweight"][0]))   # noqa: E731
    mu, sol, wt = ref.contact_params(0, 15, fric, ratio)
    assert mu == max(fric[0], 0.25 * fric[15]) == 0.5 and wt == w(15) > 0
    assert np.allclose(sol, [0.03, 0.75, 0.7, 0.85, 0.002, 0.375, 2.5], rtol=1e-7, atol=0)
    mu, sol, wt = ref.contact_params(15, 19, fric, ratio)
    assert mu == 2.0 * fric[19] and wt == w(15) + w(19)
    assert ref.contact_params(0, 15, 0.001 * fric, ratio)[0] == 0.01
    q = ref.qpos0.copy()
    q[7:] += STAND_LEVEL                                              # (within every joint limit)
    k = ref.fk(q)
    contact = [(0, 15, k["p"][10], np.array([0.0, 0.0, 1.0]), 0.0005)]
    P = ref.constraint_problem(k, q, np.zeros(ref.nd), contact, fric, ratio)
    sol_mix = ref.contact_params(0, 15, fric, ratio)[1]
    imp = impedance(sol_mix, -0.0005)[0]
    assert P["J"].shape == (4, ref.nd) and (P["imp"] == imp).all() and (P["branch"] == BRANCH_LOW).all() and not P["is_limit"].any()
    assert P["D"] == pytest.approx(1.0 / ((w(15) + 0.25 * w(15)) * 2 * 0.25 * (1 - imp) / imp), rel=1e-14)
    assert P["aref"] == pytest.approx(imp * 0.0005 / (sol_mix[3] * sol_mix[0] * sol_mix[1]) ** 2, rel=1e-14)     # at rest: the spring term alone


def test_ref_constraint_solver_on_random_problems():
    """solve_constraints on random strictly convex problems with rows that switch during the solve: the returned point has a vanishing gradient
    M (a - a0) = J^T force(a), and no point around it has a lower cost."""
    rng = np.random.default_rng(6)
    for n, nr in ((3, 2), (6, 9), (18, 40)):
        A = rng.standard_normal((n, n))
        M = A @ A.T + 0.1 * np.eye(n)
        J, aref, D, a0 = rng.standard_normal((nr, n)), rng.standard_normal(nr) * 3, rng.uniform(0.1, 50.0, nr), rng.standard_normal(n) * 3
        a, cost, active, res = solve_constraints(M, a0, J, aref, D)
        force = constraint_force(J, aref, D, a)
        assert res <= 1e-10 and 0 < active.sum() < nr and np.array_equal(active, force > 0)
        assert np.abs(M @ (a - a0) - J.T @ force).max() <= 1e-9 * (np.abs(M) @ np.abs(a0)).max()
        assert cost == pytest.approx(constraint_cost(M, a0, J, aref, D, a), rel=1e-14)
        for _ in range(20):
            assert constraint_cost(M, a0, J, aref, D, a + 1e-3 * rng.standard_normal(n)) > cost


# ---------------------------------------------------------------------------------------------------- states
def _quat_cases(rng, B):
    """Whole sphere with w < 0, a near-180-degree rotation and one non-unit stored quaternion."""
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0] = -np.abs(q[0]) * np.array([1, 1, 1, 1])                                            # w < 0
    ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
    q[1] = np.concatenate([[np.cos(0.5 * (np.pi - 1e-3))], np.sin(0.5 * (np.pi - 1e-3)) * ax])     # 179.94 degrees
    q[2] *= 1.7                                                                                  # non-unit: the library normalises it
    return q


def make_states(ref, B, seed, contact=False):
    """float32 state arrays (k, B) of B states, state b drawn from seed + b (its own stream).  contact=True: upright robots low enough that feet and
    calves are in the ground, with some joints past their limits."""
    nl, nd, nq = ref.nl, ref.nd, ref.nq
    qpos = np.zeros((nq, B)); vel = np.zeros((nd, B)); ms = np.zeros((nl, B)); cs = np.zeros((nl, 3, B))
    quats = _quat_cases(np.random.default_rng(seed + 1000), B)
    lim = ref.limit[6:]
    bounded = np.abs(lim).max(axis=1) < 1e29
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        big = b % 2 == 1
        if contact:
            tilt = rng.standard_normal(3) * 0.15
            qpos[3:7, b] = np.concatenate([[np.cos(0.5 * np.linalg.norm(tilt))], np.sin(0.5 * np.linalg.norm(tilt)) * tilt / np.linalg.norm(tilt)])
            qpos[0:3, b] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0.15, 0.3)]
        else:
            qpos[3:7, b] = quats[b]
            qpos[0:3, b] = [rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(1.5, 3.0)]          # clear of the ground for any orientation
        lo = np.where(bounded, lim[:, 0], -np.pi); hi = np.where(bounded, lim[:, 1], np.pi)
        span = hi - lo
        qpos[7:, b] = rng.uniform(lo - 0.1 * span, hi + 0.1 * span)                                  # across the range, slightly outside it
        if contact:
            qpos[7:, b] = np.where(rng.random(nd - 6) < 0.7, np.clip(ref.qpos0[7:] + np.array(_stand(ref)) + 0.2 * rng.standard_normal(nd - 6), lo - 0.1 * span, hi + 0.1 * span), qpos[7:, b])
            j = b % (nd - 6)                                                                         # at least one joint past a limit
            if bounded[j]:
                qpos[7 + j, b] = hi[j] + rng.uniform(0.02, 0.15) if b % 2 else lo[j] - rng.uniform(0.02, 0.15)
        vel[0:3, b] = rng.standard_normal(3) * (3.0 if big else 0.5)
        w = rng.standard_normal(3)
        vel[3:6, b] = w / np.linalg.norm(w) * (rng.uniform(12, 20) if big else rng.uniform(0, 2))
        vel[6:, b] = rng.standard_normal(nd - 6) * (15.0 if big else 2.0)
        # DR shifts at and beyond the walk cfg ranges (base mass [-1, 3], COM +-0.03, leg mass +-0.5)
        ms[1, b] = rng.choice([-1.5, -1.0, 3.0, 4.5]) if b % 3 == 0 else rng.uniform(-1.5, 4.5)
        ms[2:, b] = rng.uniform(-0.75, 0.75, nl - 2) * np.minimum(1.0, np.array([L["inertial_mass"] for L in ref.links[2:]]) / 1.0)
        cs[1:, :, b] = rng.uniform(-0.045, 0.045, (nl - 1, 3))
    return dict(F_QPOS=qpos.astype(np.float32), F_VEL=vel.astype(np.float32), F_MASS_SHIFT=ms.astype(np.float32),
                F_COM_SHIFT=cs.reshape(nl * 3, B).astype(np.float32))


def _stand(ref):
    if ref.m.get("robot") == "go2":
        return [0, 0, 0, 0, 0.8, 0.8, 1.0, 1.0, -1.5, -1.5, -1.5, -1.5]
    return [0.0] * (ref.nd - 6)


STAND_LEVEL = [0, 0, 0, 0, 0.9, 0.9, 0.9, 0.9, -1.5, -1.5, -1.5, -1.5]    # front and rear thighs alike: the four feet of a level go2 at one height
SHALLOW_DEPTHS = (0.2e-3, 0.7e-3, 0.4e-3, 0.95e-3)                         # of the lowest foot sphere; the contact width of the impedance curve is 1 mm
SHALLOW_LIMIT = (2e-4, 7e-4)                                                # rad past a limit; the width of the joints' curve is 1e-3 rad
FOOT_RADIUS = 0.022


def make_shallow_states(ref, B, seed):
    """States of a robot standing level on flat ground at sub-millimetre penetrations, where the impedance is on its polynomial branches (a contact
    deeper than the 1 mm width or a limit violation above 1e-3 rad takes the saturated value).  In periods of eight envs: the depth of the lowest
    foot sphere is SHALLOW_DEPTHS[b % 4] (two below the midpoint of the curve, two above); envs 2, 3, 6, 7 have 0.05 rad of joint noise (one foot
    down), the others none (several feet at one depth); envs 4-7 have one hip or calf joint SHALLOW_LIMIT[b % 2] past a limit.  The base height
    comes from the reference's kinematics; velocities are small."""
    assert ref.m.get("robot") == "go2"
    nl, nd, nq = ref.nl, ref.nd, ref.nq
    qpos = np.zeros((nq, B), np.float32); vel = np.zeros((nd, B)); ms = np.zeros((nl, B)); cs = np.zeros((nl, 3, B))
    lim = ref.limit.astype(np.float32).astype(np.float64)[6:]
    feet = [g for g in ref.m["geoms"] if g["type"] == 1 and g["data"][0] == FOOT_RADIUS]
    assert len(feet) == 4
    limit_joints = [(j, side) for j in (0, 1, 2, 3, 8, 9, 10, 11) for side in ((0, 1) if j < 4 else (1,))]   # hips both ways, calves at the upper (straight) end
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        q = ref.qpos0.copy()
        q[7:] += STAND_LEVEL
        if b % 4 >= 2:
            q[7:] += 0.05 * rng.standard_normal(nd - 6)
        q = q.astype(np.float32)
        if b % 8 >= 4:
            j, side = limit_joints[(b // 8 + b % 4 * 3) % len(limit_joints)]
            over = SHALLOW_LIMIT[b % 2]
            q[7 + j] = lim[j, 1] + over if side else lim[j, 0] - over
        q[0:2] = rng.uniform(-0.5, 0.5, 2)
        q[2] = 0.0
        k = ref.fk(q.astype(np.float64))
        lowest = min((k["p"][g["link"]] + k["R"][g["link"]] @ np.asarray(g["pos"]))[2] for g in feet) - FOOT_RADIUS
        q[2] = -lowest - SHALLOW_DEPTHS[b % 4]                         # the ground's top face is z = 0
        qpos[:, b] = q
        vel[:, b] = rng.standard_normal(nd) * np.concatenate([[0.01] * 3, [0.03] * 3, [0.05] * (nd - 6)])
        ms[1, b] = rng.uniform(-1.0, 3.0)
        ms[2:, b] = rng.uniform(-0.1, 0.1, nl - 2)
        cs[1:, :, b] = rng.uniform(-0.01, 0.01, (nl - 1, 3))
    return dict(F_QPOS=qpos, F_VEL=vel.astype(np.float32), F_MASS_SHIFT=ms.astype(np.float32), F_COM_SHIFT=cs.reshape(nl * 3, B).astype(np.float32))


def load_states(h, st):
    for name, arr in st.items():
        h.put(name, arr)
    h.sim.reset_caches(); h.sim.forward_kinematics()


def _f64(st):
    return {k: v.astype(np.float64) for k, v in st.items()}


def ref_kin(ref, st, b):
    s = _f64(st)
    return ref.fk(s["F_QPOS"][:, b], s["F_VEL"][:, b], s["F_MASS_SHIFT"][:, b], s["F_COM_SHIFT"][:, b].reshape(ref.nl, 3))


# ---------------------------------------------------------------------------------------------------- the cases
MODELS = {"go2": lambda: load_model_json(), "anymal_c": lambda: _model("anymal_c")}
B = 8


def _worst(errs):
    return max(errs) if errs else 0.0


def case_kinematics(h, ref, st, n_chk):
    """(a) FK and COM-frame velocities; returns the largest errors."""
    lp, lq = h.get("F_LINK_POS").reshape(ref.nl, 3, -1), h.get("F_LINK_QUAT").reshape(ref.nl, 4, -1)
    cdv, cda = h.get("F_LINK_CDVEL").reshape(ref.nl, 3, -1), h.get("F_LINK_CDANG").reshape(ref.nl, 3, -1)
    rc, dp = h.get("F_ROOT_COM"), h.get("F_DOF_POS")
    e = dict(pos=[], quat=[], com=[], dof=[], ang=[], vel=[])
    for b in range(n_chk):
        k = ref_kin(ref, st, b)
        e["pos"].append(np.abs(k["p"] - lp[:, :, b]).max())
        for l in range(ref.nl):
            qr = mat_to_quat(k["R"][l])
            e["quat"].append(min(np.abs(qr - lq[l, :, b]).max(), np.abs(qr + lq[l, :, b]).max()))
        e["com"].append(np.abs(k["com"] - rc[:, b]).max())
        dref = ref.dof_pos(st["F_QPOS"][:, b].astype(np.float64))
        sel = [0, 1, 2] + list(range(6, ref.nd))                    # (the free joint's angular dof_pos is evaluated lazily by the getter)
        e["dof"].append(np.abs(dref[sel] - dp[sel, b]).max())
        for l in ref.moving:
            e["ang"].append(np.abs(k["w"][l] - cda[l, :, b]).max() / (1 + np.abs(k["w"][l]).max()))
            vr = ref.point_vel(k, l, k["com"])
            e["vel"].append(np.abs(vr - cdv[l, :, b]).max() / (1 + np.abs(vr).max()))
    return {n: _worst(v) for n, v in e.items()}


# tolerances, measured float32 errors in the comments (strict / fast oracle, both models, worst over the batch)
# measured (strict / fast oracle at 8 envs, HIP at 128): pos 3.0e-7 m, quat 1.5e-7, root COM 6.6e-7 m, dof_pos 0, cd_ang 1.0e-6 and cd_vel 5.7e-6
# relative to 1 + |value|
TOL_KIN = dict(pos=2e-5, quat=2e-5, com=2e-5, dof=1e-6, ang=2e-5, vel=1e-4)


def _controls(h, ref, mode, rng):
    """Sets the control inputs of a case; returns (ctrl_mode, ctrl_pos, ext forces per env) for the reference."""
    Bn = h.B
    cm = np.zeros((ref.nd, Bn), np.int32)
    cp = np.zeros((ref.nd, Bn), np.float32)
    ext = [dict() for _ in range(Bn)]
    h.put("F_CTRL_FORCE", np.zeros((ref.nd, Bn), np.float32))
    h.put("F_CTRL_VEL", np.zeros((ref.nd, Bn), np.float32))
    h.put("F_EXT_FORCE", np.zeros((ref.nl * 6, Bn), np.float32))
    if mode == "position":
        for d in range(6, ref.nd):                                   # gains whose PD force exceeds force_range for large errors: some joints saturate
            kp, kv, fr = 40.0 + 5 * d, 0.5 + 0.1 * d, float(min(ref.force_range[d, 1], 20.0 + d))
            h.sim.set_dof_gains(d, kp, kv, -fr, fr)
            ref.set_dof_gains(d, kp, kv, -fr, fr)
        cm[6:] = 2
        cp[6:] = rng.uniform(-1.0, 1.0, (ref.nd - 6, Bn)).astype(np.float32)
        h.put("F_CTRL_POS", cp)
    h.put("I_CTRL_MODE", cm)
    return cm, cp, ext


def _set_ext(h, ref, st, rng):
    """A push-style wrench on two links per env, written as the env's push path writes it: ext_vel -= f, ext_ang -= (p_link - root_com) x f."""
    Bn = h.B
    lp = h.get("F_LINK_POS").reshape(ref.nl, 3, Bn).astype(np.float64)
    rc = h.get("F_ROOT_COM").astype(np.float64)
    ext = np.zeros((ref.nl, 6, Bn), np.float32)
    forces = [dict() for _ in range(Bn)]
    for b in range(Bn):
        for l in (1, int(rng.integers(2, ref.nl))):
            f = rng.standard_normal(3) * 40.0
            forces[b][l] = forces[b].get(l, 0) + f
    for b in range(Bn):
        for l, f in forces[b].items():
            f32 = np.asarray(f, np.float32)
            ext[l, 3:, b] -= f32
            ext[l, :3, b] -= np.cross(lp[l, :, b] - rc[:, b], f32).astype(np.float32)
    h.put("F_EXT_FORCE", ext.reshape(ref.nl * 6, Bn))
    # the reference sees the force as stored: f = -ext_vel at the link origin, and the moment about the root COM -ext_ang; that moment is
    # (p - com) x f up to float32 rounding, so the reference applies f at the origin
    return [{l: -ext[l, 3:, b].astype(np.float64) for l in forces[b]} for b in range(Bn)]


def case_dynamics(h, ref, st, mode, seed, n_chk):
    """(b)-(e) after one substep.  Returns the largest errors and the float64 references / library outputs for further checks."""
    rng = np.random.default_rng(seed)
    cm, cp, _ = _controls(h, ref, mode, rng)
    ext = _set_ext(h, ref, st, rng) if mode == "ext" else [dict() for _ in range(h.B)]
    h.sim.substep()
    M = h.get("F_MASS_MAT").reshape(ref.nd, ref.nd, -1); f = h.get("F_FORCE"); asm = h.get("F_ACC_SMOOTH")
    acc, q1, v1 = h.get("F_ACC"), h.get("F_QPOS"), h.get("F_VEL")
    s = _f64(st)
    e = dict(M=[], f=[], acc_smooth=[], qpos=[], vel=[], quat_norm=[])
    out = dict(M_ref=[], f=f, acc=acc)
    for b in range(n_chk):
        k = ref_kin(ref, st, b)
        q, v = s["F_QPOS"][:, b], s["F_VEL"][:, b]
        Mr = ref.mass_matrix(k, cm[:, b])
        out["M_ref"].append(Mr)
        e["M"].append(np.abs(Mr - M[:, :, b]).max() / np.abs(Mr).max())
        terms = [-ref.bias(k), ref.passive(q, v), ref.applied(q, v, cm[:, b], ctrl_pos=cp[:, b].astype(np.float64)), ref.external(k, ext[b])]
        fr = sum(terms)
        fscale = sum(np.abs(t) for t in terms).max()                       # scale: the sum of the magnitudes of the terms
        e["f"].append(np.abs(fr - f[:, b]).max() / fscale)
        ar = np.linalg.solve(Mr, fr)
        e["acc_smooth"].append(np.abs(ar - asm[:, b]).max() / (np.abs(np.linalg.solve(Mr, np.abs(fr))).max() + np.abs(ar).max()))
        qr, vr = ref.integrate(q, v, acc[:, b].astype(np.float64))
        e["qpos"].append(np.abs(qr - q1[:, b]).max() / (1 + np.abs(qr).max()))
        e["vel"].append(np.abs(vr - v1[:, b]).max() / (1 + np.abs(vr).max()))
        e["quat_norm"].append(abs(np.linalg.norm(q1[3:7, b].astype(np.float64)) - 1))
    return {n: _worst(v) for n, v in e.items()}, out


TOL_DYN = dict(
    M=2e-5,            # relative to max |M|; measured <= 1.5e-7 (go2 / anymal, oracles and HIP)
    f=1e-4,            # relative to the largest per-dof sum of |terms| (bias, passive, applied, external); measured <= 5.9e-6
    acc_smooth=5e-5,   # relative to max |M^-1 |f|| + max |a|; measured <= 2.0e-6 (arrow and row form)
    qpos=5e-6,         # relative to 1 + max |q|: the integrator applied to the library's own acceleration; measured <= 4.7e-8
    vel=5e-6,          # relative to 1 + max |v|; measured <= 1.2e-7
    quat_norm=5e-6,    # the stored quaternion after the step is normalised; measured <= 1.5e-7
)


def _check(errs, tol, what):
    bad = {n: (errs[n], tol[n]) for n in tol if n in errs and not errs[n] <= tol[n]}
    assert not bad, f"{what}: error / tolerance {bad} (all: {errs})"


def _leg_of(ref, l):
    """The child of the root link that carries link l (None for the root, the ground and l = -1)."""
    leg = None
    while l > -1 and l != ref.root:
        leg, l = l, ref.links[l]["parent"]
    return leg if l == ref.root else None


def con_setup(h, ref, seed, ratios=True):
    """Controls off, per-geom friction ratios drawn from the seed.  Returns (ratios, geom friction) as the library holds them."""
    rng = np.random.default_rng(seed)
    _controls(h, ref, "force", rng)
    ng = len(ref.m["geoms"])
    fr = np.ones((ng, h.B), np.float32)
    if ratios:
        fr = rng.choice([0.3, 0.7, 1.0, 1.6], (ng, h.B)).astype(np.float32)
    h.put("F_FRICTION_RATIO", fr)
    return fr, h.get("F_GEOM_FRICTION").astype(np.float64)


def con_check(h, ref, st, fr, gfric, n_chk):
    """(f) the constraint phase of the substep just run from the states st: qfrc_constraint = sum row^T efc_force, M_ref a - f = qfrc_constraint, the
    per-link contact forces, efc_force >= 0; `law`: every row's force is the one the constraint law prescribes at the library's own acceleration;
    `opt`: that acceleration is the minimiser of the float64 constraint problem (M, smooth force, rows, aref and D all from the reference).
    Returns the largest errors and, under `n_...`, what the batch covered."""
    nc, ncon = h.get("I_N_CONTACTS")[0], h.get("I_N_CONSTRAINTS")[0]
    cpos, cnrm = h.get("F_CONTACT_POS").reshape(-1, 3, h.B), h.get("F_CONTACT_NORMAL").reshape(-1, 3, h.B)
    cpen = h.get("F_CONTACT_PEN")
    geoms = h.get("I_CONTACT_GEOMS")
    maxc = geoms.shape[0] // 2
    efc, qfrc, f, acc = h.get("F_EFC_FORCE"), h.get("F_QFRC_CONSTRAINT"), h.get("F_FORCE"), h.get("F_ACC")
    cf = h.get("F_CONTACT_FORCE").reshape(ref.nl, 3, h.B)
    iters = h.get("I_SOLVER_ITERS")[0]
    s = _f64(st)
    e = dict(qfrc=[], kkt=[], cforce=[], efc_min=[], rows=[], law=[], opt=[], opt_cost=[])
    n_branch = np.zeros((2, 3), int)                                   # [contact rows, limit rows] x [low, high, saturated]
    n_coupled = n_active = n_inactive = 0
    for b in range(n_chk):
        k = ref_kin(ref, st, b)
        rows, dirs, links, contacts = [], [], [], []
        for i in range(nc[b]):
            ga, gb = geoms[i, b], geoms[maxc + i, b]
            la, lb = ref.m["geoms"][ga]["link"], ref.m["geoms"][gb]["link"]
            mu = max(gfric[ga, b] * fr[ga, b], gfric[gb, b] * fr[gb, b], 0.01)
            r, d = ref.contact_rows(k, la, lb, cpos[i, :, b].astype(np.float64), cnrm[i, :, b].astype(np.float64), mu)
            rows.append(r); dirs.append(d); links.append((la, lb))
            contacts.append((ga, gb, cpos[i, :, b].astype(np.float64), cnrm[i, :, b].astype(np.float64), float(cpen[i, b])))
        lim = ref.limit_rows(s["F_QPOS"][:, b])
        J = np.concatenate(rows + [lim]) if rows else lim
        e["rows"].append(float(abs(J.shape[0] - ncon[b])))
        lam = efc[:ncon[b], b].astype(np.float64)
        e["efc_min"].append(max(0.0, -lam.min()) if len(lam) else 0.0)
        qr = J.T @ lam
        qscale = (np.abs(J).T @ np.abs(lam)).max() + 1e-3
        e["qfrc"].append(np.abs(qr - qfrc[:, b]).max() / qscale)
        Mr = ref.mass_matrix(k, np.zeros(ref.nd))
        a = acc[:, b].astype(np.float64)
        kkt = Mr @ a - f[:, b]
        kscale = (np.abs(Mr) @ np.abs(a)).max() + np.abs(f[:, b]).max() + qscale
        e["kkt"].append(np.abs(kkt - qfrc[:, b]).max() / kscale)
        cref = np.zeros((ref.nl, 3))
        for i, (la, lb) in enumerate(links):
            force = dirs[i].T @ lam[4 * i:4 * i + 4]
            cref[la] -= force; cref[lb] += force
        e["cforce"].append(np.abs(cref - cf[:, :, b]).max() / (np.abs(cref).max() + 1e-3))
        # the constraint law and the optimum
        P = ref.constraint_problem(k, s["F_QPOS"][:, b], s["F_VEL"][:, b], contacts, gfric[:, b], fr[:, b])
        Jp, aref, D = P["J"], P["aref"], P["D"]
        if Jp.shape[0] != ncon[b]:
            e["law"].append(np.inf); e["opt"].append(np.inf)
            continue
        lscale = (D * (np.abs(Jp) @ np.abs(a) + np.abs(aref))).max() if len(D) else 1.0
        e["law"].append(np.abs(constraint_force(Jp, aref, D, a) - lam).max() / lscale if len(D) else 0.0)
        q, v = s["F_QPOS"][:, b], s["F_VEL"][:, b]
        a0 = np.linalg.solve(Mr, -ref.bias(k) + ref.passive(q, v))                     # (controls off: no actuator force)
        a_opt, cost_opt, active, _ = solve_constraints(Mr, a0, Jp, aref, D)
        e["opt"].append(np.abs(a - a_opt).max() / np.abs(a_opt).max())
        cost_scale = 0.5 * a0 @ Mr @ a0 + 0.5 * (D * aref) @ aref
        e["opt_cost"].append(max(0.0, cost_opt - constraint_cost(Mr, a0, Jp, aref, D, a)) / cost_scale)
        for lim_row in (0, 1):
            n_branch[lim_row] += np.bincount(P["branch"][P["is_limit"] == bool(lim_row)], minlength=3)
        n_coupled += any(None not in (_leg_of(ref, la), _leg_of(ref, lb)) and _leg_of(ref, la) != _leg_of(ref, lb) for la, lb in links)
        n_active += int(active.sum()); n_inactive += int((~active).sum())
    out = {n: _worst(v) for n, v in e.items()}
    out["at_cap"] = float((iters >= ref.m["solver"]["iterations"]).sum())
    out["n_iters"] = int(iters.max())
    out.update(n_low=n_branch[0, 0], n_high=n_branch[0, 1], n_sat=n_branch[0, 2], n_limit_low=n_branch[1, 0], n_limit_high=n_branch[1, 1],
               n_limit_sat=n_branch[1, 2], n_coupled=n_coupled, n_uncoupled=n_chk - n_coupled, n_active=n_active, n_inactive=n_inactive,
               n_contacts=int(nc.sum()), n_limits=sum(len(ref.limit_rows(s["F_QPOS"][:, b])) for b in range(h.B)))
    return out


def case_constraints(h, ref, st, seed, n_chk, case="flat"):
    """One substep from states in contact, checked by con_check; asserts what the batch has to cover.  Returns the errors and what con_setup set."""
    fr, gfric = con_setup(h, ref, seed)
    h.sim.substep()
    errs = con_check(h, ref, st, fr, gfric, n_chk)
    if case == "shallow":
        assert errs["n_contacts"] >= h.B, "every env of the batch touches the ground"
        # ... at the depth it was placed at: the deepest foot-ground contact is the lowest foot sphere (1e-6 m: the float32 kinematics are within
        # 3e-7 m of the reference's, TOL_KIN)
        pen, geoms, nc = h.get("F_CONTACT_PEN"), h.get("I_CONTACT_GEOMS"), h.get("I_N_CONTACTS")[0]
        for b in range(h.B):
            ga, gb = geoms[:nc[b], b], geoms[geoms.shape[0] // 2:geoms.shape[0] // 2 + nc[b], b]
            foot = [i for i in range(nc[b]) if ref.links[ref.m["geoms"][min(ga[i], gb[i])]["link"]]["is_fixed"]
                    and ref.m["geoms"][max(ga[i], gb[i])]["data"][0] == FOOT_RADIUS]
            assert foot and abs(pen[foot, b].max() - SHALLOW_DEPTHS[b % 4]) <= 1e-6, (b, pen[:nc[b], b])
    else:
        assert errs["n_contacts"] >= 2 * h.B, "the batch exercised the contact constraints"
        assert errs["n_limits"] >= h.B, "... and the joint limits"
    if n_chk == h.B:
        if case == "shallow":          # both polynomial branches of the impedance, for contacts and for limits
            assert errs["n_low"] >= 8 and errs["n_high"] >= 8 and errs["n_limit_low"] >= 1 and errs["n_limit_high"] >= 1, errs
        else:                          # the saturated value; both factorisations of the Newton Hessian (a contact between two legs couples their blocks)
            assert errs["n_sat"] >= 8 and errs["n_limit_sat"] >= 1, errs
            assert errs["n_coupled"] >= 1 and errs["n_uncoupled"] >= 1, errs
        assert errs["n_active"] >= 8 and errs["n_inactive"] >= 1, errs
    return errs, (fr, gfric)


TOL_CON = dict(
    rows=0,            # number of rows: 4 per contact + one per violated limit
    efc_min=0.0,       # every row's force is >= 0
    qfrc=2e-5,         # relative to max sum |row| |efc|; measured <= 1.4e-6 (flat and stairs)
    kkt=5e-5,          # relative to max |M| |a| + max |f| + the qfrc scale; measured <= 1.3e-6 (oracles, HIP default and every knob but
    #                    GO2SIM_TERRAIN_SOLVER_TEAM=32, see TOL_CON_EARLY_STOP).  M a - f - qfrc is the Newton gradient at the solver's last iterate
    cforce=5e-5,       # relative to max |contact force|; measured <= 1.0e-6 (stairs)
    # law and opt: ten times the worst value measured on the strict and the fast oracle at 8 and at 128 envs over flat, stairs and shallow; the margin is
    # for other sum orders (16- and 64-lane teams) and other seeds.  The HIP default build is bit-equal to the fast oracle; HIP under the knobs at
    # 128 envs: law <= 8.9e-7, opt <= 1.7e-5 (GO2SIM_TERRAIN_SOLVER_TEAM=32 on stairs, the early stop again; every other knob <= 3.8e-6),
    # warm_law <= 8.4e-7 and warm_opt <= 1.8e-5 (GO2SIM_NO_ARROW=1 on flat ground)
    law=9e-6,          # |efc_force - D max(0, -(J a - aref))| at the library's F_ACC, relative to max D (|J| |a| + |aref|); measured <= 8.7e-7 (stairs;
    #                    flat 2.0e-7, shallow 2.4e-7)
    opt=2e-4,          # max |F_ACC - a*| / max |a*| with a* the float64 minimiser; measured <= 1.7e-5 (strict oracle, stairs at 128 envs: a solve that
    #                    stops an iteration early, see TOL_CON_EARLY_STOP; otherwise stairs 5.0e-6, shallow 3.0e-6, flat 7.1e-7)
    opt_cost=1e-9,     # cost(a*) - cost(F_ACC), both in float64, relative to 1/2 a0^T M a0 + 1/2 sum D aref^2: a* is the minimiser up to a gradient of
    #                    1e-10 of the force scale, so by convexity the cost at any other point is above its by all but ~1e-10 x |F_ACC - a*| / |a*| of it
    at_cap=0,          # number of envs whose solve stopped at the model's iteration cap (50); measured: at most 10 iterations
    # the same after a following warm-started substep (its float32 Jaref has been carried through the previous solve's line searches as well)
    warm_law=4e-5,     # measured <= 3.7e-6 (stairs; flat 9.0e-7, shallow 8.0e-7)
    warm_opt=2e-4,     # measured <= 1.6e-5 (flat and stairs alike; shallow 1.4e-6)
    warm_opt_cost=1e-9,
    warm_at_cap=0,     # measured: at most 8 iterations
)
# GO2SIM_TERRAIN_SOLVER_TEAM=32 on stairs: the KKT residual is not a rounding error but the Newton gradient left when the solve stops on
# `improvement < meaninertia * ND * tolerance`; with the 32-lane sum order some stairs solves stop an iteration earlier and leave 5.6e-5 of the
# scale.  The bound for such solves is the solver's own (1e-4 class, tests/test_fast_order.py), and their F_ACC is separately required to be
# within the fast-order bound of the default build's (test_hip_knob_against_reference)
TOL_CON_EARLY_STOP = dict(TOL_CON, kkt=2e-4)


def _place_on_stairs(h, st):
    """Installs the stair heightfield and moves the robots onto a flight (16 per row, on treads and across step edges), at their height above
    the local ground."""
    hf, info = install_stairs(h.sim)
    hs, vs, (ox, oy, oz) = info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"]
    q = st["F_QPOS"]
    b = np.arange(q.shape[1])
    q[0] += (3.0 + (b % 16) * 0.21).astype(np.float32)
    q[1] += (6.0 + (b // 16) * 0.6).astype(np.float32)
    col = np.clip(((q[0] - ox) / hs).astype(int), 0, hf.shape[0] - 1)
    row = np.clip(((q[1] - oy) / hs).astype(int), 0, hf.shape[1] - 1)
    q[2] += (hf[col, row] * vs + oz).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- one case on one library
SNAP = {
    "kin": ["F_LINK_POS", "F_LINK_QUAT", "F_LINK_CDVEL", "F_LINK_CDANG", "F_ROOT_COM", "F_DOF_POS"],
    "dyn": ["F_MASS_MAT", "F_FORCE", "F_ACC_SMOOTH", "F_ACC", "F_QPOS", "F_VEL"],
    "con": ["F_FORCE", "F_ACC", "F_QPOS", "F_VEL", "F_EFC_FORCE", "F_QFRC_CONSTRAINT", "F_CONTACT_FORCE", "F_CONTACT_POS", "F_CONTACT_NORMAL",
            "F_CONTACT_PEN", "I_N_CONTACTS", "I_N_CONSTRAINTS", "I_CONTACT_GEOMS", "I_SOLVER_ITERS"],
}
CASES = {"kin": "kin", "force": "dyn", "position": "dyn", "ext": "dyn", "flat": "con", "stairs": "con", "shallow": "con"}


MULTI = ["F_QPOS", "F_VEL", "F_ACC", "F_ACC_SMOOTH", "F_FORCE", "F_MASS_MAT", "F_LINK_POS", "F_LINK_QUAT", "F_LINK_CDVEL", "F_LINK_CDANG",
         "F_EFC_FORCE", "F_QFRC_CONSTRAINT", "F_CONTACT_FORCE", "I_N_CONTACTS", "I_N_CONSTRAINTS", "I_SOLVER_ITERS", "I_IS_WARMSTART"]


def run_case(lib, name, case, n_envs, gpu=False, env=None, check=True, more_substeps=0):
    """Loads the case's states into a fresh handle (env: knobs set while the handle is created), runs it, checks nothing.  Returns (errors against
    the reference -- empty with check=False --, the library's fields of the case).  more_substeps > 0: then one scene_step of that many substeps
    (the multi-substep launch sequence: fused solve + integrate + next dynamics, or the separate launches), whose fields join the snapshot.  For a
    constraint case more_substeps = 1 also checks that warm-started substep against the reference (errors under warm_...)."""
    model = MODELS[name]()
    ref = RigidRef(model)
    with with_knobs(env):
        h = Handle(lib, pack_model(model), n_envs, gpu)
    n_chk = n_envs if check else 0
    if CASES[case] == "kin":
        st = make_states(ref, n_envs, seed=100)
        load_states(h, st)
        errs = case_kinematics(h, ref, st, n_chk)
    elif CASES[case] == "dyn":
        st = make_states(ref, n_envs, seed=200 + 10 * len(case))
        load_states(h, st)
        errs, _ = case_dynamics(h, ref, st, case, seed=7, n_chk=n_chk)
    else:
        st = make_shallow_states(ref, n_envs, seed=500) if case == "shallow" else make_states(ref, n_envs, seed=400, contact=True)
        if case == "stairs":
            _place_on_stairs(h, st)
        load_states(h, st)
        errs, con = case_constraints(h, ref, st, seed=9, n_chk=n_chk, case=case)
    snap = {n: h.get(n) for n in SNAP[CASES[case]]}
    if more_substeps:
        h.sim.scene_step(more_substeps)
        snap.update({"after %d substeps: %s" % (more_substeps, n): h.get(n) for n in MULTI})
        if CASES[case] == "con" and more_substeps == 1 and check:
            # the solve of that substep started from the previous acceleration; its problem is rebuilt from the state read back before it
            assert (snap["after 1 substeps: I_IS_WARMSTART"] == 1).all()
            w = con_check(h, ref, dict(st, F_QPOS=snap["F_QPOS"], F_VEL=snap["F_VEL"]), *con, n_chk)
            assert w["n_contacts"] >= n_envs and w["n_active"] >= 8, w
            errs.update({"warm_" + n: v for n, v in w.items()})
    return errs, snap


TOL = {"kin": TOL_KIN, "dyn": TOL_DYN, "con": TOL_CON}


# ---------------------------------------------------------------------------------------------------- CPU: both oracle builds
@pytest.fixture(params=["strict", "fast"])
def cpu_lib(request, oracle_strict_lib, oracle_fast_lib):
    return oracle_strict_lib if request.param == "strict" else oracle_fast_lib


CON_CASES = [("flat", "go2"), ("stairs", "go2"), ("shallow", "go2")]


@pytest.mark.parametrize("case,name", [(c, n) for c in ("kin", "force", "position", "ext") for n in ("go2", "anymal_c")] + CON_CASES)
def test_oracle_against_reference(cpu_lib, case, name):
    errs, _ = run_case(cpu_lib, name, case, B, more_substeps=int(CASES[case] == "con"))
    print(f"oracle {name} {case}:", {n: float("%.2e" % v) for n, v in errs.items()})
    _check(errs, TOL[CASES[case]], f"{name} {case}")


@pytest.mark.parametrize("name", ["go2", "anymal_c"])
def test_oracle_row_form_against_reference(cpu_lib, name):
    """(d) with GO2SIM_NO_ARROW=1 (read when the model is parsed): the dense row-form factorisation of the mass matrix."""
    errs, _ = run_case(cpu_lib, name, "position", B, env={"GO2SIM_NO_ARROW": "1"})
    _check(errs, TOL_DYN, f"{name} row form")


@pytest.mark.parametrize("case", ["flat", "shallow"])
def test_oracle_row_form_contacts_against_reference(oracle_fast_lib, case):
    """(f) with GO2SIM_NO_ARROW=1 on the FAST ORDER oracle (the strict build has no arrow form): every env's Newton Hessian in row form."""
    errs, _ = run_case(oracle_fast_lib, "go2", case, B, env={"GO2SIM_NO_ARROW": "1"}, more_substeps=1)
    _check(errs, TOL_CON, f"go2 {case} row form")


# ---------------------------------------------------------------------------------------------------- GPU: the HIP library and its knobs
B_GPU = 128
GPU_CASES = [(c, n) for c in ("kin", "force", "position", "ext") for n in ("go2", "anymal_c")] + CON_CASES


def _bits_equal_snaps(a, b):
    return [n for n in a if not bits_equal(a[n], b[n])]


@pytest.mark.gpu
@pytest.mark.parametrize("case,name", GPU_CASES)
def test_hip_against_reference_and_oracle(hip_lib, oracle_fast_lib, case, name):
    """(a)-(f) on the HIP library at default settings: within the float64 tolerances, and bit-equal to the FAST ORDER oracle on the same states
    (states the env never reaches: base |w| up to 20 rad/s, DR shifts beyond their ranges)."""
    more = int(CASES[case] == "con")                       # (the constraint cases: then a warm-started substep)
    errs, snap = run_case(hip_lib, name, case, B_GPU, gpu=True, more_substeps=more)
    print(f"hip default {name} {case}:", {n: float("%.2e" % v) for n, v in errs.items()})
    _check(errs, TOL[CASES[case]], f"hip {name} {case}")
    _, ref_snap = run_case(oracle_fast_lib, name, case, B_GPU, check=False, more_substeps=more)
    assert not _bits_equal_snaps(snap, ref_snap), f"HIP vs fast oracle differ in {_bits_equal_snaps(snap, ref_snap)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["go2", "anymal_c"])
def test_hip_row_form_against_reference_and_oracle(hip_lib, oracle_fast_lib, name):
    env = {"GO2SIM_NO_ARROW": "1"}
    errs, snap = run_case(hip_lib, name, "position", B_GPU, gpu=True, env=env)
    print(f"hip NO_ARROW {name}:", {n: float("%.2e" % v) for n, v in errs.items()})
    _check(errs, TOL_DYN, f"hip {name} row form")
    _, ref_snap = run_case(oracle_fast_lib, name, "position", B_GPU, env=env)
    assert not _bits_equal_snaps(snap, ref_snap), f"HIP vs fast oracle differ in {_bits_equal_snaps(snap, ref_snap)}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["flat", "shallow"])
def test_hip_row_form_contacts_against_reference_and_oracle(hip_lib, oracle_fast_lib, case):
    """GO2SIM_NO_ARROW=1 with contacts: the row-form factorisation of the Newton Hessian in every env (by default only envs with a contact between two
    legs take it), against the float64 constraint law and optimum, cold and warm-started, and bit-equal to the oracle under the same switch."""
    env = {"GO2SIM_NO_ARROW": "1"}
    errs, snap = run_case(hip_lib, "go2", case, B_GPU, gpu=True, env=env, more_substeps=1)
    print(f"hip NO_ARROW go2 {case}:", {n: float("%.2e" % v) for n, v in errs.items()})
    _check(errs, TOL_CON, f"hip go2 {case} row form")
    _, ref_snap = run_case(oracle_fast_lib, "go2", case, B_GPU, env=env, check=False, more_substeps=1)
    assert not _bits_equal_snaps(snap, ref_snap), f"HIP vs fast oracle differ in {_bits_equal_snaps(snap, ref_snap)}"


# knob -> (cases, rule[, tolerances of the constraint case]).  "bits": the knob changes the launch shape only (which kernel, how many envs per
# workgroup, dispatch order); the arithmetic of every env is that of the default build -> bit equality with it, after the single substep AND after
# a following scene_step of MORE_SUBSTEPS substeps (what selects the fused solve + integrate + next-dynamics launch, the k_integrate_fk_dynamics_team
# split between substeps or the separate launches; each knob below changes that choice).  The env-step kernels (k_pre_dynamics_team, k_env_pre,
# the step graph with GO2SIM_PAR_PRE) are covered by test_hip_knob_env_step.  "solver": the team width of the Newton solve sets the butterfly-tree
# order of its row / dof sums (README: a 16-lane team gives other last bits) -> float64 tolerances, and F_ACC within the test_fast_order.py bound
# of the default build.  "tol": the float64 tolerances.
FLAT = ("force", "position", "ext", "flat", "shallow")
MORE_SUBSTEPS = 3
KNOBS = {
    "GO2SIM_DYN_TEAM=16": (FLAT, "tol"),              # row-form mass factorisation (the arrow form needs 32 / 64 lanes): other last bits
    "GO2SIM_DYN_TEAM=64": (FLAT, "bits"),             # the same arrow-form arithmetic per env as 32 lanes; k_integrate_fk_dynamics_team<64>
    "GO2SIM_FK_TEAM=32": (FLAT + ("stairs",), "bits"),   # k_fk_team<T>; on stairs the last substep's k_integrate_fk_team<T>
    "GO2SIM_FK_TEAM=64": (FLAT + ("stairs",), "bits"),
    "GO2SIM_COLLIDE_TEAM=32": (FLAT + ("stairs",), "bits"),
    "GO2SIM_COLLIDE_TEAM=64": (FLAT + ("stairs",), "bits"),
    "GO2SIM_SOLVER_TEAM=16": (FLAT, "solver"),
    "GO2SIM_SOLVER_TEAM=64": (FLAT, "solver"),
    "GO2SIM_TERRAIN_SOLVER_TEAM=32": (("stairs",), "solver", TOL_CON_EARLY_STOP),
    "GO2SIM_NO_LPT=1": (("stairs",), "bits"),         # heaviest-first dispatch exists on heightfield scenes only (lpt_enabled: off on flat ground)
    "GO2SIM_NO_FUSE=1": (FLAT, "bits"),               # separate integrate / dynamics launches between substeps
    "GO2SIM_NO_FUSE_SOLVE=1": (FLAT, "bits"),         # solve and integrate as separate launches on flat ground
}


def _acc_within_fast_order_bound(a, b):
    """tests/test_fast_order.py: |a - b| <= 1e-5 x the per-env acceleration scale + 1e-6 when both solves stop at the same Newton iteration,
    1e-4 x the scale + 1e-6 otherwise.  Returns the worst ratio to that bound."""
    scale = np.abs(a["F_ACC"]).max(axis=0, keepdims=True)
    if "I_SOLVER_ITERS" in a:
        same = a["I_SOLVER_ITERS"] == b["I_SOLVER_ITERS"]
    else:
        same = np.ones_like(scale, bool)
    return float((np.abs(a["F_ACC"] - b["F_ACC"]) / (np.where(same, 1e-5, 1e-4) * scale + 1e-6)).max())


def _env_of(knob):
    return dict(kv.split("=") for kv in knob.split(","))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", list(KNOBS))
def test_hip_knob_against_reference(hip_lib, knob):
    """(b)-(f) on the HIP library under one launch-shape knob, set before the handle is created (read at go2sim_create)."""
    cases, rule = KNOBS[knob][:2]
    tol_con = KNOBS[knob][2] if len(KNOBS[knob]) > 2 else TOL_CON
    more = MORE_SUBSTEPS if rule == "bits" else 0
    for case in cases:
        errs, snap = run_case(hip_lib, "go2", case, B_GPU, gpu=True, env=_env_of(knob), more_substeps=more)
        _, base = run_case(hip_lib, "go2", case, B_GPU, gpu=True, check=False, more_substeps=more)
        diff = _bits_equal_snaps(snap, base)
        print(f"hip {knob} {case}:", {n: float("%.2e" % v) for n, v in errs.items()}, "fields differing from default:", diff)
        if rule == "solver":
            if "I_N_CONTACTS" in snap:
                assert np.array_equal(snap["I_N_CONTACTS"], base["I_N_CONTACTS"]) and np.array_equal(snap["I_N_CONSTRAINTS"], base["I_N_CONSTRAINTS"])
            w = _acc_within_fast_order_bound(snap, base)
            print(f"  F_ACC vs default: {w:.3f} x the fast-order bound")
            assert w <= 1.0, f"{knob} {case}: F_ACC differs from the default build by {w:.2f} x the test_fast_order.py bound"
        _check(errs, tol_con if CASES[case] == "con" else TOL[CASES[case]], f"{knob} {case}")
        if rule == "bits":
            assert not diff, f"{knob} {case}: fields differ from the default build: {diff}"


# knobs that change only the launch shape of the ENV STEP (its step graph, the fused pre-physics + dynamics kernel, the separate k_env_pre), with
# the tasks that reach them: bit equality with the default build on every observation, reward and done flag of every step and on the final state
ENV_STEP_KNOBS = {
    "GO2SIM_PAR_PRE=1": ("walk", "stairs"),           # the first collision pass as a second root of the step graph (step_graph_build)
    "GO2SIM_NO_FUSE=1": ("walk",),                    # k_env_pre, then separate dynamics / integrate launches
    "GO2SIM_DYN_TEAM=64": ("walk",),                  # k_pre_dynamics_team<64>, k_integrate_fk_dynamics_team<64>
    "GO2SIM_NO_FUSE_SOLVE=1": ("walk",),
    "GO2SIM_FK_TEAM=64": ("walk", "stairs"),          # k_fk_team<64> of the in-step reset path, k_integrate_fk_team<64> on stairs
    "GO2SIM_COLLIDE_TEAM=64": ("walk", "stairs"),
    "GO2SIM_NO_LPT=1": ("stairs",),
    "GO2SIM_NO_GRAPH=1": ("walk",),                   # the kernels of a step launched one by one instead of as a hipGraph
}


@pytest.mark.gpu
@pytest.mark.parametrize("knob", list(ENV_STEP_KNOBS))
def test_hip_knob_env_step(hip_lib, blob, knob):
    from go2_sim2real_locomotion_rl_amd.configs import get_stair_cfgs, get_walk_cfgs

    n_envs, steps = 128, 20
    for task in ENV_STEP_KNOBS[knob]:
        with with_knobs(_env_of(knob)):
            env_k = GpuEnv(hip_lib, blob, n_envs, seed=3, task=task)
        env_d = GpuEnv(hip_lib, blob, n_envs, seed=3, task=task)
        env_k.reset(); env_d.reset()
        cfg = (get_stair_cfgs if task == "stairs" else get_walk_cfgs)()[0]
        max_ep = int(np.ceil(cfg["episode_length_s"] / 0.02))                       # (policy dt 0.02 s)
        ep = env_d.torch.from_numpy((max_ep - 15 + np.arange(n_envs) % 16).astype(np.int32)).to(env_d.dev)   # staggered time-outs: the in-step reset path
        env_k.sim.env_set_episode_length(ep); env_d.sim.env_set_episode_length(ep)
        acts = make_actions(steps, n_envs, seed=3, kind="mixed", n_act=env_d.n_act)
        resets = 0
        for s, a in enumerate(acts):
            out_k, out_d = env_k.step(a), env_d.step(a)
            bad = outputs_differing(out_k, out_d)
            assert not bad, f"{knob} {task} step {s}: {bad} differ from the default build"
            resets += int(out_d[3].sum())
        for name in ("F_QPOS", "F_VEL", "F_ACC", "F_EFC_FORCE", "I_N_CONTACTS", "I_SOLVER_ITERS"):
            assert bits_equal(env_k.field(name), env_d.field(name)), f"{knob} {task}: {name} after {steps} steps"
        assert resets >= n_envs // 2, "the run went through the reset path"
        assert env_k.sim.check_errno() == 0 and env_d.sim.check_errno() == 0
        if knob != "GO2SIM_NO_GRAPH=1":                  # the step ran as a hipGraph (where GO2SIM_PAR_PRE acts), without a fallback
            assert env_k.sim.graph_status() == (True, 0), env_k.sim.graph_status()
        else:
            assert env_k.sim.graph_status()[0] is False
        print(f"hip env step {knob} {task}: {steps} steps bit-equal to the default build ({resets} resets)")
