"""FAST ORDER against the strict oracle (oracle/go2sim_cpu.cpp, `GO2SIM_FAST_ORDER`).

The HIP product sums constraint rows / dofs with lane-parallel butterfly trees and uses reciprocal forms in the triangular solves and the rank-1
Cholesky rotations; libgo2sim_cpu_fast.so mirrors that arithmetic bit for bit (every `-m gpu` parity test compares the HIP library with it at
tolerance 0).  These tests bound what the change of order does to the results, against the strict oracle that follows the reference's CPU
(serial) variants -- north_star's "within a stated fp32 tolerance, with contact counts and done masks bit-exact":

* one rigid substep from IDENTICAL states (the strict trajectory's state is uploaded into the fast oracle before every step, so no chaotic growth
  enters): accelerations within 1e-5 of the per-env acceleration scale (+ 1e-6 absolute) for every env whose two solves stop at the SAME Newton
  iteration (measured: <= 1.6e-6 of the scale); 5-8 % of the solves stop at different iterations (one apart, rarely two) -- the solve stops on `improvement < tol`, both iterates
  are then converged to the solver's own tolerance -- and for those the bound is the solver's: 1e-4 of the scale (measured: <= 6e-5, one stairs env
  with 56 rows); positions / velocities after the step within the substep (0.01 s) times the acceleration bound + 2e-6, contact counts and constraint counts equal;
* free trajectories over a short horizon: observations within 2e-4, rewards within 2e-5 after 4 env steps, done masks and contact counts equal.
"""
import numpy as np
import pytest

from util import CpuEnv, F, make_actions, with_knobs

STATE = ["F_QPOS", "F_VEL", "F_QACC_WS", "F_CTRL_FORCE", "F_CTRL_POS", "F_CTRL_VEL", "F_EXT_FORCE", "F_MASS_SHIFT", "F_COM_SHIFT", "F_GEOM_FRICTION",
         "F_NORMAL_CACHE", "F_SORT_VALUE"]
ISTATE = ["I_CTRL_MODE", "I_IS_WARMSTART", "I_FIRST_TIME", "I_SORT_IG"]


def _copy_state(src, dst):
    for name in STATE + ISTATE:
        dst.sim.set_field_np(F(name), src.field(name))
    dst.sim.forward_kinematics()


@pytest.mark.parametrize("task,kind", [("walk", "0.5"), ("walk", "2.0"), ("stairs", "0.5"), ("jump", "0.5")])
def test_one_substep_from_identical_states(oracle_strict_lib, oracle_fast_lib, blob, task, kind):
    n, steps = 48, 40
    strict = CpuEnv(oracle_strict_lib, blob, n, seed=4, task=task)
    fast = CpuEnv(oracle_fast_lib, blob, n, seed=4, task=task)
    strict.reset(); fast.reset()
    acts = make_actions(steps, n, seed=4, kind=kind, n_act=strict.n_act)
    worst_acc = worst_q = 0.0
    n_rows = 0
    for s in range(steps):
        strict.step(acts[s])                                           # advances the strict trajectory (env step: control inputs, resets)
        _copy_state(strict, fast)
        strict.sim.substep(); fast.sim.substep()                       # one rigid substep from the same state on both
        assert np.array_equal(strict.field("I_N_CONTACTS"), fast.field("I_N_CONTACTS")), f"step {s}: contact counts"
        assert np.array_equal(strict.field("I_N_CONSTRAINTS"), fast.field("I_N_CONSTRAINTS")), f"step {s}: constraint counts"
        a_s, a_f = strict.field("F_ACC"), fast.field("F_ACC")
        scale = np.abs(a_s).max(axis=0, keepdims=True)
        same_it = (strict.field("I_SOLVER_ITERS") == fast.field("I_SOLVER_ITERS"))                # [1, n]: the two solves stopped at the same iteration
        err = np.abs(a_s - a_f) / (np.where(same_it, 1e-5, 1e-4) * scale + 1e-6)
        worst_acc = max(worst_acc, float(err.max()))
        # the state after the step inherits the acceleration difference times the substep (0.01 s): bound = dt x the acceleration bound + 2e-6
        qb = 0.01 * (np.where(same_it, 1e-5, 1e-4) * scale + 1e-6) + 2e-6
        worst_q = max(worst_q, float((np.abs(strict.field("F_QPOS") - fast.field("F_QPOS")) / qb).max()), float((np.abs(strict.field("F_VEL") - fast.field("F_VEL")) / qb).max()))
        n_rows += int(strict.field("I_N_CONSTRAINTS").sum())
        _copy_state(strict, fast)                                       # (the extra substep is undone on the fast side by the next upload; the strict env
        #                                                                  simply continues from its own post-substep state: one more substep of physics per step)
    assert n_rows > 20 * steps, "the run exercised the constraint solver"
    assert worst_acc <= 1.0, f"accelerations differ by {worst_acc:.2f} x the stated bound"
    assert worst_q <= 1.0, f"positions / velocities after one substep differ by {worst_q:.2f} x the stated bound"


@pytest.mark.parametrize("task", ["walk", "stairs", "jump"])
def test_short_free_trajectories(oracle_strict_lib, oracle_fast_lib, blob, task):
    n, steps = 64, 4
    strict = CpuEnv(oracle_strict_lib, blob, n, seed=9, task=task)
    fast = CpuEnv(oracle_fast_lib, blob, n, seed=9, task=task)
    strict.reset(); fast.reset()
    acts = make_actions(steps, n, seed=9, kind="0.5", n_act=strict.n_act)
    for s in range(steps):
        o_s, p_s, r_s, d_s, t_s = strict.step(acts[s])
        o_f, p_f, r_f, d_f, t_f = fast.step(acts[s])
        assert np.array_equal(d_s, d_f) and np.array_equal(t_s, t_f), f"step {s}: done masks"
        assert np.array_equal(strict.field("I_N_CONTACTS"), fast.field("I_N_CONTACTS")), f"step {s}: contact counts"
        assert np.abs(o_s - o_f).max() <= 2e-4, f"step {s}: observations differ by {np.abs(o_s - o_f).max():.2e}"
        assert np.abs(r_s - r_f).max() <= 2e-5, f"step {s}: rewards differ by {np.abs(r_s - r_f).max():.2e}"


@pytest.mark.parametrize("task,kind", [("walk", "2.0"), ("stairs", "0.5"), ("jump", "0.5")])
def test_free_run_statistics_agree(oracle_strict_lib, oracle_fast_lib, blob, task, kind):
    """Free runs diverge bit-wise after a few steps (contact-rich dynamics amplify the last bit), so the long-horizon statement is statistical: over
    512 envs x 300 steps the strict and the FAST ORDER oracle give the same behaviour -- mean reward, resets (falls / time-outs) and mean contact
    count.  Measured: mean reward within 0.8 %, resets within 1, contacts within 0.2 %."""
    n, steps = 512, 300
    stats = {}
    for name, lib in (("strict", oracle_strict_lib), ("fast", oracle_fast_lib)):
        env = CpuEnv(lib, blob, n, seed=21, task=task)
        env.reset()
        acts = make_actions(steps, n, seed=21, kind=kind, n_act=env.n_act)
        rew = contacts = 0.0
        resets = 0
        for a in acts:
            _, _, r, d, _ = env.step(a)
            rew += float(r.mean()); resets += int(d.sum()); contacts += float(env.field("I_N_CONTACTS").mean())
        stats[name] = (rew / steps, resets, contacts / steps)
    (r_s, n_s, c_s), (r_f, n_f, c_f) = stats["strict"], stats["fast"]
    assert abs(r_s - r_f) <= 0.03 * abs(r_s) + 1e-3, f"mean reward {r_s:.5f} vs {r_f:.5f}"
    assert abs(n_s - n_f) <= 0.05 * n_s + 3, f"resets {n_s} vs {n_f}"
    assert abs(c_s - c_f) <= 0.02 * c_s + 0.02, f"mean contacts {c_s:.4f} vs {c_f:.4f}"


def test_arrow_form_against_row_form(oracle_fast_lib, blob):
    """The FAST ORDER factorisation of the Newton Hessian has two forms: the arrow form (legs eliminated first, csrc/go2sim.hip ts_cholesky_factor_arrow /
    oracle cholesky_factor_arrow) whenever no Hessian entry couples two legs, and the dense row form otherwise.  GO2SIM_NO_ARROW=1 (read when a model is
    parsed) switches the arrow form off; both solve the same systems, so short free runs agree like fast against strict."""
    n, steps = 64, 4
    arrow = CpuEnv(oracle_fast_lib, blob, n, seed=9, task="walk")
    with with_knobs({"GO2SIM_NO_ARROW": "1"}):
        rows = CpuEnv(oracle_fast_lib, blob, n, seed=9, task="walk")
    arrow.reset(); rows.reset()
    acts = make_actions(24, n, seed=9, kind="0.5", n_act=arrow.n_act)
    differ = False
    for s in range(steps):
        o_a, p_a, r_a, d_a, t_a = arrow.step(acts[s])
        o_r, p_r, r_r, d_r, t_r = rows.step(acts[s])
        assert np.array_equal(d_a, d_r) and np.array_equal(arrow.field("I_N_CONTACTS"), rows.field("I_N_CONTACTS")), f"step {s}"
        assert np.abs(o_a - o_r).max() <= 2e-4 and np.abs(r_a - r_r).max() <= 2e-5, f"step {s}: {np.abs(o_a - o_r).max():.2e}"
    for s in range(steps, 24):                                          # (contacts begin after a few steps: the two forms must then differ in the last bits)
        o_a = arrow.step(acts[s])[0]; o_r = rows.step(acts[s])[0]
        differ = differ or not np.array_equal(o_a, o_r)
    assert differ, "the switch had no effect: the arrow form was not taken"
