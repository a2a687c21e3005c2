"""The evaluation statistics (include/go2sim_evalstats.h) without a GPU: the numpy restatement tests/evalstats_ref.py against a plain per-env Python
loop that follows the header line by line (Python floats are IEEE float64, the float32 pieces go through numpy float32 scalars), on the shared case
table, bit for bit; the reduce's tree against a hand evaluation; the derived metrics (evaluation.bin_metrics) on cases computed by hand."""
import math

import numpy as np
import pytest

import evalstats_cases as T
import evalstats_ref as R
from go2_sim2real_locomotion_rl_amd.capi import C
from go2_sim2real_locomotion_rl_amd.evaluation import METRICS, bin_metrics, robot_weight

ES, EI = R.ES, R.EI


class EnvLoop:
    """one env, the header's law statement by statement"""

    def __init__(self, settle_steps, max_episodes, torque_limit=23.7, dof_vel_limit=30.0, feet=R.FEET):
        self.settle, self.max_ep, self.tl, self.vl, self.feet = settle_steps, max_episodes, torque_limit, dof_vel_limit, feet
        self.run_f, self.tot_f, self.run_i, self.tot_i = [0.0] * R.M, [0.0] * R.M, [0] * R.K, [0] * R.K

    def step(self, x, b):
        if self.tot_i[EI["EPISODES"]] >= self.max_ep:
            return
        if x["reset"][b]:
            for q in range(R.M):
                r, t = self.run_f[q], self.tot_f[q]
                self.tot_f[q] = t + r if q < R.NSUMS else (r if r > t else t)
                self.run_f[q] = 0.0
            self.tot_i[EI["EPISODES"]] += 1
            self.tot_i[EI["FALLS"]] += 1 if x["time_out"][b] == 0 else 0
            for q in range(EI["LENGTH_STEPS"], R.K):
                self.tot_i[q] += self.run_i[q]
                self.run_i[q] = 0
            return
        k = self.run_i[EI["LENGTH_STEPS"]]
        self.run_i[EI["LENGTH_STEPS"]] = k + 1
        if k < self.settle:
            return
        f = lambda name, i: float(x[name][b, i])                            # float32 -> float64, exact
        cx, cy, cyaw, vx, vy, wz = f("commands", 0), f("commands", 1), f("commands", 2), f("base_lin_vel", 0), f("base_lin_vel", 1), f("base_ang_vel", 2)
        gx, gy = f("projected_gravity", 0), f("projected_gravity", 1)
        power = tau2 = 0.0
        over_t = over_v = False
        for j in range(R.NDOF):
            tau, qd = f("torque", j), f("dof_vel", j)
            power = power + abs(tau * qd)
            tau2 = tau2 + tau * tau
            if abs(tau) > self.run_f[ES["PEAK_TORQUE"]]:
                self.run_f[ES["PEAK_TORQUE"]] = abs(tau)
            if abs(qd) > self.run_f[ES["PEAK_DOF_VEL"]]:
                self.run_f[ES["PEAK_DOF_VEL"]] = abs(qd)
            over_t, over_v = over_t or abs(tau) > self.tl, over_v or abs(qd) > self.vl
        with np.errstate(invalid="ignore", over="ignore"):
            for l in self.feet:
                fx, fy, fz = x["cf"][b, l]                                  # numpy float32 scalars: every operation rounds to float32
                n = float(np.sqrt((fx * fx + fy * fy) + fz * fz))
                if n > self.run_f[ES["PEAK_FOOT_FORCE"]]:
                    self.run_f[ES["PEAK_FOOT_FORCE"]] = n
            v0, v1 = x["base_lin_vel"][b, 0], x["base_lin_vel"][b, 1]
            speed = float(np.sqrt(v0 * v0 + v1 * v1))
        ex, ey, ew = cx - vx, cy - vy, cyaw - wz
        add = {"N": 1.0, "LIN_ERR2": ex * ex + ey * ey, "YAW_ERR2": ew * ew, "VX": vx, "VY": vy, "WZ": wz, "ABS_POWER": power, "TORQUE2": tau2,
               "TILT2": gx * gx + gy * gy, "SPEED": speed}
        for name, v in add.items():
            self.run_f[ES[name]] = self.run_f[ES[name]] + v
        self.run_i[EI["OVER_TORQUE"]] += int(over_t)
        self.run_i[EI["OVER_DOF_VEL"]] += int(over_v)


def test_indices_are_the_headers():
    assert all(C["GO2SIM_ES_" + k] == v for k, v in ES.items()) and all(C["GO2SIM_EI_" + k] == v for k, v in EI.items())
    assert (C["GO2SIM_ES_M"], C["GO2SIM_ES_NSUMS"], C["GO2SIM_EI_K"], C["GO2SIM_EBIN_K"]) == (R.M, R.NSUMS, R.K, R.KB)
    assert (C["GO2SIM_EBIN_ENVS"], C["GO2SIM_EBIN_COMPLETE"], C["GO2SIM_EVALSTATS_NDOF"], C["GO2SIM_NL"]) == (R.EBIN_ENVS, R.EBIN_COMPLETE, R.NDOF, R.N_LINKS)


@pytest.mark.parametrize("case", sorted(T.CASES))
def test_restatement_is_the_per_env_loop(case):
    n = 65
    seq = T.sequence(n, **T.CASES[case])
    model = R.Model(n, **T.model_kwargs(case))
    loops = [EnvLoop(**T.model_kwargs(case)) for _ in range(n)]
    for t, x in enumerate(seq):
        model.step(x)
        for b, loop in enumerate(loops):
            loop.step(x, b)
        want = (np.array([l.run_f for l in loops]).T, np.array([l.run_i for l in loops]).T, np.array([l.tot_f for l in loops]).T,
                np.array([l.tot_i for l in loops]).T)
        assert not R.same_state(model.state()[:4], want), (case, t)
    # the table does what its rows' names say
    ep, n_s = model.tot_i[EI["EPISODES"]], model.tot_f[ES["N"]]
    assert ep.max() == T.CASES[case]["max_episodes"] and ep[0] >= 1 and model.tot_i[EI["FALLS"]].sum() > 0
    assert (model.tot_i[EI["FALLS"]] < ep).any()                            # time-outs next to falls
    if case == "short_episodes":
        assert ((ep > 0) & (n_s == 0)).any()                                # closed episodes without one sample
    if case == "one_episode":
        assert (ep == 1).sum() > n // 2 and not model.run_i[:, ep == 1].any()       # ignored after the first close
    if case == "special_values":
        f = model.tot_f + model.run_f
        assert np.isnan(f[ES["ABS_POWER"]]).any() and np.isinf(f[ES["TORQUE2"]]).any() and np.isnan(f[ES["VX"]]).any()
        peaks = np.concatenate([model.tot_f[R.NSUMS:], model.run_f[R.NSUMS:]])
        assert not np.isnan(peaks).any() and np.isinf(peaks).any()            # a NaN never enters a maximum, an infinity does
    else:
        assert model.tot_i[EI["OVER_TORQUE"]].sum() > 0 and model.tot_i[EI["OVER_DOF_VEL"]].sum() > 0


def test_reduce_is_the_lane_walk_and_the_tree():
    n, n_bins = 600, 3
    rng = np.random.default_rng(0)
    model = R.Model(n, n_bins=n_bins, bins=np.arange(n) % 2, max_episodes=2)     # bin 2 is empty
    model.tot_f[:] = rng.standard_normal((R.M, n)) * 10.0 ** rng.integers(-8, 8, (R.M, n))
    model.tot_f[R.NSUMS:] = np.abs(model.tot_f[R.NSUMS:])
    model.tot_i[:] = rng.integers(0, 5, (R.K, n))
    bin_f, bin_i = model.reduce()
    for k in range(2):
        for q in (0, 4, ES["PEAK_DOF_VEL"]):
            lanes = []
            for i in range(256):
                p = 0.0
                for e in range(i, n, 256):
                    if e % 2 == k:
                        x = float(model.tot_f[q, e])
                        p = p + x if q < R.NSUMS else (x if x > p else p)
                lanes.append(p)
            s = 128
            while s >= 1:
                lanes = [(lanes[i] + lanes[i + s] if q < R.NSUMS else max(lanes[i], lanes[i + s])) for i in range(s)]
                s //= 2
            assert bin_f[k, q] == lanes[0]
        assert bin_i[k, :R.K].tolist() == model.tot_i[:, k::2].astype(np.int64).sum(1).tolist()
        assert bin_i[k, R.EBIN_ENVS] == 300 and bin_i[k, R.EBIN_COMPLETE] == (model.tot_i[0, k::2] >= 2).sum()
    assert not bin_f[2].any() and not bin_i[2].any()
    assert bin_f[0, ES["PEAK_TORQUE"]] == model.tot_f[ES["PEAK_TORQUE"], 0::2].max()


def test_clear_of_a_subset():
    n = 9
    model = R.Model(n, settle_steps=0, max_episodes=2)
    for x in T.sequence(n, 6, 7, 0.3):
        model.step(x)
    before = [a.copy() for a in model.state()[:4]]
    model.clear([2, 5, -1, n])
    for a, b in zip(model.state()[:4], before):
        assert not a[:, [2, 5]].any() and np.array_equal(np.delete(a, [2, 5], 1), np.delete(b, [2, 5], 1), equal_nan=True)


# ---- the derived metrics on hand-computed cases ---------------------------------------------------------------------------------------------
def constant_inputs(n, cmd, vel, wz, tau, qd, reset, time_out):
    z = np.zeros((n, 3), np.float32)
    cf = np.zeros((n, R.N_LINKS, 3), np.float32)
    cf[:, 10] = (0.0, 3.0, 4.0)                                             # a foot force of 5 N
    return dict(commands=z + np.float32(cmd), base_lin_vel=z + np.float32(vel), base_ang_vel=z + np.float32([0.0, 0.0, wz]),
                projected_gravity=z + np.float32([0.25, 0.0, -1.0]), dof_vel=np.full((n, 12), qd, np.float32), torque=np.full((n, 12), tau, np.float32), cf=cf,
                reset=np.full(n, reset, np.uint8), time_out=np.full(n, time_out, np.float32))


def test_constant_command_and_velocity():
    """8 envs, settle 2: every episode is 10 steps of command (1, 0, 0.5) at velocity (0.5, 0.25, .) and yaw rate 0.5, torque 2 N m at 4 rad/s on every
    joint, then a time-out; two episodes each.  All values are dyadic: the sums are exact and the metrics known in closed form."""
    n, dt = 8, 0.02
    model = R.Model(n, settle_steps=2, max_episodes=2)
    for _ in range(2):
        for _ in range(10):
            model.step(constant_inputs(n, (1.0, 0.0, 0.5), (0.5, 0.25, 0.0), 0.5, 2.0, 4.0, 0, 0.0))
        model.step(constant_inputs(n, (1.0, 0.0, 0.5), (0.5, 0.25, 0.0), 0.5, 2.0, 4.0, 1, 1.0))
    model.step(constant_inputs(n, (1.0, 0.0, 0.5), (9.0, 9.0, 0.0), 9.0, 99.0, 99.0, 0, 0.0))       # ignored: both episodes are closed
    bin_f, bin_i = model.reduce()
    mass, g = robot_weight()
    m = bin_metrics(bin_f[0], bin_i[0], dt, mass, g)
    assert set(METRICS) <= set(m)
    samples = n * 2 * 8                                                     # ten steps less the two settle steps
    assert (m["episodes"], m["falls"], m["fall_rate"], m["n_samples"], m["complete"], m["envs"]) == (16, 0, 0.0, samples, True, n)
    assert abs(m["mean_episode_s"] - 10 * dt) < 1e-12
    assert m["lin_vel_rmse"] == math.sqrt(0.25 + 0.0625) and m["yaw_rate_rmse"] == 0.0
    assert (m["mean_vx"], m["mean_vy"], m["mean_wz"]) == (0.5, 0.25, 0.5)
    assert m["mean_abs_power_W"] == 12 * 8.0 and m["torque_rms"] == 2.0 and (m["peak_torque"], m["peak_dof_vel"], m["peak_foot_force"]) == (2.0, 4.0, 5.0)
    assert m["frac_steps_over_torque"] == 0.0 and m["frac_steps_over_dof_vel"] == 0.0 and m["tilt_rms"] == 0.25
    speed = float(np.sqrt(np.float32(0.5 * 0.5 + 0.25 * 0.25)))
    assert m["cost_of_transport"] == (96.0 * samples) / (mass * g * (bin_f[0][ES["SPEED"]])) and abs(bin_f[0][ES["SPEED"]] - samples * speed) < 1e-9
    assert abs(mass - 15.019) < 1e-9 and g == 9.81
    assert abs(m["cost_of_transport"] - 96.0 / (15.019 * 9.81 * math.sqrt(0.3125))) < 1e-6


def test_a_single_fall_and_the_limits():
    """4 envs in two bins; env 0 falls after 5 steps (torque 30 N m: over the limit on each of its 4 samples), the others run on"""
    n = 4
    model = R.Model(n, n_bins=2, bins=[0, 1, 1, 1], settle_steps=1, max_episodes=1)
    for _ in range(5):
        x = constant_inputs(n, (0.5, 0.0, 0.0), (0.5, 0.0, 0.0), 0.0, 2.0, 4.0, 0, 0.0)
        x["torque"][0] = 30.0
        x["dof_vel"][0, 3] = -31.0
        model.step(x)
    x = constant_inputs(n, (0.5, 0.0, 0.0), (0.5, 0.0, 0.0), 0.0, 2.0, 4.0, 0, 0.0)
    x["reset"][0] = 1
    model.step(x)
    bin_f, bin_i = model.reduce()
    fell, rest = (bin_metrics(bin_f[k], bin_i[k], 0.02, 15.0, 10.0) for k in range(2))
    assert (fell["episodes"], fell["falls"], fell["fall_rate"], fell["n_samples"], fell["complete"]) == (1, 1, 1.0, 4, True)
    assert fell["mean_episode_s"] == 5 * 0.02 and fell["lin_vel_rmse"] == 0.0 and fell["peak_torque"] == 30.0 and fell["peak_dof_vel"] == 31.0
    assert fell["frac_steps_over_torque"] == 1.0 and fell["frac_steps_over_dof_vel"] == 1.0
    assert fell["cost_of_transport"] == (4 * (11 * 120.0 + 930.0)) / (15.0 * 10.0 * 4 * 0.5)
    # nothing closed in the other bin: no totals, ratios undefined, not complete
    assert (rest["episodes"], rest["falls"], rest["n_samples"], rest["complete"], rest["envs"]) == (0, 0, 0, False, 3)
    assert rest["fall_rate"] is None and rest["lin_vel_rmse"] is None and rest["cost_of_transport"] is None and rest["peak_torque"] == 0.0
    assert model.run_f[ES["N"], 1] == 5.0                                   # the running record is not reported before its episode closes
