"""The evaluation statistics of include/go2sim_evalstats.h restated in numpy float64: the step's law over all envs at once (`Model.step`), the clear,
and the reduce's lane walk and tree (`Model.reduce`).  Maxima and limits are explicit comparisons (`np.where(x > m, x, m)`), never np.maximum: a NaN
compares false and does not enter.  The float32 pieces (the speed, the foot-force norm) are numpy float32 operations in the header's order.

Inputs of one step, in one canonical layout whatever the device layout under test: a dict of float32 arrays `commands`, `base_lin_vel`,
`base_ang_vel`, `projected_gravity` [n][3], `dof_vel`, `torque` [n][12], `cf` [n][n_links][3] (link 0 is the ground), `reset` uint8 [n], `time_out`
float32 [n]."""
import numpy as np

# the header's indices (tests/test_evalstats_capi.py holds them to the header)
ES = {name: i for i, name in enumerate(("N", "LIN_ERR2", "YAW_ERR2", "VX", "VY", "WZ", "ABS_POWER", "TORQUE2", "TILT2", "SPEED", "PEAK_TORQUE", "PEAK_DOF_VEL",
                                        "PEAK_FOOT_FORCE"))}
EI = {name: i for i, name in enumerate(("EPISODES", "FALLS", "LENGTH_STEPS", "OVER_TORQUE", "OVER_DOF_VEL"))}
M, NSUMS, K, KB, NDOF, LANES = 13, 10, 5, 7, 12, 256
EBIN_ENVS, EBIN_COMPLETE = 5, 6
N_LINKS = 14
FEET = (10, 11, 12, 13)                                                     # the four calf links, the model's numbering
FOOT_MASK = sum(1 << l for l in FEET)


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)                     # the widening is exact


def gt_max(x, m):
    """m = (x > m) ? x : m"""
    with np.errstate(invalid="ignore"):
        return np.where(x > m, x, m)


def norm32(F):
    F = np.asarray(F, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((F[..., 0] * F[..., 0] + F[..., 1] * F[..., 1]) + F[..., 2] * F[..., 2]).astype(np.float32)


class Model:
    def __init__(self, n_envs, n_bins=1, bins=None, settle_steps=0, max_episodes=1, torque_limit=23.7, dof_vel_limit=30.0, foot_links=FEET):
        self.n, self.n_bins = int(n_envs), int(n_bins)
        self.bins = np.zeros(self.n, np.int32) if bins is None else np.asarray(bins, np.int32).copy()
        self.settle_steps, self.max_episodes = int(settle_steps), int(max_episodes)
        self.torque_limit, self.dof_vel_limit, self.foot_links = float(torque_limit), float(dof_vel_limit), tuple(sorted(foot_links))
        self.run_f, self.tot_f = np.zeros((M, self.n)), np.zeros((M, self.n))
        self.run_i, self.tot_i = np.zeros((K, self.n), np.int32), np.zeros((K, self.n), np.int32)
        self.bin_f, self.bin_i = np.zeros((self.n_bins, M)), np.zeros((self.n_bins, KB), np.int64)

    def state(self):
        return self.run_f, self.run_i, self.tot_f, self.tot_i, self.bin_f, self.bin_i

    def step(self, x):
        active = self.tot_i[EI["EPISODES"]] < self.max_episodes
        reset = np.asarray(x["reset"]) != 0
        close, live = active & reset, active & ~reset
        with np.errstate(invalid="ignore", over="ignore"):
            # the episode closes
            for q in range(M):
                merged = self.tot_f[q] + self.run_f[q] if q < NSUMS else gt_max(self.run_f[q], self.tot_f[q])
                self.tot_f[q] = np.where(close, merged, self.tot_f[q])
                self.run_f[q] = np.where(close, 0.0, self.run_f[q])
            self.tot_i[EI["EPISODES"]] += close
            self.tot_i[EI["FALLS"]] += close & (np.asarray(x["time_out"], np.float32) == 0)
            for q in range(EI["LENGTH_STEPS"], K):
                self.tot_i[q] += np.where(close, self.run_i[q], 0)
                self.run_i[q] = np.where(close, 0, self.run_i[q])
            # a step of the episode
            k = self.run_i[EI["LENGTH_STEPS"]].copy()
            self.run_i[EI["LENGTH_STEPS"]] += live
            sample = live & (k >= self.settle_steps)
            c, v, w, g = f64(x["commands"]), f64(x["base_lin_vel"]), f64(x["base_ang_vel"]), f64(x["projected_gravity"])
            tau, qd = f64(x["torque"]), f64(x["dof_vel"])
            ex, ey, ew = c[:, 0] - v[:, 0], c[:, 1] - v[:, 1], c[:, 2] - w[:, 2]
            power, tau2 = np.zeros(self.n), np.zeros(self.n)
            peak_tau, peak_qd = self.run_f[ES["PEAK_TORQUE"]].copy(), self.run_f[ES["PEAK_DOF_VEL"]].copy()
            over_tau, over_qd = np.zeros(self.n, bool), np.zeros(self.n, bool)
            for j in range(NDOF):
                atau, aqd = np.abs(tau[:, j]), np.abs(qd[:, j])
                power = power + np.abs(tau[:, j] * qd[:, j])
                tau2 = tau2 + tau[:, j] * tau[:, j]
                peak_tau, peak_qd = gt_max(atau, peak_tau), gt_max(aqd, peak_qd)
                over_tau, over_qd = over_tau | (atau > self.torque_limit), over_qd | (aqd > self.dof_vel_limit)
            peak_foot = self.run_f[ES["PEAK_FOOT_FORCE"]].copy()
            for l in self.foot_links:
                peak_foot = gt_max(norm32(np.asarray(x["cf"], np.float32)[:, l]).astype(np.float64), peak_foot)
            v32 = np.asarray(x["base_lin_vel"], np.float32)
            speed = np.sqrt(v32[:, 0] * v32[:, 0] + v32[:, 1] * v32[:, 1]).astype(np.float32).astype(np.float64)
            add = [np.ones(self.n), ex * ex + ey * ey, ew * ew, v[:, 0], v[:, 1], w[:, 2], power, tau2, g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1], speed]
            for q in range(NSUMS):
                self.run_f[q] = np.where(sample, self.run_f[q] + add[q], self.run_f[q])
            for q, peak in ((ES["PEAK_TORQUE"], peak_tau), (ES["PEAK_DOF_VEL"], peak_qd), (ES["PEAK_FOOT_FORCE"], peak_foot)):
                self.run_f[q] = np.where(sample, peak, self.run_f[q])
            self.run_i[EI["OVER_TORQUE"]] += sample & over_tau
            self.run_i[EI["OVER_DOF_VEL"]] += sample & over_qd

    def clear(self, idx=None):
        idx = np.arange(self.n) if idx is None else np.asarray([b for b in idx if 0 <= b < self.n], np.int64)
        for a in (self.run_f, self.tot_f, self.run_i, self.tot_i):
            a[:, idx] = 0

    def _walk_and_tree(self, x, k, op, dtype):
        p = np.zeros(LANES, dtype)
        for start in range(0, self.n, LANES):                               # lane i takes the envs i, i + 256, .. ascending
            e = np.arange(start, min(start + LANES, self.n))
            mine = self.bins[e] == k
            p[:len(e)] = np.where(mine, op(p[:len(e)], x[e]), p[:len(e)])
        stride = LANES // 2
        while stride >= 1:
            p[:stride] = op(p[:stride], p[stride:2 * stride])
            stride //= 2
        return p[0]

    def reduce(self):
        add = lambda a, b: a + b
        larger = lambda a, b: gt_max(b, a)                                  # (b > a) ? b : a
        complete = (self.tot_i[EI["EPISODES"]] >= self.max_episodes).astype(np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(self.n_bins):
                for q in range(M):
                    self.bin_f[k, q] = self._walk_and_tree(self.tot_f[q], k, add if q < NSUMS else larger, np.float64)
                for q in range(K):
                    self.bin_i[k, q] = self._walk_and_tree(self.tot_i[q].astype(np.int64), k, add, np.int64)
                self.bin_i[k, EBIN_ENVS] = self._walk_and_tree(np.ones(self.n, np.int64), k, add, np.int64)
                self.bin_i[k, EBIN_COMPLETE] = self._walk_and_tree(complete, k, add, np.int64)
        return self.bin_f, self.bin_i


def same_f64(got, want):
    """bit-equal, a NaN matching any NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def same_state(got, want):
    """-> the names of the arrays of two (run_f, run_i, tot_f, tot_i, bin_f, bin_i) states that differ"""
    names = ("run_f", "run_i", "tot_f", "tot_i", "bin_f", "bin_i")
    return [n for n, g, w in zip(names, got, want)
            if not (same_f64(g, w) if n.endswith("_f") else (np.asarray(g).shape == np.asarray(w).shape and np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64))))]
