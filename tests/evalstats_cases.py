"""The case table the evaluation statistics' tests share (tests/test_evalstats_ref.py on the host, tests/test_evalstats_gpu.py through the C ABI):
synthetic step sequences in the canonical layout of tests/evalstats_ref.py, and the configurations they run under.

Magnitudes are a walking Go2's: commands within 1 m/s, joint speeds of some 12 rad/s and torques of some 12 N m with tails beyond the limits (30 rad/s,
23.7 N m), foot forces up to 150 N.  Every sequence resets a third of its envs on the very first call."""
import numpy as np

from evalstats_ref import N_LINKS, NDOF

SIZES = (1, 63, 65, 257)                                                    # wave and workgroup edges
BIN_COUNTS = (1, 3, 5)                                                      # 5: bin 3 stays empty

# name -> configuration and sequence; `reset_p` is the per-step reset probability
CASES = {
    "plain": dict(settle_steps=2, max_episodes=3, steps=24, reset_p=0.15, seed=1),
    "settle_zero": dict(settle_steps=0, max_episodes=2, steps=16, reset_p=0.15, seed=2),
    "short_episodes": dict(settle_steps=5, max_episodes=4, steps=24, reset_p=0.30, seed=3),      # most episodes end inside their settle steps
    "one_episode": dict(settle_steps=1, max_episodes=1, steps=20, reset_p=0.20, seed=4),         # what follows the first close is ignored
    "special_values": dict(settle_steps=0, max_episodes=3, steps=14, reset_p=0.10, seed=5, special=True),
}


def bins_for(n, n_bins):
    b = np.arange(n)
    if n_bins == 5:
        return np.array([0, 1, 2, 4], np.int32)[b % 4]
    return (b % n_bins).astype(np.int32)


def sequence(n, steps, seed, reset_p, special=False, **_):
    """-> a list of `steps` input dicts for n envs"""
    rng = np.random.default_rng(1000 * seed + n)
    out = []
    for t in range(steps):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        cf = rng.standard_normal((n, N_LINKS, 3)) * 60.0 * (rng.random((n, N_LINKS, 1)) < 0.5)
        reset = rng.random(n) < reset_p
        if t == 0:
            reset[::3] = True
        x = dict(commands=f32(rng.uniform(-1.0, 1.0, (n, 3))), base_lin_vel=f32(0.5 * rng.standard_normal((n, 3))),
                 base_ang_vel=f32(0.8 * rng.standard_normal((n, 3))), projected_gravity=f32(0.2 * rng.standard_normal((n, 3))),
                 dof_vel=f32(12.0 * rng.standard_normal((n, NDOF))), torque=f32(12.0 * rng.standard_normal((n, NDOF))), cf=f32(cf),
                 reset=reset.astype(np.uint8), time_out=f32(reset & (rng.random(n) < 0.5)))
        if special:
            e = t % n
            kind = t % 7
            if kind == 0:
                x["torque"][e, 3] = np.nan
            elif kind == 1:
                x["torque"][e, 0] = np.inf
            elif kind == 2:
                x["dof_vel"][e, 11] = -np.inf
            elif kind == 3:
                x["dof_vel"][e, 5] = np.nan
            elif kind == 4:
                x["cf"][e, 10] = (np.nan, 1.0, 2.0); x["cf"][e, 12] = (0.0, -np.inf, 0.0)
            elif kind == 5:
                x["base_lin_vel"][e, 0] = np.nan
            else:
                x["torque"][e, 7] = -np.inf; x["dof_vel"][e, 7] = 0.0          # inf * 0: a NaN power next to an infinite peak
            x["reset"][e] = 0                                               # the value is sampled (settle_steps is 0)
            x["time_out"][e] = 0.0
        out.append(x)
    return out


def model_kwargs(case):
    return {k: CASES[case][k] for k in ("settle_steps", "max_episodes")}
