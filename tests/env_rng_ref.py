"""The stream map of the library's random draws (include/go2sim_rng.h) and its numpy restatement.

STREAMS has one row per drawn quantity: which purpose, which env word, which key, which block and which word(s) of Philox4x32-10 feed it, and through
which transform.  The functions below restate the transforms and the laws built on them (rand_float, rand_int, _lerp_range, the command law, the mix
branch of sample_level, the terrain-row assignment) on the words of tests/policy_ref.py::philox4x32.  It imports nothing of the project but those
words, like tests/tiles_ref.py and tests/wells_ref.py; tests/env_rng_cases.py drives the oracle builds (tests/test_env_rng_ref.py) and the HIP
library (tests/test_env_rng_gpu.py) through it.

Compared to the bit: everything whose transform is rand_float, rand_int or a comparison (every op is one IEEE binary32 or binary64 operation here as
in the library).  Compared within a bound: what passes through dm_normal2 or dm_sincos, against float64.  The two bounds are 4 x the worst deviation
measured on the CPU build of include/go2sim_detmath.h, rounded up to one digit (tests/test_env_rng_ref.py measures them again and holds them):

    dm_normal2 against float64 Box-Muller, 2^16 Philox blocks (purpose 1, seeds 5 and 0x300000005):  worst 1.68e-6  ->  NORMAL_ABS = 7e-6
    euler_to_quat_wxyz (roll, pitch in +-5 deg, yaw 0) against float64, 2^16 pairs:                   worst 8.7e-8   ->  QUAT_ABS   = 4e-7

A wrong word moves a normal by O(1) and a quaternion component by O(0.04), so either bound separates."""
import collections
import math

import numpy as np

import policy_ref as PR

F = np.float32
U24 = 2.0 ** -24
NORMAL_ABS = 7e-6
QUAT_ABS = 4e-7

# the purposes, restated (tests/test_env_rng_ref.py compares them with capi.C, which reads include/go2sim_rng.h and the sensors' headers)
PURPOSE = dict(ACTION_NOISE=1, PUSH=2, CMD=3, OBS_NOISE=4, RESET_DR=5, GLOBAL_DR=6, RESET_CMD=7, RESET_POSE=8, TERRAIN_ROW=9, TERRAIN_PERM=10,
               POLICY_NOISE=11, LIDAR=12, STAIRINFO=13, TILES=14, WELLS=15, RESET_KPKD=16)
ENV_PURPOSES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)          # the streams both the oracle and the HIP library have
GLOBAL_ENV_WORD = 0xFFFFFFFF
NOBS_MAX, NACT_MAX, LIDAR_MAX = 64, 32, 64              # how far the open-ended rows below are enumerated for the distinctness check

Row = collections.namedtuple("Row", "name quantity purpose env key cells transform")
# env: "env" the env index | "global" 0xffffffff | "rank" the shuffle rank p | "row" the policy's batch row
# key: "step" | "reset" | "reset|sync" | "policy_step" | "scan_step"
# cells: the (block, word) pairs the quantity reads


def _cells(blocks, words):
    return tuple((b, w) for b in blocks for w in words)


def _rows():
    P = PURPOSE
    R = []

    def add(name, purpose, env, key, cells, transform, quantity=None):
        R.append(Row(name, quantity or name, purpose, env, key, tuple(cells), transform))

    add("action_noise", P["ACTION_NOISE"], "env", "step", _cells(range(3), range(4)), "normal")          # motor 4 blk + k: normal k of block blk
    add("push.fx", P["PUSH"], "env", "step", [(0, 0)], "rand_float")
    add("push.fy", P["PUSH"], "env", "step", [(0, 1)], "rand_float")
    add("push.duration", P["PUSH"], "env", "step", [(0, 2)], "rand_int")
    for k, n in enumerate(("x", "y", "yaw")):
        add("cmd." + n, P["CMD"], "env", "step", [(0, k)], "rand_float")
    add("cmd.axis", P["CMD"], "env", "step", [(0, 3)], "rand_int")
    add("obs_noise", P["OBS_NOISE"], "env", "step", _cells(range(NOBS_MAX // 4), range(4)), "normal")    # observation i: normal i % 4 of block i / 4
    add("reset.kp_factors", P["RESET_DR"], "env", "reset", _cells(range(0, 3), range(4)), "rand_float")
    add("reset.kd_factors", P["RESET_DR"], "env", "reset", _cells(range(3, 6), range(4)), "rand_float")
    add("reset.gravity_offset", P["RESET_DR"], "env", "reset", _cells([6], range(3)), "rand_float")
    add("reset.motor_strength", P["RESET_DR"], "env", "reset", _cells(range(7, 10), range(4)), "rand_float")
    add("reset.env_friction", P["RESET_DR"], "env", "reset", [(10, 0)], "rand_float")
    add("reset.env_mass", P["RESET_DR"], "env", "reset", [(10, 1)], "rand_float")
    add("global.mix_decision", P["GLOBAL_DR"], "global", "reset|sync", [(0, 0)], "compare")
    add("global.mix_level", P["GLOBAL_DR"], "global", "reset|sync", [(0, 1)], "u01")
    add("global.friction", P["GLOBAL_DR"], "global", "reset|sync", [(0, 2)], "rand_float")
    add("global.mass", P["GLOBAL_DR"], "global", "reset|sync", [(0, 3)], "rand_float")
    add("global.com", P["GLOBAL_DR"], "global", "reset|sync", _cells([1], range(3)), "rand_float")
    add("global.leg_mass", P["GLOBAL_DR"], "global", "reset|sync", _cells([2], range(4)), "rand_float")
    for k, n in enumerate(("x", "y", "yaw")):
        add("reset_cmd." + n, P["RESET_CMD"], "env", "reset", [(0, k)], "rand_float")
    add("reset_cmd.axis", P["RESET_CMD"], "env", "reset", [(0, 3)], "rand_int")
    add("pose.z", P["RESET_POSE"], "env", "reset", [(0, 0)], "rand_float")
    add("pose.roll", P["RESET_POSE"], "env", "reset", [(0, 1)], "rand_float")
    add("pose.pitch", P["RESET_POSE"], "env", "reset", [(0, 2)], "rand_float")
    add("pose.delay", P["RESET_POSE"], "env", "reset", [(0, 3)], "rand_int")
    add("terrain.near_row", P["TERRAIN_ROW"], "rank", "reset", [(0, 0)], "rand_int")
    add("terrain.easy_row", P["TERRAIN_ROW"], "rank", "reset", [(0, 1)], "rand_int")
    add("terrain.perm", P["TERRAIN_PERM"], "env", "reset", [(0, 0)], "rank")
    add("kpkd.kp", P["RESET_KPKD"], "env", "reset", [(0, 0)], "rand_float")
    add("kpkd.kd", P["RESET_KPKD"], "env", "reset", [(0, 1)], "rand_float")
    # ---- the streams of the other references, copied so that the distinctness check covers them
    add("policy.noise", P["POLICY_NOISE"], "row", "policy_step", _cells(range(NACT_MAX // 4), range(4)), "normal")      # policy_ref.noise64
    add("lidar.latency", P["LIDAR"], "env", "scan_step", [(0, 0)], "u01")                                               # lidar_ref.draws
    add("lidar.blackout", P["LIDAR"], "env", "scan_step", [(0, 1)], "u01")
    add("lidar.offset", P["LIDAR"], "env", "scan_step", _cells([0], (2, 3)), "normal")
    add("lidar.ray_noise", P["LIDAR"], "env", "scan_step", _cells(range(1, 1 + LIDAR_MAX // 2), (0, 1)), "normal")      # rays 2 (blk - 1), 2 (blk - 1) + 1
    add("lidar.ray_dropout", P["LIDAR"], "env", "scan_step", _cells(range(1, 1 + LIDAR_MAX // 2), (2, 3)), "u01")
    add("stairinfo.edge_height", P["STAIRINFO"], "env", "scan_step", _cells([0], (0, 1)), "normal")                     # stairinfo_ref.draws
    add("stairinfo.depth", P["STAIRINFO"], "env", "scan_step", _cells([0], (2, 3)), "normal")
    add("stairinfo.flip", P["STAIRINFO"], "env", "scan_step", [(1, 0)], "u01")
    add("stairinfo.latency", P["STAIRINFO"], "env", "scan_step", [(1, 1)], "u01")
    add("stairinfo.blackout", P["STAIRINFO"], "env", "scan_step", [(1, 2)], "u01")
    add("tiles.row", P["TILES"], "env", "reset", [(0, 0)], "mod")                                                       # tiles_ref.spawn
    add("tiles.col", P["TILES"], "env", "reset", [(0, 1)], "mod")
    add("tiles.jitter_x", P["TILES"], "env", "reset", [(0, 2)], "u01")
    add("tiles.jitter_y", P["TILES"], "env", "reset", [(0, 3)], "u01")
    add("wells.x", P["WELLS"], "env", "reset", [(0, 0)], "u01")                                                         # wells_ref.spawn
    add("wells.y", P["WELLS"], "env", "reset", [(0, 1)], "u01")
    add("wells.yaw", P["WELLS"], "env", "reset", [(0, 2)], "rand_float")
    # the well spawn forms roll and pitch a second time from their words of the pose block: the same quantities, declared as such
    add("wells.roll", P["RESET_POSE"], "env", "reset", [(0, 1)], "rand_float", quantity="pose.roll")
    add("wells.pitch", P["RESET_POSE"], "env", "reset", [(0, 2)], "rand_float", quantity="pose.pitch")
    return R


STREAMS = _rows()
ROWS = {r.name: r for r in STREAMS}


def clashes(streams=STREAMS):
    """Pairs of rows that hold different quantities and read one (purpose, block, word): [(row a, row b, (purpose, block, word))], each pair once."""
    seen, out, told = {}, [], set()
    for r in streams:
        for cell in r.cells:
            k = (r.purpose,) + cell
            o = seen.setdefault(k, r)
            if o.quantity != r.quantity and (o.name, r.name) not in told:
                told.add((o.name, r.name))
                out.append((o.name, r.name, k))
    return out


def mixed_kinds(streams=STREAMS):
    """Purposes whose rows do not agree on the key kind or on the env-word kind: {purpose: (set of keys, set of env words)}"""
    kinds = collections.defaultdict(lambda: (set(), set()))
    for r in streams:
        kinds[r.purpose][0].add(r.key); kinds[r.purpose][1].add(r.env)
    return {p: k for p, k in kinds.items() if len(k[0]) != 1 or len(k[1]) != 1}


# ---- words and transforms -----------------------------------------------------------------------------------------------------------------------
def words(seed, purpose, env, key, block):
    """uint32 [..., 4]: dm_philox(env, key, purpose, block; low word of the seed, high word), broadcast over env / key / block"""
    r = PR.philox4x32(np.asarray(env, np.uint64), np.asarray(key, np.uint64), np.uint64(purpose), np.asarray(block, np.uint64),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([np.asarray(w, np.uint64).astype(np.uint32) for w in r], axis=-1)


def u01(w):
    """dm_u01: the top 24 bits, exact in float32"""
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(F) * F(U24)


def rand_float(lo, hi, w):
    """gs_rand_float with python-float bounds: f32(hi - lo) * u + f32(lo), the difference formed in float64"""
    return (F(float(hi) - float(lo)) * u01(w) + F(float(lo))).astype(F)


def rand_int(lo, hi, w):
    return (int(lo) + (np.asarray(w, np.uint32).astype(np.int64) % (int(hi) - int(lo) + 1))).astype(np.int32)


def normals(w):
    """float64 [..., 4]: the two Box-Muller pairs (w0, w1), (w2, w3) of blocks w [..., 4]"""
    w = np.asarray(w, np.uint64)
    a, b = PR.box_muller(w[..., 0], w[..., 1])
    c, d = PR.box_muller(w[..., 2], w[..., 3])
    return np.stack([a, b, c, d], axis=-1)


def clamp01(x):
    return max(0.0, min(1.0, float(x)))


def lerp(a, b, t):
    return float(a) + (float(b) - float(a)) * clamp01(t)


def lerp_range(rng, t):
    """_lerp_range(easy, hard, t_sample) in float64; rng = ((easy lo, easy hi), (hard lo, hard hi)) -> (lo, hi)"""
    (elo, ehi), (hlo, hhi) = rng
    return lerp(elo, hlo, t), lerp(ehi, hhi, t)


# ---- the laws -------------------------------------------------------------------------------------------------------------------------------------
def sample_level(level, curr, w):
    """CurriculumManager.sample_level on block 0 of the global stream: (t_sample, took the mix branch).  curr: enabled, mix_prob_current,
    mix_level_low, mix_level_high.  The decision compares two float32 (u01 and the probability as the library stores it)."""
    if not curr["enabled"]:
        return 1.0, None
    if u01(w[0]) < F(curr["mix_prob_current"]):
        return clamp01(level), False
    hi = min(float(level), float(curr["mix_level_high"]))
    lo = min(float(curr["mix_level_low"]), hi)
    return clamp01(lo + (hi - lo) * float(u01(w[1]))), True


def commands(w, ranges, compound, envs, n_standing):
    """_resample_commands on blocks w [n][4] of envs `envs`: float32 [n][3].  ranges: ((x lo, hi), (y lo, hi), (yaw lo, hi)), the current ones."""
    w = np.asarray(w, np.uint32)
    cmd = np.stack([rand_float(ranges[k][0], ranges[k][1], w[:, k]) for k in range(3)], axis=1)
    if not compound:
        choice = rand_int(0, 2, w[:, 3])
        cmd = np.where(np.arange(3)[None, :] == choice[:, None], cmd, F(0)).astype(F)
    cmd[np.asarray(envs) < n_standing] = F(0)
    return cmd


def terrain_ranks(seed, envs, reset_call):
    """The shuffle of the reset envs `envs` (ascending): rank of each = number of reset envs with a smaller purpose-10 key, ties by env index."""
    key = words(seed, PURPOSE["TERRAIN_PERM"], envs, reset_call, 0)[:, 0].astype(np.int64)
    order = np.lexsort((np.arange(len(envs)), key))
    rank = np.empty(len(envs), np.int64)
    rank[order] = np.arange(len(envs))
    return rank


def terrain_rows(seed, envs, reset_call, max_row):
    """_assign_terrain_rows: 40 % of the reset envs (by rank) on max_row, 30 % one or two rows below, the rest on the easy rows -> (rows, class
    0 frontier / 1 near / 2 easy)"""
    n = len(envs)
    rank = terrain_ranks(seed, envs, reset_call)
    n_frontier, n_near = int(n * 0.40), int(n * 0.30)
    w = words(seed, PURPOSE["TERRAIN_ROW"], rank, reset_call, 0)
    near = rand_int(max(0, max_row - 2), max(0, max_row - 1), w[:, 0]) if max_row >= 2 else np.full(n, max_row, np.int32)
    easy = rand_int(0, max_row - 3 if max_row >= 3 else 0, w[:, 1])
    cls = np.where(rank < n_frontier, 0, np.where(rank < n_frontier + n_near, 1, 2))
    return np.where(cls == 0, max_row, np.where(cls == 1, near, easy)).astype(np.int32), cls


def quat64(roll, pitch, yaw=0.0):
    """euler_to_quat_wxyz in float64 of float32 angles: [n][4]"""
    r, p, y = (np.asarray(v, np.float64) / 2.0 for v in (roll, pitch, np.broadcast_to(yaw, np.shape(roll))))
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=-1)


class Draws:
    """Every draw of one handle, by stream.  P holds plain python values:
      seed; ranges: name -> ((easy lo, hi), (hard lo, hi)) for friction, kpf, kdf, kpr, kdr, mass, com, legm, goff, mstr; has: name -> bool;
      curr (sample_level); init_z (lo, hi); init_euler_deg (lo, hi); min_delay, max_delay; push_dur (lo, hi) in steps; compound; n_standing;
      friction_interval (the throttle of the global friction draw)"""

    def __init__(self, P):
        self.P, self.seed = P, P["seed"]
        self.friction_counter = 0

    def w(self, purpose, env, key, block):
        return words(self.seed, PURPOSE[purpose], env, key, block)

    # -- purpose 6
    def global_dr(self, key, level, n_throttle, first_sync=False):
        """The global draws of reset call (or sync call) `key`: dict t_sample, mixed, friction (None when the throttle holds it back), mass, com,
        leg_mass.  `n_throttle` reset envs are counted for the friction throttle."""
        P = self.P
        w = self.w("GLOBAL_DR", GLOBAL_ENV_WORD, key, np.arange(3))
        ts, mixed = sample_level(level, P["curr"], w[0])
        out = {"t_sample": ts, "mixed": mixed, "friction": None}
        if P["has"]["friction"]:
            self.friction_counter += n_throttle
            if self.friction_counter >= P["friction_interval"]:
                self.friction_counter = 0
                out["friction"] = rand_float(*lerp_range(P["ranges"]["friction"], ts), w[0, 2])
        out["mass"] = rand_float(*lerp_range(P["ranges"]["mass"], ts), w[0, 3])
        out["com"] = rand_float(*lerp_range(P["ranges"]["com"], ts), w[1, :3])
        out["leg_mass"] = rand_float(*lerp_range(P["ranges"]["legm"], ts), w[2, :4])
        return out

    # -- purpose 5
    def reset_dr(self, envs, rc, ts):
        """kp_factors, kd_factors, motor_strength [n][12], gravity_offset [n][3], env_friction, env_mass [n]"""
        R = self.P["ranges"]
        w = self.w("RESET_DR", np.asarray(envs)[:, None], rc, np.arange(11)[None, :])          # [n][11][4]
        n = len(envs)
        return {"kp_factors": rand_float(*lerp_range(R["kpf"], ts), w[:, 0:3]).reshape(n, 12),
                "kd_factors": rand_float(*lerp_range(R["kdf"], ts), w[:, 3:6]).reshape(n, 12),
                "gravity_offset": rand_float(*lerp_range(R["goff"], ts), w[:, 6, :3]),
                "motor_strength": rand_float(*lerp_range(R["mstr"], ts), w[:, 7:10]).reshape(n, 12),
                "env_friction": rand_float(*lerp_range(R["friction"], ts), w[:, 10, 0]),
                "env_mass": rand_float(*lerp_range(R["mass"], ts), w[:, 10, 1])}

    # -- purpose 16
    def kpkd(self, envs, rc, ts):
        w = self.w("RESET_KPKD", envs, rc, 0)
        return rand_float(*lerp_range(self.P["ranges"]["kpr"], ts), w[:, 0]), rand_float(*lerp_range(self.P["ranges"]["kdr"], ts), w[:, 1])

    # -- purpose 8
    def pose(self, envs, rc, delay_max_cur):
        """z float32, roll, pitch float32 (radians), delay int32"""
        P = self.P
        w = self.w("RESET_POSE", envs, rc, 0)
        d2r = math.pi / 180.0
        lo, hi = P["init_euler_deg"][0] * d2r, P["init_euler_deg"][1] * d2r
        max_d = max(P["min_delay"], min(delay_max_cur, P["max_delay"]))
        return {"z": rand_float(P["init_z"][0], P["init_z"][1], w[:, 0]), "roll": rand_float(lo, hi, w[:, 1]), "pitch": rand_float(lo, hi, w[:, 2]),
                "delay": rand_int(P["min_delay"], max_d, w[:, 3])}

    # -- purposes 7 and 3
    def reset_commands(self, envs, rc, ranges):
        return commands(self.w("RESET_CMD", envs, rc, 0), ranges, self.P["compound"], envs, self.P["n_standing"])

    def step_commands(self, envs, step, ranges):
        return commands(self.w("CMD", envs, step, 0), ranges, self.P["compound"], envs, self.P["n_standing"])

    # -- purpose 2
    def push(self, envs, step, force_lo, force_hi):
        """(force float32 [n][2], duration int32 [n])"""
        w = self.w("PUSH", envs, step, 0)
        return (np.stack([rand_float(force_lo, force_hi, w[:, 0]), rand_float(force_lo, force_hi, w[:, 1])], axis=1),
                rand_int(self.P["push_dur"][0], self.P["push_dur"][1], w[:, 2]))

    # -- purposes 1 and 4
    def action_noise(self, envs, step):
        """float64 [n][12]"""
        return normals(self.w("ACTION_NOISE", np.asarray(envs)[:, None], step, np.arange(3)[None, :])).reshape(len(envs), 12)

    def obs_noise(self, envs, step, nobs):
        """float64 [n][nobs]"""
        nblk = (nobs + 3) // 4
        return normals(self.w("OBS_NOISE", np.asarray(envs)[:, None], step, np.arange(nblk)[None, :])).reshape(len(envs), 4 * nblk)[:, :nobs]


def obs_noise_vec(nobs, level, noise, scales):
    """_rebuild_obs_noise_vec: python-float products rounded into the float32 vector.  noise / scales: dicts ang_vel, gravity, dof_pos, dof_vel"""
    v = np.zeros(nobs, F)
    v[0:3] = F(noise["ang_vel"] * scales["ang_vel"] * level)
    v[3:6] = F(noise["gravity"] * level)
    v[9:21] = F(noise["dof_pos"] * scales["dof_pos"] * level)
    v[21:33] = F(noise["dof_vel"] * scales["dof_vel"] * level)
    return v
