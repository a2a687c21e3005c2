"""The stream map of the random draws (tests/env_rng_ref.py STREAMS; include/go2sim_rng.h) on the CPU: that the map is well formed, and that both
oracle builds draw every quantity of purposes 1..10 from the Philox word the map names.  The HIP library runs the same scenarios in
tests/test_env_rng_gpu.py.

(a) Well-formedness: no two rows with different quantities share a (purpose, block, word); every purpose has one key kind and one env-word kind; the
    purposes are distinct across env, sensors and policy; every number is capi.C's.  (With GO2SIM_RNG_RESET_KPKD = 11, as it was, the first check
    fails naming kpkd.kp / kpkd.kd against policy.noise.)
(b) Oracle == numpy, row by row (tests/env_rng_cases.py).  To the bit where the transform is rand_float, rand_int or a comparison.  Within a bound
    where the value passes through dm_normal2 or dm_sincos; the bound is 4 x the worst deviation measured here, rounded up to one digit:

        dm_normal2 against float64 Box-Muller, 2^16 Philox blocks per seed:   measured 1.42e-6 (seed 5), 1.68e-6 (seed 0x300000005)  ->  7e-6
        euler_to_quat_wxyz against float64 over +-5 deg, 2^16 pairs:          measured 8.7e-8                                        ->  4e-7

    The two measurements are repeated below and the bounds held to them (4 x measured <= bound, bound <= 8 x measured).
(c) Coverage: every row of purposes 1..10 had at least one value compared, both branches of sample_level were taken, and env_reset, reset_idx and
    in-step resets all produced resets.  The policy's row (11) is held by tests/test_policy_ref.py, the sensors' rows by their own references, purpose
    16 by tests/test_env_rng_gpu.py (the oracle has no PLS-off path)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import env_rng_cases as K
import env_rng_ref as R
import lidar_ref
import policy_ref as PR
import stairinfo_ref
import tiles_ref
import wells_ref
from go2_sim2real_locomotion_rl_amd import capi

ENV_ROWS = K.rows_of(R.ENV_PURPOSES)


# ---- (a) the map --------------------------------------------------------------------------------------------------------------------------------------
def test_no_two_quantities_share_a_word():
    found = R.clashes()
    assert not found, "different quantities read one word: " + "; ".join(f"{a} and {b} at (purpose, block, word) {c}" for a, b, c in found)


def test_the_old_number_of_the_pls_off_gains_clashes_with_the_policy_noise():
    """The defect this map was written for: purpose 11 twice.  The check above names both rows."""
    old = [r._replace(purpose=11) if r.name.startswith("kpkd.") else r for r in R.STREAMS]
    found = R.clashes(old)
    assert {(a, b) for a, b, _ in found} == {("kpkd.kp", "policy.noise"), ("kpkd.kd", "policy.noise")}, found
    assert {cell for _, _, cell in found} == {(11, 0, 0), (11, 0, 1)}


def test_one_key_and_one_env_word_per_purpose():
    assert R.mixed_kinds() == {}


def test_purposes_are_distinct_and_are_the_headers():
    C = capi.C
    names = {"ACTION_NOISE", "PUSH", "CMD", "OBS_NOISE", "RESET_DR", "GLOBAL_DR", "RESET_CMD", "RESET_POSE", "TERRAIN_ROW", "TERRAIN_PERM", "POLICY_NOISE",
             "RESET_KPKD"}
    in_header = {k[len("GO2SIM_RNG_"):]: v for k, v in C.items() if k.startswith("GO2SIM_RNG_")}
    assert set(in_header) == names, "include/go2sim_rng.h and the map list the same streams"
    for n in names:
        assert R.PURPOSE[n] == in_header[n], n
    for n in ("LIDAR", "STAIRINFO", "TILES", "WELLS"):
        assert R.PURPOSE[n] == C[f"GO2SIM_{n}_RNG_PURPOSE"], n
    assert (lidar_ref.PURPOSE, stairinfo_ref.PURPOSE, tiles_ref.PURPOSE, wells_ref.PURPOSE, wells_ref.PURPOSE_POSE) == (
        R.PURPOSE["LIDAR"], R.PURPOSE["STAIRINFO"], R.PURPOSE["TILES"], R.PURPOSE["WELLS"], R.PURPOSE["RESET_POSE"])
    assert len(set(R.PURPOSE.values())) == len(R.PURPOSE), "two streams with one number draw the same words"
    assert {r.purpose for r in R.STREAMS} == set(R.PURPOSE.values()), "every purpose has a row and every row a listed purpose"
    assert np.array_equal(PR.noise64(3, 5, 7, 2), R.normals(R.words(7, R.PURPOSE["POLICY_NOISE"], np.arange(3)[:, None], 2, np.arange(2)[None, :])).reshape(3, 8)[:, :5])


# ---- the two measured bounds -------------------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include "go2sim_detmath.h"
extern "C" {
void normal_probe(int n, const unsigned* w, float* out) {
  for (int i = 0; i < n; ++i) { dm_normal2(w[4 * i], w[4 * i + 1], out + 4 * i, out + 4 * i + 1); dm_normal2(w[4 * i + 2], w[4 * i + 3], out + 4 * i + 2, out + 4 * i + 3); } }
void quat_probe(int n, const float* roll, const float* pitch, float* out) {   /* euler_to_quat_wxyz as env_reset_one has it, yaw = 0 */
  for (int i = 0; i < n; ++i) {
    float sr, cr, sp, cp, sy, cy;
    dm_sincos(roll[i] / 2.0f, &sr, &cr); dm_sincos(pitch[i] / 2.0f, &sp, &cp); dm_sincos(0.0f / 2.0f, &sy, &cy);
    out[4 * i] = cr * cp * cy + sr * sp * sy; out[4 * i + 1] = sr * cp * cy - cr * sp * sy;
    out[4 * i + 2] = cr * sp * cy + sr * cp * sy; out[4 * i + 3] = cr * cp * sy - sr * sp * cy; } }
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("env_rng_probe")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(capi.REPO_ROOT, "include"), str(d / "probe.cpp"), "-o",
                    str(d / "probe.so")], check=True)
    return ctypes.CDLL(str(d / "probe.so"))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_normal_bound_is_four_times_the_measured_deviation(probe):
    n, worst = 1 << 16, 0.0
    for case in K.SEEDS.values():
        w = np.ascontiguousarray(R.words(case["seed"], R.PURPOSE["ACTION_NOISE"], np.arange(n), 0, 0))
        out = np.zeros((n, 4), np.float32)
        probe.normal_probe(n, _p(w), _p(out))
        dev = float(np.abs(out.astype(np.float64) - R.normals(w)).max())
        print(f"dm_normal2 vs float64 Box-Muller, seed {case['seed']:#x}: worst {dev:.3e}")
        worst = max(worst, dev)
    assert 4.0 * worst <= R.NORMAL_ABS <= 8.0 * worst, (worst, R.NORMAL_ABS)


def test_quaternion_bound_is_four_times_the_measured_deviation(probe):
    n = 1 << 16
    lo, hi = np.radians(-5.0), np.radians(5.0)                          # init_euler_range of the walk configuration
    w = R.words(5, R.PURPOSE["RESET_POSE"], np.arange(n), 0, 0)
    roll, pitch = np.ascontiguousarray(R.rand_float(lo, hi, w[:, 1])), np.ascontiguousarray(R.rand_float(lo, hi, w[:, 2]))
    out = np.zeros((n, 4), np.float32)
    probe.quat_probe(n, _p(roll), _p(pitch), _p(out))
    worst = float(np.abs(out.astype(np.float64) - R.quat64(roll, pitch)).max())
    print(f"euler_to_quat_wxyz vs float64: worst {worst:.3e}")
    assert 4.0 * worst <= R.QUAT_ABS <= 8.0 * worst, (worst, R.QUAT_ABS)


# ---- (b), (c) the oracle builds ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["strict", "fast"])
def tally(request, blob):
    """Every scenario once per oracle build; the tests below read the tally.  GO2SIM_TEST_ORACLE_LIB points the strict case at another build of the
    oracle (a copy with a planted fault: DESIGN.md "Stream map" lists which rows each fault fails)."""
    alt = os.environ.get("GO2SIM_TEST_ORACLE_LIB")
    if alt and request.param == "strict":
        lib = capi.Go2SimLib(os.path.abspath(alt), "go2sim_cpu_")
    else:
        lib = request.getfixturevalue("oracle_fast_lib" if request.param == "fast" else "oracle_strict_lib")
    return K.run_all(lib, blob, gpu=False)


@pytest.mark.parametrize("row", ENV_ROWS)
def test_oracle_draws_the_row_from_its_word(tally, row):
    K.check_row(tally, row)


def test_every_env_row_was_compared(tally):
    K.check_coverage(tally, R.ENV_PURPOSES)
    assert not [r for r in tally.n if R.ROWS[r].purpose not in R.ENV_PURPOSES], "the oracle has no PLS-off path"
