"""The stream map of the random draws (tests/env_rng_ref.py STREAMS; include/go2sim_rng.h) on the HIP product library: the scenarios and assertions
of tests/test_env_rng_ref.py (tests/env_rng_cases.py), against the same numpy reference and the same two bounds, plus what only the product has:

  * purpose 16, the per-env gains with per-leg stiffness off: GO2SIM_F_BASE_KP / GO2SIM_F_BASE_KD of modes A and B equal the numpy draw to the bit on
    env_reset, on reset_idx and on in-step resets;
  * both forms of the reset draws: the one-lane form (env_reset, reset_idx) and the team form (in-step resets, lane k forms block k); the coverage
    check asserts that both paths produced resets;
  * the shared-globals path, keyed by sync_calls (the oracle runs that scenario too).

Each seed runs in a few seconds: 33 envs x 13 steps and smaller."""
import pytest

import env_rng_cases as K
import env_rng_ref as R

PURPOSES = R.ENV_PURPOSES + (R.PURPOSE["RESET_KPKD"],)
ROWS = K.rows_of(PURPOSES)


@pytest.fixture(scope="module")
def tally(hip_lib, blob):
    return K.run_all(hip_lib, blob, gpu=True)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS)
def test_hip_draws_the_row_from_its_word(tally, row):
    K.check_row(tally, row)


@pytest.mark.gpu
def test_every_row_was_compared_on_both_reset_paths(tally):
    K.check_coverage(tally, PURPOSES)
