"""The stairwell env's part of the C ABI exists: the header's constants, the new config word and the exported symbols of the product library."""
import ctypes
import os

import pytest

from go2_sim2real_locomotion_rl_amd import capi
from go2_sim2real_locomotion_rl_amd.capi import C

FUNCS = ("go2sim_wells_create", "go2sim_wells_destroy", "go2sim_wells_step", "go2sim_wells_clear", "go2sim_wells_get_alive", "go2sim_wells_set_alive",
         "go2sim_wells_alive_ep")


def test_constants():
    assert C["GO2SIM_WELLS_RNG_PURPOSE"] == 15 and C["GO2SIM_TILES_RNG_PURPOSE"] == 14 and C["GO2SIM_LIDAR_RNG_PURPOSE"] == 12
    assert C["GO2SIM_WELLS_PRIV_EXTRA"] == 56 and C["GO2SIM_WELLS_AXIS_MAX"] == 16 and C["GO2SIM_WELLS_LEVELS_MAX"] == 16
    assert C["GO2SIM_IC_WELL_SPAWN"] == C["GO2SIM_IC_TILE_N_COLS"] + 1 == C["GO2SIM_IC_COUNT"] - 1      # a new word after the existing ones
    assert C["GO2SIM_R_COUNT"] == 35                                                                     # the alive term is not a core reward id


def test_header_declares_the_entry_points():
    assert sorted(capi.DECLARED_WELLS_FUNCS) == sorted(FUNCS)
    assert all(f in capi.PRODUCT_ONLY_FUNCS for f in FUNCS)
    text = open(capi.WELLS_HEADER).read()
    for word in ("purpose 15", "alive is added after the core's sum", "Lane t owns the columns"):
        assert word in text


def test_product_library_exports_them():
    if not os.path.exists(capi.HIP_LIB):
        pytest.fail(f"{capi.HIP_LIB} is not built")
    lib = ctypes.CDLL(capi.HIP_LIB)
    for f in FUNCS:
        assert hasattr(lib, f), f
