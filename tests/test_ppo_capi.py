"""Boundary checks of the PPO-update C ABI (include/go2sim_train.h) that need no GPU: the header parses into a list of its own, the product
library exports it, and the lists the CPU-twin tests walk are as they were."""
import ctypes
import os
import re

from go2_sim2real_locomotion_rl_amd import capi

import ppo_cases as PC

EXPECTED = {"go2sim_ppo_create", "go2sim_ppo_destroy", "go2sim_ppo_minibatch_grad", "go2sim_ppo_apply", "go2sim_ppo_update", "go2sim_ppo_export",
            "go2sim_ppo_import", "go2sim_ppo_stats"}


def test_train_header_parses():
    assert EXPECTED <= set(capi.DECLARED_TRAIN_FUNCS)
    assert all(n.startswith("go2sim_ppo_") for n in capi.DECLARED_TRAIN_FUNCS)
    C = capi.C
    assert [C["GO2SIM_PPO_" + n] for n in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V")] == [0, 1, 2, 3]
    assert C["GO2SIM_PPO_ROW_CHUNK"] == PC.ROW_CHUNK
    assert C["GO2SIM_PPO_N_STATS"] == C["GO2SIM_PPO_ST_COUNT"] + 1


def test_hip_library_exports_every_train_function(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in capi.DECLARED_TRAIN_FUNCS:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_declared_funcs_unchanged():
    """The update has no go2sim_cpu_ twin: the list the CPU-twin export test walks holds go2sim.h and go2sim_policy.h only."""
    own = capi._parse_header(capi.HEADER)[1] + capi._parse_header(os.path.join(capi.REPO_ROOT, "include", "go2sim_policy.h"))[1]
    assert capi.DECLARED_FUNCS == own
    assert len(capi.DECLARED_FUNCS) == 53
    assert not set(capi.DECLARED_FUNCS) & set(capi.DECLARED_TRAIN_FUNCS)


def test_struct_layouts_match_the_header():
    """ctypes mirrors of go2sim_ppo_cfg_t / go2sim_ppo_batch_t: field names in the header's order"""
    txt = open(capi.TRAIN_HEADER).read()
    cfg = txt[txt.index("typedef struct go2sim_ppo_cfg {"):txt.index("} go2sim_ppo_cfg_t;")]
    pos = [re.search(r"\b" + n + r"\s*[,;]", cfg).start() for n, _ in capi.PpoCfg._fields_]
    assert pos == sorted(pos)
    batch = txt[txt.index("typedef struct go2sim_ppo_batch {"):txt.index("} go2sim_ppo_batch_t;")]
    pos = [batch.index("* " + n + ";") for n in capi.PpoBatch.FIELDS]
    assert pos == sorted(pos)
    assert ctypes.sizeof(capi.PpoCfg) == 11 * 8 + 2 * 4 and ctypes.sizeof(capi.PpoBatch) == 9 * ctypes.sizeof(ctypes.c_void_p)


def test_product_still_does_not_reference_the_oracle():
    pkg = os.path.join(capi.REPO_ROOT, "go2_sim2real_locomotion_rl_amd")
    for fn in ("ppo.py", "runner.py", os.path.join("csrc", "go2sim_train.hip"), os.path.join("csrc", "go2sim_mlp_dev.h")):
        txt = open(os.path.join(pkg, fn)).read()
        assert "libgo2sim_cpu" not in txt and "go2sim_cpu_" not in txt and "load_cpu_oracle_lib" not in txt, fn
    inc = open(capi.TRAIN_HEADER).read()
    assert "go2sim_cpu_" not in inc
