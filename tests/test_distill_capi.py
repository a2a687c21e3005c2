"""Boundary checks of the distillation C ABI (include/go2sim_distill.h) that need no GPU: the header parses into a list of its own, the prefix holds, the list
is disjoint from every other list, the product library exports it, and the lists the CPU-twin tests walk are as they were."""
import ctypes
import os
import re

from go2_sim2real_locomotion_rl_amd import capi

EXPECTED = {"go2sim_distill_act", "go2sim_distill_create", "go2sim_distill_destroy", "go2sim_distill_window_grad", "go2sim_distill_loss_only", "go2sim_distill_apply",
            "go2sim_distill_update", "go2sim_distill_n_params", "go2sim_distill_export", "go2sim_distill_import", "go2sim_distill_n_padded",
            "go2sim_distill_export_padded", "go2sim_distill_set_step", "go2sim_distill_reset_stats", "go2sim_distill_stats"}


def test_distill_header_parses():
    assert set(capi.DECLARED_DISTILL_FUNCS) == EXPECTED and len(capi.DECLARED_DISTILL_FUNCS) == len(EXPECTED)
    assert all(n.startswith("go2sim_distill_") for n in capi.DECLARED_DISTILL_FUNCS)
    C = capi.C
    assert [C["GO2SIM_DISTILL_" + n] for n in ("PARAMS", "GRADS", "ADAM_M", "ADAM_V")] == [0, 1, 2, 3]
    assert (C["GO2SIM_DISTILL_MSE"], C["GO2SIM_DISTILL_HUBER"]) == (0, 1)
    assert C["GO2SIM_DISTILL_N_STATS"] == C["GO2SIM_DISTILL_ST_WINDOWS"] + 1 == 6
    assert C["GO2SIM_DISTILL_SUB_ROWS"] % C["GO2SIM_PPO_ROW_CHUNK"] == 0


def test_distill_list_is_disjoint_from_every_other_list():
    others = [capi.DECLARED_FUNCS, capi.DECLARED_TRAIN_FUNCS, capi.DECLARED_RNN_FUNCS, capi.DECLARED_NORM_FUNCS, capi.DECLARED_LIDAR_FUNCS, capi.DECLARED_STAIRINFO_FUNCS]
    for lst in others:
        assert not set(lst) & set(capi.DECLARED_DISTILL_FUNCS)
        assert not any(n.startswith("go2sim_distill_") for n in lst)
    assert len(capi.DECLARED_FUNCS) == 53                                   # no CPU twin: the list the twin tests walk is as it was
    assert all(n.startswith("go2sim_ppo_") for n in capi.DECLARED_TRAIN_FUNCS)
    for other in ("go2sim.h", "go2sim_policy.h", "go2sim_train.h"):
        assert "go2sim_distill_" not in open(os.path.join(capi.REPO_ROOT, "include", other)).read()


def test_hip_library_exports_every_distill_function(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in capi.DECLARED_DISTILL_FUNCS:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_cfg_layout_matches_the_header():
    txt = open(capi.DISTILL_HEADER).read()
    cfg = txt[txt.index("typedef struct go2sim_distill_cfg {"):txt.index("} go2sim_distill_cfg_t;")]
    pos = [re.search(r"\b" + n + r"\s*[,;]", cfg).start() for n, _ in capi.DistillCfg._fields_]
    assert pos == sorted(pos)
    assert ctypes.sizeof(capi.DistillCfg) == 5 * 8 + 2 * 4


def test_kernels_are_shared_not_copied():
    """the backward kernels, the chunk reduction, the norm and Adam live in one device header that both updates include"""
    csrc = os.path.join(capi.REPO_ROOT, "go2_sim2real_locomotion_rl_amd", "csrc")
    shared = open(os.path.join(csrc, "go2sim_train_dev.h")).read()
    for fn in ("go2sim_train.hip", "go2sim_distill.hip"):
        txt = open(os.path.join(csrc, fn)).read()
        assert '#include "go2sim_train_dev.h"' in txt, fn
        for k in ("k_train_forward", "k_bwd_dw", "k_bwd_db", "k_bwd_da", "k_reduce_partials", "k_sumsq", "k_adam"):
            assert re.search(r"__global__[^;{]*\b" + k + r"\b", txt) is None, (fn, k)
            assert re.search(r"__global__[^;{]*\b" + k + r"\b", shared) is not None, k
            assert k in txt, (fn, k)
    for fn in ("distillation.py", os.path.join("csrc", "go2sim_distill.hip"), os.path.join("csrc", "go2sim_train_dev.h")):
        txt = open(os.path.join(capi.REPO_ROOT, "go2_sim2real_locomotion_rl_amd", fn)).read()
        assert "libgo2sim_cpu" not in txt and "go2sim_cpu_" not in txt and "load_cpu_oracle_lib" not in txt, fn
