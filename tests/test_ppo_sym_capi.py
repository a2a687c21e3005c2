"""Boundary checks of the mirror-symmetry part of the PPO-update C ABI (include/go2sim_train.h) that need no GPU: the header declares the new entry
points and capi parses them, the product library exports them, the ctypes mirror of go2sim_ppo_mirror_t follows the header, and the existing
statistics layout is as it was."""
import ctypes
import re

from go2_sim2real_locomotion_rl_amd import capi

NEW = {"go2sim_ppo_set_mirror", "go2sim_ppo_symmetry_loss"}


def test_header_declares_the_mirror_entry_points():
    assert NEW <= set(capi.DECLARED_TRAIN_FUNCS)
    assert not NEW & set(capi.DECLARED_FUNCS)                  # no CPU twin: they stay out of the list the twin tests walk
    assert capi.C["GO2SIM_PPO_N_STATS"] == 8 and capi.C["GO2SIM_PPO_ST_COUNT"] == 7
    txt = open(capi.TRAIN_HEADER).read()
    assert re.search(r"int go2sim_ppo_set_mirror\(go2sim_ppo_t\* h, const go2sim_ppo_mirror_t\* mirror, void\* stream\);", txt)
    assert re.search(r"int go2sim_ppo_create\(go2sim_mlp_t\* actor, go2sim_mlp_t\* critic, int n_actions, const go2sim_ppo_cfg_t\* cfg, "
                     r"int max_rows_per_minibatch, go2sim_ppo_t\*\* out\);", txt), "go2sim_ppo_create keeps its signature"
    for phrase in ("use_data_augmentation", "use_mirror_loss", "L_sym", "detached", "(M x)[j] = sign[j] x[src[j]]"):
        assert phrase in txt, f"the header states the law: {phrase!r}"


def test_hip_library_exports_the_mirror_entry_points(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in NEW:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_mirror_struct_layout_matches_the_header():
    txt = open(capi.TRAIN_HEADER).read()
    body = txt[txt.index("typedef struct go2sim_ppo_mirror {"):txt.index("} go2sim_ppo_mirror_t;")]
    pos = [re.search(r"\b" + n + r"\s*;", body).start() for n, _ in capi.PpoMirror._fields_]
    assert pos == sorted(pos) and len(pos) == 9
    assert ctypes.sizeof(capi.PpoMirror) == 6 * ctypes.sizeof(ctypes.c_void_p) + 2 * 4 + 8
    assert capi.PpoMirror.mirror_loss_coeff.offset == 6 * ctypes.sizeof(ctypes.c_void_p) + 8
