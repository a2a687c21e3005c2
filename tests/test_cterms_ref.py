"""The contact terms (include/go2sim_cterms.h) without a GPU: the numpy restatement tests/cterms_ref.py against the reference's own methods
(tests/golden/ref_cterms.npz, tools/make_ref_cterms_fixtures.py), the header, the library's symbols and the ctypes struct, the configuration
(flatten_walk_cfg, get_stair_info_cfgs against tests/golden/ref_cfgs_stair_info.json) and the refusals."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest

import cterms_ref as R
from go2_sim2real_locomotion_rl_amd import Go2SimError, capi
from go2_sim2real_locomotion_rl_amd.capi import C
from go2_sim2real_locomotion_rl_amd.configs import (CONTACT_TERM_NAMES, flatten_base_cfg, flatten_walk_cfg, get_crouch_cfgs, get_rough_cfgs, get_stair_cfgs,
                                                    get_stair_info_cfg, get_stair_info_cfgs, get_stair_info_terrain_cfg, get_stair_lidar_cfgs,
                                                    get_stairwell_cfgs, get_walk_cfgs)
from go2_sim2real_locomotion_rl_amd.contact_terms import CtermsCfg, contact_term_scales, link_mask, non_foot_links, resolve_body_links
from go2_sim2real_locomotion_rl_amd.model_blob import load_model_json

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUNCS = ("go2sim_cterms_create", "go2sim_cterms_destroy", "go2sim_cterms_step", "go2sim_cterms_clear", "go2sim_cterms_get_state",
         "go2sim_cterms_set_state", "go2sim_cterms_ep")
BLOCKS = ("random", "edge_body", "edge_stumble", "zero", "special")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "ref_cterms.npz"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the restatement against the reference's own methods --------------------------------------------------------------------------------
def test_tables_are_the_tools_and_the_links_the_models(fx):
    assert tuple(fx["robot_links"]) == R.ROBOT_LINKS == tuple(l["name"] for l in load_model_json()["links"][1:])
    assert tuple(fx["body_links"]) == R.THIGHS and tuple(fx["stumble_links"]) == R.NON_FEET and len(R.NON_FEET) == 9
    assert np.array_equal(bits(fx["random_forces"]), bits(R.random_rows(300, seed=7)))
    assert np.array_equal(bits(fx["edge_body_forces"]), bits(R.edge_rows(R.BODY_THRESHOLD, R.THIGHS)[0]))
    n = R.norms64(fx["random_forces"])
    assert n.max() < 50.0 and (n == 0).mean() > 0.3 and len(fx["random_forces"]) == 300


@pytest.mark.parametrize("block", [b for b in BLOCKS if b != "special"])
def test_body_contact_counts_are_the_references(fx, block):
    F, thr = fx[block + "_forces"], float(fx[block + "_body_threshold"])
    frac = R.check_ambiguity_cap(F, R.THIGHS, thr)                         # the reference alone holds the cap
    lo, hi, _ = R.body_count_sets(F, R.THIGHS, thr)
    got = fx[block + "_body_contact"]
    print(f"{block}: {len(F)} rows, {100 * frac:.2f} % ambiguous link-rows, counts {np.unique(got).tolist()}")
    assert got.dtype == np.float32 and np.all((lo <= got) & (got <= hi)) and np.array_equal(got, np.round(got))
    assert np.array_equal(R.law32(F, R.THIGHS, R.NON_FEET, thr, float(fx[block + "_stumble_threshold"]))[0][lo == hi], got[lo == hi])


@pytest.mark.parametrize("block", [b for b in BLOCKS if b != "special"])
def test_stumble_is_the_references_within_the_bound(fx, block):
    F, thr = fx[block + "_forces"], float(fx[block + "_stumble_threshold"])
    pen, bound = R.stumble64(F, R.NON_FEET, thr)
    for name, got in (("reference", fx[block + "_stumble"]), ("float32 law", R.law32(F, R.THIGHS, R.NON_FEET, 1.0, thr)[1])):
        err = np.abs(got.astype(np.float64) - pen)
        print(f"{block}, {name}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, largest penalty {pen.max():.3f}")
        assert np.all(err <= bound)
    assert block != "random" or (pen > 0).mean() > 0.5


def test_threshold_edges(fx):
    """single-component forces: at the threshold 0, one float32 above it 1 -- in x, y and z, both signs"""
    for block, over_key, links in (("edge_body", "edge_body_over", R.THIGHS), ("edge_stumble", "edge_stumble_over", (R.NON_FEET[0], R.NON_FEET[-1]))):
        F, over = fx[block + "_forces"], fx[over_key]
        assert len(F) == len(links) * 12 and over.sum() == len(F) // 2
        assert ((F != 0).sum((1, 2)) == 1).all() and (F < 0).any() and all((F[:, :, c] != 0).any() for c in range(3))
        count, pen = R.law32(F, R.THIGHS, R.NON_FEET)
        assert np.array_equal(bits(count), bits(fx[block + "_body_contact"])) and np.array_equal(bits(pen), bits(fx[block + "_stumble"]))
        lo, hi, amb = R.body_count_sets(F, R.THIGHS, R.BODY_THRESHOLD)
        assert not amb.any() and np.array_equal(lo, count)
    assert np.array_equal(fx["edge_body_body_contact"], fx["edge_body_over"].astype(np.float32))
    assert np.array_equal(fx["edge_stumble_stumble"] > 0, fx["edge_stumble_over"])
    assert np.all(fx["edge_stumble_stumble"][fx["edge_stumble_over"]] == np.nextafter(np.float32(5), np.float32(9)) - np.float32(5))


def test_zero_threshold_and_special_values(fx):
    z = fx["zero_forces"]
    loaded = (R.norms64(z)[:, list(R.THIGHS)] > 0).sum(1)
    assert np.array_equal(fx["zero_body_contact"], loaded.astype(np.float32)) and fx["zero_body_contact"][-1] == 0 and fx["zero_stumble"][-1] == 0
    F = fx["special_forces"]
    count, pen = R.law32(F, R.THIGHS, R.NON_FEET)
    assert np.array_equal(bits(count), bits(fx["special_body_contact"])) and np.array_equal(np.isnan(pen), np.isnan(fx["special_stumble"]))
    assert np.array_equal(pen[~np.isnan(pen)], fx["special_stumble"][~np.isnan(pen)])
    assert count.tolist() == [0.0, 1.0, 1.0, 2.0, 0.0]                      # a NaN norm compares false, an infinite one true
    assert np.isnan(pen[[0, 1, 4]]).all() and np.isposinf(pen[[2, 3]]).all()


def test_hand_over_and_episode_model():
    ep = R.Episode(3)
    inc = R.inc32(-2.0)
    assert inc == np.float32(-2.0 * 0.02)                                   # the product in float64, rounded once
    rew = ep.step(np.zeros(3, np.float32), {0: np.float32([1, 0, 2]) * inc}, [0, 0, 0])
    rew = ep.step(rew, {0: np.float32([1, 1, 0]) * inc}, [1, 0, 0])
    assert ep.steps[0].tolist() == [0, 2, 2] and ep.sum[0, 0] == 0 and ep.steps[1].tolist() == [0, 0, 0]
    two = np.float32(inc + inc)
    assert ep.ep[0, 0] == two / (np.float32(2) * np.float32(0.02)) and rew[0] == two and rew[2] == np.float32(2) * inc
    ep.clear([2, 1])
    assert ep.ep[0, 1] == inc / (np.float32(2) * np.float32(0.02)) and ep.steps[0].tolist() == [0, 0, 0]
    assert R.hand_over(np.float32(0), 0) == 0.0                             # max(steps, 1)


# ---- 2. header, library, struct -----------------------------------------------------------------------------------------------------------
def test_header_parses_into_its_own_list():
    assert sorted(capi.DECLARED_CTERMS_FUNCS) == sorted(FUNCS)
    assert all(f in capi.PRODUCT_ONLY_FUNCS for f in FUNCS)
    others = [capi.DECLARED_FUNCS, capi.DECLARED_TRAIN_FUNCS, capi.DECLARED_RNN_FUNCS, capi.DECLARED_NORM_FUNCS, capi.DECLARED_LIDAR_FUNCS,
              capi.DECLARED_STAIRINFO_FUNCS, capi.DECLARED_DISTILL_FUNCS, capi.DECLARED_RDISTILL_FUNCS, capi.DECLARED_ACT_FUNCS, capi.DECLARED_RND_FUNCS,
              capi.DECLARED_TILES_FUNCS, capi.DECLARED_WELLS_FUNCS, capi.DECLARED_STATE_FUNCS]
    assert all(not set(FUNCS) & set(o) for o in others)
    assert len(capi.DECLARED_FUNCS) == 53 and C["GO2SIM_R_COUNT"] == 35     # neither the core's ABI nor its reward ids grew
    assert C["GO2SIM_CTERMS_LINKS_MAX"] == 32 and (C["GO2SIM_CTERMS_BODY"], C["GO2SIM_CTERMS_STUMBLE"], C["GO2SIM_CTERMS_N"]) == (0, 1, 2)
    text = open(capi.CTERMS_HEADER).read()
    for word in ("a NaN norm compares false", "the terms are added after the core's sum", "one lane per env", "first body_contact, then stumble"):
        assert word in text


def test_product_library_exports_every_function():
    if not os.path.exists(capi.HIP_LIB):
        pytest.fail(f"{capi.HIP_LIB} is not built")
    lib = ctypes.CDLL(capi.HIP_LIB)
    for f in FUNCS:
        assert hasattr(lib, f), f


def test_ctypes_struct_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(capi.CTERMS_HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{(.*?)\} go2sim_cterms_cfg_t;", text, flags=re.S).group(1)
    ctype = {"double": ctypes.c_double, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32}
    want = []
    for decl in body.split(";"):
        if decl.strip():
            t, names = decl.split(None, 1)
            want += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert CtermsCfg._fields_ == want and ctypes.sizeof(CtermsCfg) == 5 * 8 + 4 * 4


def test_create_refuses_before_any_device_work():
    """the argument checks of go2sim_cterms_create come before its first HIP call: they answer without a GPU"""
    if not os.path.exists(capi.HIP_LIB):
        pytest.fail(f"{capi.HIP_LIB} is not built")
    lib = ctypes.CDLL(capi.HIP_LIB)

    def create(**kw):
        c = CtermsCfg(dt=0.02, body_contact_scale=-2.0, stumble_scale=0.0, body_contact_threshold=1.0, stumble_threshold=5.0, n_envs=4, n_links=14,
                      body_mask=R.model_mask(R.THIGHS), stumble_mask=R.model_mask(R.NON_FEET))
        for k, v in kw.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        rc = lib.go2sim_cterms_create(0, ctypes.byref(c), ctypes.byref(h))
        assert not h.value
        return rc

    bad = C["GO2SIM_E_BADARG"]
    assert create(body_mask=1 << 14) == bad and create(stumble_mask=1 << 31) == bad            # a mask bit at or above n_links
    assert create(n_envs=0) == bad and create(n_links=0) == bad and create(n_links=33) == bad
    assert create(dt=0.0) == bad and create(dt=float("nan")) == bad
    for key in ("body_contact_scale", "stumble_scale", "body_contact_threshold", "stumble_threshold"):
        assert create(**{key: float("nan")}) == bad
    assert lib.go2sim_cterms_create(0, None, None) == bad and lib.go2sim_cterms_step(None, 4, None, 1, 1, 1, None, None, None, None) == bad


# ---- 3. configuration ---------------------------------------------------------------------------------------------------------------------
def family_cfgs():
    out = {"walk": get_walk_cfgs(), "walk_nopls": get_walk_cfgs(False), "stairs": get_stair_cfgs(), "stairs_nopls": get_stair_cfgs(False),
           "rough_grid": get_rough_cfgs("grid"), "rough_heightmap": get_rough_cfgs("heightmap")}
    for name, (get, extra_key) in {"stairs_lidar": (get_stair_lidar_cfgs, "GO2SIM_LIDAR_PRIV_EXTRA"), "stairs_info": (get_stair_info_cfgs, "GO2SIM_STAIRINFO_PRIV_EXTRA"),
                                   "stairwell": (get_stairwell_cfgs, "GO2SIM_WELLS_PRIV_EXTRA")}.items():
        for pls in (True, False):
            env_cfg, obs_cfg, reward_cfg, command_cfg = get(pls)
            n_in = 33 + env_cfg["num_actions"]                               # the inner rows Go2Env hands to flatten_walk_cfg
            out[name + ("" if pls else "_nopls")] = (env_cfg, dict(obs_cfg, num_obs=n_in, num_privileged_obs=n_in + C[extra_key]), reward_cfg, command_cfg)
    return out


@pytest.mark.parametrize("family", sorted(family_cfgs()))
def test_flatten_accepts_both_names_and_leaves_the_core_alone(family):
    env_cfg, obs_cfg, reward_cfg, command_cfg = family_cfgs()[family]
    f0, i0, names0 = flatten_walk_cfg(8, env_cfg, obs_cfg, reward_cfg, command_cfg)
    for extra in ({"body_contact": -2.0}, {"stumble": -1.0}, {"stumble": -1.0, "body_contact": -2.0}, {"body_contact": 0.0}):
        rc = copy.deepcopy(reward_cfg)
        scales = dict(extra)
        scales.update(rc["reward_scales"])                                   # the new names FIRST in the dictionary: the core's order must not move
        rc["reward_scales"] = scales
        f, i, names = flatten_walk_cfg(8, env_cfg, obs_cfg, rc, command_cfg)
        assert names == names0 and not set(names) & set(CONTACT_TERM_NAMES)
        assert i[C["GO2SIM_IC_N_REWARDS"]] == i0[C["GO2SIM_IC_N_REWARDS"]] == len(names0)
        assert np.array_equal(i, i0) and np.array_equal(f, f0)               # every core id, every scale, everything else
        want = (extra.get("body_contact", 0.0), extra.get("stumble", 0.0))
        assert contact_term_scales(rc) == want


def test_default_stair_info_cfgs_are_unchanged():
    for pls in (True, False):
        want = get_stair_cfgs(pls)
        want[0]["stair_info"] = get_stair_info_cfg()
        want[0]["terrain"] = get_stair_info_terrain_cfg()
        n_in = 33 + want[0]["num_actions"]
        want[1]["num_obs"], want[1]["num_privileged_obs"] = n_in + 4, n_in + 4 + 55 + 1 + 4
        got = get_stair_info_cfgs(pls)
        assert got == want and got == get_stair_info_cfgs(pls, script_values=False)
        assert list(got[2]["reward_scales"]) == list(want[2]["reward_scales"])
        assert "body_contact" not in got[2]["reward_scales"] and "body_contact_names" not in got[0]
        assert got[0]["curriculum"]["level_init"] == 0.65 and got[2]["feet_height_target"] == 0.17


def test_script_values_equal_the_reference_script():
    ref = json.load(open(os.path.join(GOLDEN, "ref_cfgs_stair_info.json")))
    env_cfg, obs_cfg, reward_cfg, command_cfg = get_stair_info_cfgs(script_values=True)
    assert env_cfg == ref["env_cfg"] and obs_cfg == ref["obs_cfg"] and reward_cfg == ref["reward_cfg"] and command_cfg == ref["command_cfg"]
    assert list(reward_cfg["reward_scales"]) == list(ref["reward_cfg"]["reward_scales"])       # the same order: body_contact last in both
    assert list(reward_cfg["reward_scales"])[-1] == "body_contact" and reward_cfg["reward_scales"]["body_contact"] == -2.0
    assert env_cfg["curriculum"]["level_init"] == 0.2 and reward_cfg["feet_height_target"] == 0.15
    assert env_cfg["body_contact_names"] == ["FR_thigh", "FL_thigh"] and env_cfg["body_contact_threshold"] == 1.0
    diff = get_stair_info_cfgs(script_values=True, stair_info=dict(get_stair_info_cfg(), height_scale=4.0))
    assert diff[0]["stair_info"]["height_scale"] == 4.0 and diff[2] == reward_cfg


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_link_names_resolve_against_the_model():
    assert resolve_body_links() == [7, 6] and resolve_body_links(["RR_thigh", "base"]) == [9, 1]
    assert [l - 1 for l in resolve_body_links()] == list(R.THIGHS) and [l - 1 for l in non_foot_links()] == list(R.NON_FEET)
    assert link_mask(resolve_body_links()) == R.model_mask(R.THIGHS) == 0xC0 and link_mask(non_foot_links()) == R.model_mask(R.NON_FEET) == 0x3FE
    with pytest.raises(Go2SimError, match=r"\['FR_tigh'\] are no links of the robot.*FR_thigh"):
        resolve_body_links(["FR_thigh", "FR_tigh"])
    with pytest.raises(Go2SimError, match="planeLink"):                      # the ground is no link of the robot
        resolve_body_links(["planeLink"])
    with pytest.raises(Go2SimError, match="link index"):
        link_mask([32])


def test_the_base_env_keeps_refusing_both_names():
    env_cfg, obs_cfg, reward_cfg, command_cfg = get_crouch_cfgs()
    for name in CONTACT_TERM_NAMES:
        rc = copy.deepcopy(reward_cfg)
        rc["reward_scales"][name] = -1.0
        with pytest.raises(AttributeError, match=f"_reward_{name}"):
            flatten_base_cfg(8, env_cfg, obs_cfg, rc, command_cfg)
