"""Boundary checks of the activation C ABI (include/go2sim_activation.h) that need no GPU: the header parses into a list of its own, the list is disjoint
from every other list, the product library exports it, the enum is what the header says, the lists the CPU-twin tests walk are as they were, and the
Python classes refuse `crelu` and unknown names before anything touches the device."""
import ctypes
import os

import pytest

from go2_sim2real_locomotion_rl_amd import capi

NAMES = ("elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "identity")


def test_act_header_parses_into_its_own_list():
    assert capi.DECLARED_ACT_FUNCS == ["go2sim_act_set", "go2sim_act_get"]
    C = capi.C
    assert [C["GO2SIM_ACT_" + n.upper()] for n in NAMES] == [0, 1, 2, 3, 4, 5, 6] and C["GO2SIM_ACT_COUNT"] == 7
    assert capi.ACTIVATIONS == {n: i for i, n in enumerate(NAMES)}


def test_act_list_is_disjoint_from_every_other_list():
    others = [capi.DECLARED_FUNCS, capi.DECLARED_TRAIN_FUNCS, capi.DECLARED_RNN_FUNCS, capi.DECLARED_NORM_FUNCS, capi.DECLARED_LIDAR_FUNCS,
              capi.DECLARED_STAIRINFO_FUNCS, capi.DECLARED_DISTILL_FUNCS]
    for lst in others:
        assert not set(lst) & set(capi.DECLARED_ACT_FUNCS)
        assert not any(n.startswith("go2sim_act_") for n in lst)
    assert len(capi.DECLARED_FUNCS) == 53                                   # no CPU twin: the list the twin tests walk is as it was
    inc = os.path.join(capi.REPO_ROOT, "include")
    for other in sorted(f for f in os.listdir(inc) if f.endswith(".h") and f != "go2sim_activation.h"):
        assert "go2sim_act_" not in open(os.path.join(inc, other)).read(), other


def test_hip_library_exports_both_functions(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in capi.DECLARED_ACT_FUNCS:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_the_header_states_the_table_and_the_timing_of_the_setter():
    txt = open(capi.ACT_HEADER).read()
    for word in ("nn.ELU", "nn.SELU", "nn.ReLU", "nn.LeakyReLU", "nn.Tanh", "nn.Sigmoid", "nn.Identity", "crelu", "1.0507009873554805", "1.6732632423543772",
                 "before the network's first launch", "captured"):
        assert word in txt, word


@pytest.mark.parametrize("cls", ["ActorCritic", "ActorCriticRecurrent", "StudentTeacher"])
def test_crelu_and_unknown_names_are_refused_without_a_device(cls, monkeypatch):
    import torch

    import go2_sim2real_locomotion_rl_amd as pkg
    from go2_sim2real_locomotion_rl_amd.capi import Go2SimError

    def no_device(*a, **k):
        raise AssertionError("the refusal must come before anything touches the device")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    make = getattr(pkg, cls)
    with pytest.raises(Go2SimError, match="crelu"):
        make(19, 23, 8, [24], [24], activation="crelu")
    with pytest.raises(Go2SimError) as e:
        make(19, 23, 8, [24], [24], activation="swish")
    assert "swish" in str(e.value) and all(n in str(e.value) for n in NAMES)


def test_resolve_activation():
    from go2_sim2real_locomotion_rl_amd.policy import resolve_activation

    assert [resolve_activation(n) for n in NAMES] == list(NAMES) and resolve_activation("ELU") == "elu"
