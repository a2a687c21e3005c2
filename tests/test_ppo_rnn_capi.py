"""Boundary checks of the recurrent-policy C ABI (include/go2sim_rnn.h) that need no GPU: the header parses into a list of its own, the product library
exports every function of it, the ctypes mirror follows the header, and the lists of the other headers are as they were."""
import ctypes
import os

from go2_sim2real_locomotion_rl_amd import capi

EXPECTED = {"go2sim_lstm_create", "go2sim_lstm_destroy", "go2sim_lstm_set_params", "go2sim_lstm_get_params", "go2sim_lstm_step", "go2sim_ppo_create_recurrent",
            "go2sim_ppo_rnn_minibatch_grad", "go2sim_ppo_rnn_update"}


def test_rnn_header_parses():
    assert set(capi.DECLARED_RNN_FUNCS) == EXPECTED
    assert not set(capi.DECLARED_RNN_FUNCS) & (set(capi.DECLARED_FUNCS) | set(capi.DECLARED_TRAIN_FUNCS))
    txt = open(capi.RNN_HEADER).read()
    step = txt[txt.index("int go2sim_lstm_step("):]
    step = step[:step.index(";")]
    pos = [step.index(a) for a in ("go2sim_lstm_t* mem_a", "const float* x_a", "const float* h_in_a", "float* c_out_a", "go2sim_lstm_t* mem_c", "const uint8_t* reset",
                                   "int n_rows", "void* stream")]
    assert pos == sorted(pos)
    assert "go2sim_cpu_" not in txt


def test_hip_library_exports_every_rnn_function(libs_built):
    lib = ctypes.CDLL(capi.HIP_LIB)
    for name in capi.DECLARED_RNN_FUNCS:
        assert hasattr(lib, name), f"libgo2sim.so does not export {name}"


def test_state_struct_matches_the_header():
    txt = open(capi.RNN_HEADER).read()
    st = txt[txt.index("typedef struct go2sim_ppo_rnn_state {"):txt.index("} go2sim_ppo_rnn_state_t;")]
    pos = [st.index("* " + n + ";") for n in capi.PpoRnnState.FIELDS]
    assert pos == sorted(pos) and ctypes.sizeof(capi.PpoRnnState) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_the_other_lists_are_unchanged():
    assert len(capi.DECLARED_FUNCS) == 53 and all(n.startswith("go2sim_ppo_") for n in capi.DECLARED_TRAIN_FUNCS)
    pkg = os.path.join(capi.REPO_ROOT, "go2_sim2real_locomotion_rl_amd")
    txt = open(os.path.join(pkg, "csrc", "go2sim_lstm_dev.h")).read()
    assert "go2sim_cpu_" not in txt and "libgo2sim_cpu" not in txt


def test_package_exports_the_recurrent_policy():
    import go2_sim2real_locomotion_rl_amd as pkg

    assert pkg.ActorCriticRecurrent.is_recurrent is True and pkg.ActorCritic.is_recurrent is False
    assert issubclass(pkg.ActorCriticRecurrent, pkg.ActorCritic)
