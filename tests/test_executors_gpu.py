"""The two executors of the env step's launch list -- the step graph and plain launches -- named outright with GO2SIM_GRAPH=1 / GO2SIM_GRAPH=0 (so the
test does not depend on which of them is the default): every output of every step and the final state, bit for bit, on the walk, the stairs and a
base env, with envs resetting on every step, new output tensors in the middle of the run and a fresh action tensor per step (the per-step
arguments of three graph nodes)."""
import numpy as np
import pytest

from util import GpuEnv, bits_equal, make_actions, outputs_differing, with_knobs

pytestmark = pytest.mark.gpu

FIELDS = ["F_QPOS", "F_VEL", "F_ACC", "F_EFC_FORCE", "I_N_CONTACTS", "I_SOLVER_ITERS"]
ENV_BUFS = [("COMMANDS", 3, np.float32), ("EPISODE_LENGTH", 1, np.int32), ("EPISODE_SUMS", 32, np.float32), ("REW_TERMS", 32, np.float32),
            ("FEET_AIR_TIME", 4, np.float32), ("FOOT_CONTACT", 4, np.int32), ("BASE_EULER", 3, np.float32)]


def _env(hip_lib, blob, n_envs, task, graph):
    with with_knobs({"GO2SIM_GRAPH": "1" if graph else "0"}):
        return GpuEnv(hip_lib, blob, n_envs, seed=9, task=task)


@pytest.mark.parametrize("task,n_envs", [("walk", 130), ("walk", 4096), ("stairs", 70), ("jump_dr", 130)])
def test_graph_and_plain_executors_bit_equal(hip_lib, blob, task, n_envs):
    import torch
    from go2_sim2real_locomotion_rl_amd.capi import C

    steps = 10 if n_envs == 4096 else 24
    g, p = _env(hip_lib, blob, n_envs, task, True), _env(hip_lib, blob, n_envs, task, False)
    assert g.sim.graph_status() == (True, 0) and p.sim.graph_status()[0] is False, "each handle runs the executor it was asked for"
    g.reset(); p.reset()
    from util import task_cfg
    max_ep = int(task_cfg(task, n_envs)[1][C["GO2SIM_IC_MAX_EPISODE_LENGTH"]])
    ep = torch.from_numpy((max_ep - steps + 1 + np.arange(n_envs) % steps).astype(np.int32)).to(g.dev)     # a time-out on every step
    g.sim.env_set_episode_length(ep); p.sim.env_set_episode_length(ep)
    resets = reset_steps = 0
    for s, a in enumerate(make_actions(steps, n_envs, seed=5, kind="0.5", n_act=g.n_act)):
        if s == steps // 2:                                        # new output tensors: new arguments of the last graph node
            for e in (g, p):
                e.obs = torch.zeros_like(e.obs); e.priv = torch.zeros_like(e.priv); e.rew = torch.zeros_like(e.rew)
        og, op = g.step(a), p.step(a)
        bad = outputs_differing(og, op)
        bad += [n for n, k, dt in ENV_BUFS if not bits_equal(g.env_buf(n, k, dt), p.env_buf(n, k, dt))]
        assert not bad, f"{task} step {s}: {bad} differ between the executors"
        resets += int(og[3].sum()); reset_steps += int(og[3].sum() > 0)
    bad = [f for f in FIELDS if not bits_equal(g.field(f), p.field(f))]
    assert not bad, f"{task}: {bad} differ after {steps} steps"
    assert reset_steps == steps, (reset_steps, resets)
    assert g.sim.check_errno() == p.sim.check_errno() == 0
    assert g.sim.graph_status() == (True, 0) and p.sim.graph_status()[0] is False, "no fallback, no switch during the run"
