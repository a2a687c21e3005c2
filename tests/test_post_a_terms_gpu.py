"""k_env_post_a's reward terms on both of its paths -- the worker waves' straight-line section (terms by id: a mask over ids per wave, id -> list slot, scales
by id, all built by deal_terms on the host) and the loop over the list (wave 0's stateful terms; every wave where the list names an id twice) -- and the
split of the frame math between wave 0 and the workers, against the FAST ORDER oracle at tolerance 0 after EVERY step, at 130 envs (a partial last workgroup,
and in it a partial wave).

Compared per step: the reward, the per-term rewards, the episode sums, feet_air_time, the done flags, the time-outs, the commands, base_euler and both
observation vectors.  _last_base_pos_x has no accessor in the C ABI: it is compared through forward_progress (the stairs list and the five-term list), whose
value on step s + 1 is base_pos.x minus the word stored on step s, so a wrong word shows in `rew_terms` one step later.

Every case asserts on the oracle's own outputs that it reaches what it is for (resets and command resamples inside the run, live terms)."""
import numpy as np
import pytest

from util import CpuEnv, F, GpuEnv, bits_equal, make_actions, outputs_differing, task_cfg

pytestmark = pytest.mark.gpu

N_ENVS = 130
ENV_BUFS = [("REW_TERMS", 32, np.float32), ("EPISODE_SUMS", 32, np.float32), ("FEET_AIR_TIME", 4, np.float32), ("COMMANDS", 3, np.float32),
            ("BASE_EULER", 3, np.float32)]


def _pair(oracle_lib, hip_lib, blob, task, mutate=None, edit_icfg=None):
    """The two sides on one configuration; edit_icfg(f, i) changes the flattened words after the name -> id translation (what no reward dict can say:
    the same id twice) and both sides are configured again with them."""
    cpu = CpuEnv(oracle_lib, blob, N_ENVS, seed=5, task=task, mutate=mutate)
    gpu = GpuEnv(hip_lib, blob, N_ENVS, seed=5, task=task, mutate=mutate)
    if edit_icfg is not None:
        f, i, *_ = task_cfg(task, N_ENVS, mutate=mutate)
        edit_icfg(f, i)
        cpu.sim.env_configure(f, i); gpu.sim.env_configure(f, i)
        cpu.icfg = i
    return cpu, gpu


def _run(cpu, gpu, steps, spread, seed, tag):
    """Resets both, staggers the episode counters over the last `spread` steps of the episode, runs `steps` steps of 2 N(0, 1) actions and compares after
    every step.  Returns (resets, command changes of envs that were not reset on that step, the oracle's term matrix summed in magnitude over the run)."""
    cpu.reset(); gpu.reset()
    max_ep = int(cpu.icfg[F("IC_MAX_EPISODE_LENGTH")])
    ep = (max_ep - spread + 1 + np.arange(N_ENVS) % spread).astype(np.int32)
    cpu.sim.env_set_episode_length(ep)
    gpu.sim.env_set_episode_length(gpu.torch.from_numpy(ep).to(gpu.dev))
    resets = resampled = 0
    live = np.zeros(32)
    cmd_before = cpu.env_buf("COMMANDS", 3).copy()
    for s, a in enumerate(make_actions(steps, N_ENVS, seed=seed, kind="2.0", n_act=cpu.n_act)):
        oc = cpu.step(a); og = gpu.step(a)
        bad = outputs_differing(oc, og)
        bad += [n for n, k, dt in ENV_BUFS if not bits_equal(cpu.env_buf(n, k, dt), gpu.env_buf(n, k, dt))]
        assert not bad, f"{tag} step {s}: {bad} differ from the fast oracle"
        cmd = cpu.env_buf("COMMANDS", 3)
        resets += int(oc[3].sum())
        resampled += int(((cmd != cmd_before).any(axis=1) & (oc[3] == 0)).sum())
        cmd_before = cmd.copy()
        live += np.abs(cpu.env_buf("REW_TERMS", 32)).sum(axis=0)
    assert cpu.sim.check_errno() == gpu.sim.check_errno() == 0
    return resets, resampled, live


@pytest.mark.parametrize("task", ["walk", "stairs"])
def test_shipped_lists(oracle_lib, hip_lib, blob, task):
    """The walk list (19 terms) and the stairs list (20: base_height and foot_clearance above the terrain, forward_progress among wave 0's terms), 40 steps,
    the episode counters staggered so that envs time out and are reset on every step and others pass a resample step without a reset."""
    cpu, gpu = _pair(oracle_lib, hip_lib, blob, task)
    n = len(cpu.reward_names)
    assert n == (19 if task == "walk" else 20)
    resets, resampled, live = _run(cpu, gpu, 40, 50, 21, task)
    assert resets >= 40, resets
    assert resampled > 0, "a command was resampled outside a reset"
    assert (live[:n] > 0).sum() >= n - 2 and not live[n:].any(), live


def test_jump(oracle_lib, hip_lib, blob):
    """The base env: no term runs in k_env_post_a (the rewards follow the reset, in k_env_post_b_team); the kernel's frame math, termination and statistics do."""
    cpu, gpu = _pair(oracle_lib, hip_lib, blob, "jump")
    resets, _, live = _run(cpu, gpu, 20, 20, 23, "jump")
    assert resets >= 20 and live.any()


FIVE = ["foot_clearance", "feet_stance", "forward_progress", "feet_air_time", "tracking_lin_vel"]


def test_five_terms_stateful_in_the_middle(oracle_lib, hip_lib, blob):
    """Five terms in an order that is not the order of their ids (12, 18, 34, 10, 0), the three stateful ones in the middle with feet_stance AHEAD of
    feet_air_time (it reads the air times of the step before), one worker term on either side: slot != id order, two worker waves with one term, one idle."""

    def mutate(env_cfg, obs_cfg, reward_cfg, command_cfg):
        full = reward_cfg["reward_scales"]
        reward_cfg["reward_scales"] = {n: (full[n] if full.get(n, 0.0) != 0.0 else 0.5) for n in FIVE}

    cpu, gpu = _pair(oracle_lib, hip_lib, blob, "walk", mutate=mutate)
    assert list(cpu.reward_names) == FIVE
    resets, resampled, live = _run(cpu, gpu, 20, 20, 25, "five terms")
    assert resets >= 20 and (live[:5] > 0).all() and not live[5:].any(), live


def test_one_id_twice(oracle_lib, hip_lib, blob):
    """The walk list with dof_vel's entry renamed to dof_acc: one id in two slots with two scales, which no id -> slot table can hold, so the host must send
    every wave through the loop over the list.  Both slots carry the term, each with its own scale."""
    ks = {}

    def edit(f, i):
        names = list(task_cfg("walk", N_ENVS)[2])
        ks["acc"], ks["vel"] = names.index("dof_acc"), names.index("dof_vel")
        i[F("IC_REWARD_ID0") + ks["vel"]] = i[F("IC_REWARD_ID0") + ks["acc"]]
        assert f[F("FC_REWARD_SCALE0") + ks["vel"]] != f[F("FC_REWARD_SCALE0") + ks["acc"]] and f[F("FC_REWARD_SCALE0") + ks["vel"]] != 0.0

    cpu, gpu = _pair(oracle_lib, hip_lib, blob, "walk", edit_icfg=edit)
    resets, resampled, live = _run(cpu, gpu, 20, 20, 27, "one id twice")
    terms = cpu.env_buf("REW_TERMS", 32)
    assert resets >= 20 and terms[:, ks["acc"]].any() and terms[:, ks["vel"]].any()
    assert not np.array_equal(terms[:, ks["acc"]], terms[:, ks["vel"]]), "the two slots have their own scales"
