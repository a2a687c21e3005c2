"""Env snapshots on the device (include/go2sim_state.h, Go2Env.state_dict / load_state_dict): a continued run and a restored run agree in every bit.

One walk handle of 37 envs (a partial wavefront, no multiple of a team size) steps 30 times, is saved, and steps 40 more times while everything a
step returns is recorded -- the window holds time-outs, falls, command resamples, pushes and curriculum updates (asserted).  The record is then put
back into the same handle, into a second handle that has meanwhile done something else, and into a handle that runs the other executor; each must
replay the recording bit for bit and end in the same state (every go2sim_get_field field, every go2sim_env_get buffer, the globals, the record
itself).  Every env family does the same through Go2Env.  A record that does not belong to a handle is refused and leaves it untouched."""
import copy

import numpy as np
import pytest
import torch

from util import GpuEnv, bits_equal, outputs_differing, task_cfg, with_knobs

pytestmark = pytest.mark.gpu

N, WARM, WINDOW, SEED = 37, 30, 40, 1
PUSH_COLS = slice(100, 103)      # the push force in the walk layout's privileged row: 49 observations, then 3 + 1 + 36 + 1 + 3 + 4 + 3 columns in front of it
ENV_BUFS = [("COMMANDS", 3, np.float32), ("EPISODE_LENGTH", 1, np.int32), ("BASE_LIN_VEL", 3, np.float32), ("BASE_ANG_VEL", 3, np.float32),
            ("PROJECTED_GRAVITY", 3, np.float32), ("DOF_POS", 12, np.float32), ("DOF_VEL", 12, np.float32), ("BASE_POS", 3, np.float32),
            ("BASE_QUAT", 4, np.float32), ("BASE_EULER", 3, np.float32), ("EPISODE_SUMS", 32, np.float32), ("FOOT_CONTACT", 4, np.int32),
            ("FEET_AIR_TIME", 4, np.float32), ("REW_TERMS", 32, np.float32), ("TORQUE", 12, np.float32), ("TERRAIN_ROW", 1, np.int32),
            ("GROUND_HEIGHT", 1, np.float32), ("SPAWN_POS", 3, np.float32), ("TILE_ROW", 1, np.int32), ("TILE_COL", 1, np.int32)]


def fields():
    from go2_sim2real_locomotion_rl_amd.capi import C

    return sorted(k[len("GO2SIM_"):] for k in C if k.startswith("GO2SIM_F_") or k.startswith("GO2SIM_I_"))


def where_records_differ(a, b):
    """the parts of two records (uint8 arrays) that differ, each with its first differing word and the words' count: what a failure message shows"""
    from go2_sim2real_locomotion_rl_amd.capi import C, state_record_parts

    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return [("size", a.size, b.size)]
    n = 4 * C["GO2SIM_STATE_HDR_WORDS"]
    out = [("header", int(i)) for i in np.nonzero(a[:n].view(np.int32) != b[:n].view(np.int32))[0][:4]]
    for name, at, nbytes in state_record_parts(a[:n].view(np.int32)):
        d = np.nonzero(a[at:at + nbytes].view(np.int32) != b[at:at + nbytes].view(np.int32))[0]
        if d.size:
            out.append((name, int(d[0]), int(d.size)))
    return out or [("padding", int(np.nonzero(a != b)[0][0]))] if not np.array_equal(a, b) else []


def busy(env_cfg, obs_cfg, reward_cfg, command_cfg):
    """The walk cfgs with the events of a long run brought into a short one: tight roll / pitch limits (falls), episodes of 15 steps (time-outs),
    commands resampled every 5 steps, a push every 0.2 s from level 0 on, and a curriculum that updates every 6 episodes, moves after one hard update and has room to move."""
    env_cfg.update({"termination_if_roll_greater_than": 8, "termination_if_pitch_greater_than": 8, "episode_length_s": 0.3, "resampling_time_s": 0.1,
                    "push_interval_s": 0.2})
    env_cfg["curriculum"].update({"level_init": 0.5, "update_every_episodes": 6, "hard_streak": 1, "cooldown_updates": 0, "step_down": 0.002,
                                  "push_start": 0.0, "push_interval_easy_s": 0.2})


def make_env(hip_lib, blob, n=N, seed=SEED, task="walk", graph=True, mutate=busy, whole=False):
    with with_knobs({"GO2SIM_GRAPH": "1" if graph else "0", "GO2SIM_STATE_WHOLE": "1" if whole else "0"}):
        env = GpuEnv(hip_lib, blob, n, seed=seed, task=task, mutate=mutate)
    assert env.sim.graph_status()[0] is graph
    env.reset()
    from go2_sim2real_locomotion_rl_amd.capi import C
    max_ep = int(task_cfg(task, n, mutate)[1][C["GO2SIM_IC_MAX_EPISODE_LENGTH"]])
    ep = (np.arange(n) % max_ep).astype(np.int32)                          # the envs' episodes end staggered over the steps
    env.sim.env_set_episode_length(torch.from_numpy(ep).to(env.dev))
    return env


def actions(n_steps, n, n_act, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(n_steps, n, n_act, generator=g)).numpy()


def globals_bytes(env):
    return bytes(env.sim.env_globals())


def save(env):
    rec = torch.empty(env.sim.state_size(), dtype=torch.uint8, device=env.dev)
    env.sim.state_save(rec)
    torch.cuda.synchronize()
    return rec.cpu()


def load(env, rec, nbytes=None):
    rc = env.sim.state_load(rec.to(env.dev), nbytes)
    torch.cuda.synchronize()
    return rc


def end_state(env):
    return {"fields": {f: env.get(f) for f in fields()}, "bufs": {n: env.env_buf(n, k, dt) for n, k, dt in ENV_BUFS}, "globals": globals_bytes(env),
            "record": save(env).numpy()}


@pytest.fixture(scope="module")
def recording(hip_lib, blob):
    """-> the saved env, its record after WARM steps, the window's actions, what every step of the window returned, the end state, the events"""
    env = make_env(hip_lib, blob)
    acts = actions(WARM + WINDOW, N, env.n_act, seed=5)
    for a in acts[:WARM]:
        env.step(a)
    rec, level0 = save(env), env.sim.env_globals().level
    at_save = {"fields": {f: env.get(f) for f in fields()}, "bufs": {n: env.env_buf(n, k, dt) for n, k, dt in ENV_BUFS}, "globals": globals_bytes(env)}
    steps, events = [], dict(resets=0, time_outs=0, falls=0, resamples=0, pushed=0, levels={level0})
    cmd = env.env_buf("COMMANDS", 3)
    for a in acts[WARM:]:
        out = tuple(np.copy(x) for x in env.step(a))
        steps.append((out, globals_bytes(env)))
        rst, to = out[3] != 0, out[4] != 0
        new_cmd = env.env_buf("COMMANDS", 3)
        events["resets"] += int(rst.sum()); events["time_outs"] += int((rst & to).sum()); events["falls"] += int((rst & ~to).sum())
        events["resamples"] += int(((new_cmd != cmd).any(axis=1) & ~rst).sum())
        events["pushed"] += int((out[1][:, PUSH_COLS] != 0).any(axis=1).sum())
        events["levels"].add(env.sim.env_globals().level)
        cmd = new_cmd
    assert env.sim.check_errno() == 0
    return dict(env=env, record=rec, actions=acts[WARM:], steps=steps, end=end_state(env), events=events, at_save=at_save)


def replay(env, recording, tag, same_format=True):
    # right after the load, before any step: the field API, the env buffers and the globals show what the saved handle showed when it was saved
    want = recording["at_save"]
    bad = [f for f in want["fields"] if not bits_equal(env.get(f), want["fields"][f])]
    bad += [n for n, k, dt in ENV_BUFS if not bits_equal(env.env_buf(n, k, dt), want["bufs"][n])]
    assert not bad and globals_bytes(env) == want["globals"], f"{tag}: {bad} differ right after the load"
    for s, (a, (want, want_globals)) in enumerate(zip(recording["actions"], recording["steps"])):
        got = env.step(a)
        bad = outputs_differing(want, got)
        assert not bad, f"{tag} step {s}: {bad} differ from the continued run"
        assert globals_bytes(env) == want_globals, f"{tag} step {s}: the globals differ"
    end, want = end_state(env), recording["end"]
    bad = [f for f in want["fields"] if not bits_equal(end["fields"][f], want["fields"][f])]
    bad += [n for n in want["bufs"] if not bits_equal(end["bufs"][n], want["bufs"][n])]
    assert not bad, f"{tag}: {bad} differ after the window"
    assert end["globals"] == want["globals"]
    assert not same_format or np.array_equal(end["record"], want["record"]), f"{tag}: the records differ after the window: {where_records_differ(end['record'], want['record'])}"
    assert env.sim.check_errno() == 0


def test_round_trip_on_one_handle(recording):
    from go2_sim2real_locomotion_rl_amd.capi import C

    ev = recording["events"]
    print("window:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in ev.items()})
    assert ev["time_outs"] > 0 and ev["falls"] > 0 and ev["resamples"] > 0 and ev["pushed"] > 0, ev
    assert len(ev["levels"]) > 1, "no curriculum level change inside the window"
    env, rec = recording["env"], recording["record"]
    words = rec[:4 * C["GO2SIM_STATE_HDR_WORDS"]].view(torch.int32)
    assert words[C["GO2SIM_STATE_W_MAGIC"]] == C["GO2SIM_STATE_MAGIC"] and words[C["GO2SIM_STATE_W_N_ENVS"]] == N
    assert words[C["GO2SIM_STATE_W_STEP_COUNT"]] == WARM and rec.numel() % 16 == 0
    assert env.sim.env_globals().step_count == WARM + WINDOW
    assert load(env, rec) == 0
    assert env.sim.env_globals().step_count == WARM
    replay(env, recording, "same handle")


def test_into_another_handle(hip_lib, blob, recording):
    other = make_env(hip_lib, blob)
    for a in actions(13, N, other.n_act, seed=77):                          # meanwhile: other actions, another step count
        other.step(1.5 * a)
    assert load(other, recording["record"]) == 0
    replay(other, recording, "second handle")


def test_across_executors(hip_lib, blob, recording):
    plain = make_env(hip_lib, blob, graph=False)
    for a in actions(3, N, plain.n_act, seed=78):
        plain.step(a)
    assert load(plain, recording["record"]) == 0
    replay(plain, recording, "plain launches")
    assert plain.sim.graph_status()[0] is False and recording["env"].sim.graph_status() == (True, 0)


def test_whole_pool_form_agrees_with_the_carried_form(hip_lib, blob, recording):
    """GO2SIM_STATE_WHOLE=1 carries every row and every chunk of the pools, which is correct by construction: the same run saved and restored in that
    form replays the recording of the carried form.  The two forms' records are not interchangeable, and the carried one is the smaller."""
    from go2_sim2real_locomotion_rl_amd.capi import C

    whole = make_env(hip_lib, blob, whole=True)
    for a in actions(WARM + WINDOW, N, whole.n_act, seed=5)[:WARM]:
        whole.step(a)
    rec = save(whole)
    words = lambda r: r[:4 * C["GO2SIM_STATE_HDR_WORDS"]].view(torch.int32)
    w, c = words(rec), words(recording["record"])
    assert w[C["GO2SIM_STATE_W_AF_CARRIED"]] * 4 == w[C["GO2SIM_STATE_W_AF_STRIDE"]] and w[C["GO2SIM_STATE_W_F_CARRIED"]] == w[C["GO2SIM_STATE_W_F_ROWS"]]
    assert c[C["GO2SIM_STATE_W_AF_CARRIED"]] < w[C["GO2SIM_STATE_W_AF_CARRIED"]] and c[C["GO2SIM_STATE_W_AI_CARRIED"]] < w[C["GO2SIM_STATE_W_AI_CARRIED"]]
    print(f"record bytes per env: carried {recording['record'].numel() / N:.0f}, whole pools {rec.numel() / N:.0f}")
    assert recording["record"].numel() < 0.8 * rec.numel()
    assert load(whole, recording["record"]) == C["GO2SIM_E_BADARG"] and load(recording["env"], rec) == C["GO2SIM_E_BADARG"]
    for a in actions(7, N, whole.n_act, seed=79):                            # move on, then come back
        whole.step(a)
    assert load(whole, rec) == 0
    replay(whole, recording, "whole-pool form", same_format=False)


def test_another_heightfield_is_refused(hip_lib, blob):
    """The model digest covers the installed heightfield: a stairs record does not load into a handle whose field differs in one cell."""
    from go2_sim2real_locomotion_rl_amd.capi import C
    from go2_sim2real_locomotion_rl_amd.configs import build_stair_terrain, get_stair_cfgs

    a, b, same = (make_env(hip_lib, blob, task="stairs", mutate=None) for _ in range(3))
    hf, info = build_stair_terrain(get_stair_cfgs()[0]["terrain"])
    hf = hf.copy(); hf[3, 3] += 1
    b.sim.set_terrain(hf, info["horizontal_scale"], info["vertical_scale"], info["terrain_origin"])
    rec = save(a)
    assert rec.numel() == b.sim.state_size()
    assert load(b, rec) == C["GO2SIM_E_BADARG"] and load(same, rec) == 0


REFUSALS = {"37 envs into 38": dict(n=N + 1), "walk into stairs": dict(task="stairs", mutate=None), "seed 1 into seed 2": dict(seed=SEED + 1),
            "short bytes": dict(), "bumped version": dict()}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_handle_untouched(hip_lib, blob, recording, case):
    from go2_sim2real_locomotion_rl_amd.capi import C

    kw = REFUSALS[case]
    target, twin = make_env(hip_lib, blob, **kw), make_env(hip_lib, blob, **kw)
    acts = actions(16, target.B, target.n_act, seed=9)
    for a in acts[:6]:
        target.step(a); twin.step(a)
    rec, nbytes = recording["record"].clone(), None
    if case == "short bytes":
        nbytes = rec.numel() - 16
    elif case == "bumped version":
        rec[:4 * C["GO2SIM_STATE_HDR_WORDS"]].view(torch.int32)[C["GO2SIM_STATE_W_VERSION"]] += 1
    elif case != "37 envs into 38":
        assert rec.numel() == target.sim.state_size(), "same size: the header's words are what refuses it"
    assert load(target, rec, nbytes) == C["GO2SIM_E_BADARG"], case
    for s, a in enumerate(acts[6:]):
        bad = outputs_differing(target.step(a), twin.step(a))
        assert not bad, f"{case}, step {s} after the refusal: {bad} differ from the untouched twin"
    assert globals_bytes(target) == globals_bytes(twin)
    ours, theirs = save(target).numpy(), save(twin).numpy()
    assert np.array_equal(ours, theirs), f"{case}: the state differs from the untouched twin's: {where_records_differ(ours, theirs)}"


# ---- every env family through Go2Env -------------------------------------------------------------------------------------------------------
B_ENV, HALF, ENV_SEED = 24, 20, 11


def family_cfgs(family):
    from go2_sim2real_locomotion_rl_amd import configs as K

    cfgs = {"walk": lambda: K.get_walk_cfgs(), "walk_pls_off": lambda: K.get_walk_cfgs(pls_enable=False), "base": lambda: K.get_crouch_cfgs(),
            "stairs": lambda: K.get_stair_cfgs(), "stairs_lidar": lambda: K.get_stair_lidar_cfgs(), "stairs_info": lambda: K.get_stair_info_cfgs(),
            "rough_heightmap": lambda: K.get_rough_cfgs("heightmap", seed=3), "rough_grid": lambda: K.get_rough_cfgs("grid", seed=3),
            "stairwell": lambda: K.get_stairwell_cfgs(), "walk_engine_gain": lambda: K.get_walk_cfgs(pls_enable=False)}[family]()
    cfgs = copy.deepcopy(cfgs)
    if family == "walk_engine_gain":                                         # engine PD whose motor gains are the batch mean of the gains drawn at each reset call:
        cfgs[0].pop("kp_factor_range"); cfgs[0].pop("kd_factor_range")       # k_env_engine_gains rewrites the device model tables after every step with a reset
    if family != "base":                                                     # falls inside 40 steps, and a curriculum that moves
        cfgs[0].update({"termination_if_roll_greater_than": 10, "termination_if_pitch_greater_than": 10})
        cfgs[0]["curriculum"].update({"update_every_episodes": 4, "hard_streak": 1, "cooldown_updates": 0, "step_down": 0.002})
    if family in ("stairs_lidar", "stairs_info"):                            # DR level 1: the scan's stale rows and blackouts at their full probabilities
        cfgs[0]["curriculum"].update({"level_init": 1.0, "step_down": 0.0})
    return cfgs


def make_family_env(family):
    from go2_sim2real_locomotion_rl_amd import Go2Env, init

    init(seed=ENV_SEED)
    if family == "rough_grid":
        np.random.seed(3)                                                    # the grid's tiles come from numpy's global generator
    env = Go2Env(B_ENV, *family_cfgs(family), seed=ENV_SEED)
    buf = env.episode_length_buf.clone()
    buf[::3] = env.max_episode_length - 8 - torch.arange(0, B_ENV, 3, device=buf.device, dtype=buf.dtype)      # time-outs in both halves
    env.episode_length_buf = buf
    return env


def env_actions(t, n_act, scale=1.5):
    g = torch.Generator().manual_seed(300 + t)
    return (scale * torch.randn(B_ENV, n_act, generator=g)).to("cuda:0")


def ibits(t):
    t = t.detach().contiguous().cpu()
    return t.reshape(-1).view(torch.uint8).numpy().copy()


def flat(x, prefix=""):
    """a nest of dicts / lists / tensors / numbers -> {path: bytes or value}"""
    if isinstance(x, dict):
        return {k2: v for k, v in x.items() for k2, v in flat(v, f"{prefix}{k}.").items()}
    if isinstance(x, (list, tuple)):
        return {k2: v for k, v in enumerate(x) for k2, v in flat(v, f"{prefix}{k}.").items()}
    return {prefix[:-1]: ibits(x) if torch.is_tensor(x) else x}


def differing(a, b):
    a, b = flat(a), flat(b)
    return sorted(set(a) ^ set(b)) + [k for k in a if k in b and not (np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])]


def step_record(env, t):
    obs, rew, reset, extras = env.step(env_actions(t, env.num_actions))
    return {"obs": obs, "critic": extras["observations"]["critic"], "rew": rew.clone(), "reset": reset.clone(), "time_outs": extras["time_outs"].clone(),
            "extras": {k: v for k, v in extras.items() if k not in ("observations", "time_outs")}}


@pytest.mark.parametrize("family", ["walk", "walk_pls_off", "walk_engine_gain", "base", "stairs", "stairs_lidar", "stairs_info", "rough_heightmap", "rough_grid",
                                    "stairwell"])
def test_every_env_family(family):
    env = make_family_env(family)
    for t in range(HALF):
        env.step(env_actions(t, env.num_actions))
    state = env.state_dict()
    assert all(torch.is_tensor(v) and v.device.type == "cpu" or isinstance(v, (int, str)) for v in state.values()), "CPU tensors and plain values only"
    gains0 = [float(v) for v in env.engine_gains]
    rows0 = env._env_view("TERRAIN_ROW", 1, torch.int32).clone()
    want = [step_record(env, t) for t in range(HALF, 2 * HALF)]
    want = [{k: (v if k == "extras" else ibits(v)) for k, v in r.items()} for r in want]
    want = [dict(r, extras=flat(r["extras"])) for r in want]
    end = env.state_dict()

    resets = sum(int(r["reset"].sum()) for r in want)
    assert resets > 0, "no env was reset inside the window"
    n_in = getattr(env, "_lidar_n_in", 0)
    live = [(want[t]["reset"] == 0) & (want[t - 1]["reset"] == 0) for t in range(1, HALF)]
    obs = [r["obs"].view(np.float32).reshape(B_ENV, -1) for r in want]
    if family == "stairs":
        assert not env._lock_terrain_rows and (env._env_view("TERRAIN_ROW", 1, torch.int32) != rows0).any(), "the row curriculum did not move"
    if family == "stairs_lidar":
        scan = [o[:, n_in:].view(np.int32) for o in obs]
        stale = sum(int((l & (scan[t] == scan[t - 1]).all(axis=1) & (scan[t] != 0).any(axis=1)).sum()) for t, l in zip(range(1, HALF), live))
        black = sum(int((l & (scan[t] == 0).all(axis=1)).sum()) for t, l in zip(range(1, HALF), live))
        print(f"{family}: {stale} stale rows, {black} blackouts, {resets} resets")
        assert stale > 0 and black > 0
    if family == "stairs_info":
        # a stale row repeats the stored edge and direction (to an ulp: a divide and a multiply by the scale, include/go2sim_stairinfo.h step 5); fresh
        # noise on the edge makes that a coincidence otherwise; a blackout is the scaled maximum range with direction 0
        cfg = env.env_cfg["stair_info"]
        far = np.float32(np.float32(cfg["edge_detection"]["max_range"]) * np.float32(cfg["edge_dist_scale"]))
        four = [o[:, n_in:n_in + 4] for o in obs]
        near = lambda a, b: np.abs(a - b) <= 4 * np.spacing(np.abs(b))
        stale = sum(int((l & near(four[t][:, 0], four[t - 1][:, 0]) & (four[t][:, 3] == four[t - 1][:, 3]) & (four[t - 1][:, 0] != far)).sum())
                    for t, l in zip(range(1, HALF), live))
        black = sum(int((l & (four[t][:, 0] == far) & (four[t][:, 3] == 0)).sum()) for t, l in zip(range(1, HALF), live))
        print(f"{family}: {stale} stale rows, {black} blackouts, {resets} resets")
        assert stale > 0 and black > 0

    other = make_family_env(family)
    meanwhile = 0
    for t in range(12):                                                       # meanwhile: other actions, falls and time-outs, hence resets with other draws
        meanwhile += int(other.step(env_actions(900 + t, other.num_actions, scale=2.0))[2].sum())
    assert meanwhile > 0, "the second env did not reset before the load"
    if family == "walk_engine_gain":
        assert env._sim.env_globals().engine_kp != gains0[0], "no reset call changed the batch gain inside the window"
        assert [float(v) for v in other.engine_gains] != gains0, "the second env's model tables already hold the saved gains"
    other.load_state_dict(state)
    obs_now, extras_now = other.get_observations()
    assert np.array_equal(ibits(obs_now), ibits(state["obs_buf"])) and np.array_equal(ibits(extras_now["observations"]["critic"]), ibits(state["privileged_obs_buf"] if other.num_privileged_obs else state["obs_buf"]))
    assert not differing(other.state_dict(), state), "a loaded env saves what it loaded"
    for t in range(HALF, 2 * HALF):
        got = step_record(other, t)
        w = want[t - HALF]
        bad = [k for k in ("obs", "critic", "rew", "reset", "time_outs") if not np.array_equal(ibits(got[k]), w[k])]
        bad += differing(got["extras"], w["extras"])
        assert not bad, f"{family} step {t}: {bad} differ from the continued run"
    now = other.state_dict()
    bad = differing(now, end)
    assert not bad, f"{family}: {bad} of state_dict() differ after the window; core: {where_records_differ(now['core'].numpy(), end['core'].numpy())}"
    assert env.check_errno() == 0 and other.check_errno() == 0


def test_load_state_dict_names_what_does_not_match():
    from go2_sim2real_locomotion_rl_amd import Go2Env, Go2SimError, get_stair_cfgs, get_walk_cfgs, init

    init(seed=ENV_SEED)
    walk = Go2Env(B_ENV, *get_walk_cfgs(), seed=ENV_SEED)
    state = walk.state_dict()
    twin = Go2Env(B_ENV, *get_walk_cfgs(), seed=ENV_SEED)
    for env, word in ((Go2Env(B_ENV, *get_stair_cfgs(), seed=ENV_SEED), "family"), (Go2Env(B_ENV + 1, *get_walk_cfgs(), seed=ENV_SEED), "num_envs")):
        with pytest.raises(Go2SimError, match=word):
            env.load_state_dict(state)
    other_seed = Go2Env(B_ENV, *get_walk_cfgs(), seed=ENV_SEED + 1)
    ref_seed = Go2Env(B_ENV, *get_walk_cfgs(), seed=ENV_SEED + 1)
    with pytest.raises(Go2SimError, match="seed"):
        other_seed.load_state_dict(state)
    cfgs = get_walk_cfgs()
    cfgs[2]["reward_scales"]["action_rate"] *= 2.0                            # same family and widths: the configuration digest is what differs
    with pytest.raises(Go2SimError, match="configuration digest"):
        Go2Env(B_ENV, *cfgs, seed=ENV_SEED).load_state_dict(state)
    for t in range(6):                                                        # the refused env steps as one that was never asked
        a = env_actions(t, 16, scale=0.5)
        o1, r1, d1, _ = other_seed.step(a)
        o2, r2, d2, _ = ref_seed.step(a)
        assert np.array_equal(ibits(o1), ibits(o2)) and np.array_equal(ibits(r1), ibits(r2)) and np.array_equal(ibits(d1), ibits(d2)), t
    assert not differing(other_seed.state_dict(), ref_seed.state_dict())
    twin.load_state_dict(state)                                               # and the one it belongs to takes it
    assert not differing(twin.state_dict(), state)
