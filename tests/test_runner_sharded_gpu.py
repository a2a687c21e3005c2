"""Two ranks on one card train one policy: two fresh child processes (this file run as a script, never a fork of the pytest process) on cuda:0 with a
gloo group, each with a 32-env walk ``Go2Env(shared_globals=True)`` and an ``OnPolicyRunner`` over the reference's train_cfg (24 steps per env cut
to 4), two iterations.  A third child runs rank 0's shard alone.  The parent waits with a time limit of its own and compares the files the children
write.  The gloo group rehearses the call sequence of the sharded update, not the RCCL transport (DESIGN.md "(e) Multi-GPU")."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS, STEPS, ITERS, SEED = 32, 4, 2, 11
CHILD_LIMIT_S = 150


def train_cfg():
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_cfgs_walk.json")))["train_cfg"]      # the reference's nets and hyper-parameters
    cfg["num_steps_per_env"] = STEPS
    return cfg


def worker(rank, world, port, out_dir):
    from datetime import timedelta

    import torch
    import torch.distributed as dist

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if world > 1:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_walk_cfgs, init
        from go2_sim2real_locomotion_rl_amd.distributed import shard_seed

        torch.cuda.set_device(0)
        init(seed=shard_seed(SEED, rank))
        env = Go2Env(N_ENVS, *get_walk_cfgs(), seed=shard_seed(SEED, rank), shared_globals=True)
        # a few episodes end inside the eight steps, at other steps on each rank: the logged means are not the initial zeros
        ep = env.episode_length_buf.clone()
        ep[:4 - 2 * rank] = int(env.max_episode_length) - 3 - 2 * rank
        env.episode_length_buf = ep
        tag = f"r{rank}" if world > 1 else "solo"
        runner = OnPolicyRunner(env, train_cfg(), log_dir=os.path.join(out_dir, "logs_" + tag))
        assert (runner.group is not None) == (world > 1) and runner.rank == rank
        initial = runner.policy.state_dict()
        first, act = {}, runner.alg.act

        def recording_act(obs, critic_obs):
            a = act(obs, critic_obs)
            first.setdefault("actions", a.detach().cpu().clone())
            first.setdefault("mean", runner.policy.action_mean.detach().cpu().clone())
            return a

        runner.alg.act = recording_act
        log = runner.learn(ITERS)
        opt = runner.alg.optimizer_state_dict()
        # the same input on every rank after training: the means are the parameters', the samples the rank's noise stream's
        probe_obs, probe_cobs = torch.zeros(N_ENVS, 49, device=env.device), torch.zeros(N_ENVS, 104, device=env.device)
        probe = runner.policy.act(probe_obs, probe_cobs).detach().cpu().clone()
        probe_mean = runner.policy.action_mean.detach().cpu().clone()
        assert env.check_errno() == 0
        trained = runner.policy.state_dict()
        reloaded = None
        if world > 1:                                           # load(): every rank reads rank 0's file, then takes rank 0's parameters
            dist.barrier()                                      # the file is there
            runner.alg.update()                                 # move the parameters away from the file's first
            assert not torch.equal(runner.policy.state_dict()["std"], trained["std"])
            runner.load(os.path.join(out_dir, "logs_r0", f"model_{ITERS}.pt"))
            reloaded = runner.policy.state_dict()
            assert runner.current_learning_iteration == ITERS and runner.alg.optimizer_state_dict()["step"] == opt["step"]
        torch.save({"state": trained, "reloaded": reloaded, "initial": initial, "exp_avg": opt["exp_avg"], "exp_avg_sq": opt["exp_avg_sq"], "step": opt["step"],
                    "lr": opt["lr"], "log": log, "first": first, "probe": probe, "probe_mean": probe_mean,
                    "level": float(env.curriculum_level)}, os.path.join(out_dir, tag + ".pt"))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
def test_two_ranks_train_one_policy(tmp_path):
    import numpy as np
    import torch

    port, out = _free_port(), str(tmp_path)
    jobs = [("r0", 0, 2), ("r1", 1, 2), ("solo", 0, 1)]
    procs = []
    for tag, rank, world in jobs:
        logf = open(tmp_path / f"{tag}.log", "w")
        procs.append((tag, subprocess.Popen([sys.executable, os.path.abspath(__file__), str(rank), str(world), str(port), out], stdout=logf,
                                            stderr=subprocess.STDOUT, cwd=ROOT), logf))
    deadline, failed = time.monotonic() + CHILD_LIMIT_S, []
    for tag, p, logf in procs:
        try:
            if p.wait(timeout=max(0.0, deadline - time.monotonic())) != 0:
                failed.append(f"{tag} exited with {p.returncode}")
        except subprocess.TimeoutExpired:
            failed.append(f"{tag} exceeded {CHILD_LIMIT_S} s")
            break
    for tag, p, logf in procs:                                  # nothing is left running, whatever happened
        if p.poll() is None:
            p.kill()
            p.wait()
        logf.close()
    assert not failed, "; ".join(failed) + "\n" + "\n".join(f"--- {tag}\n" + open(tmp_path / f"{tag}.log").read()[-3000:] for tag, _, _ in procs)

    r0, r1, solo = (torch.load(tmp_path / f"{tag}.pt") for tag, _, _ in jobs)
    bits = lambda t: t.contiguous().numpy().view(np.int32)
    # one policy: parameters, Adam's vectors, step count and learning rate are the same bits on both ranks, from rank 0's initial weights on
    for k in r0["state"]:
        assert np.array_equal(bits(r0["state"][k]), bits(r1["state"][k])), k
        assert np.array_equal(bits(r0["initial"][k]), bits(r1["initial"][k])), k
        assert not torch.equal(r0["state"][k], r0["initial"][k]), k
    assert np.array_equal(bits(r0["exp_avg"]), bits(r1["exp_avg"])) and np.array_equal(bits(r0["exp_avg_sq"]), bits(r1["exp_avg_sq"]))
    n_steps = ITERS * train_cfg()["algorithm"]["num_learning_epochs"] * train_cfg()["algorithm"]["num_mini_batches"]
    assert r0["step"] == r1["step"] == n_steps and r0["lr"] == r1["lr"]
    # both logs carry the global means
    assert len(r0["log"]) == len(r1["log"]) == ITERS
    for a, b in zip(r0["log"], r1["log"]):
        for k in ("mean_reward", "mean_episode_length", "learning_rate", "value_loss", "surrogate_loss", "entropy"):
            assert a[k] == b[k], (k, a[k], b[k])
    assert r0["log"][-1]["mean_episode_length"] > 0 and r0["log"][-1]["learning_rate"] == r0["lr"]
    assert r0["log"][-1]["mean_episode_length"] != solo["log"][-1]["mean_episode_length"], "the means are over both shards' episodes"
    assert r0["level"] == r1["level"]                           # one curriculum
    for r in (r0, r1):                                          # load() on both ranks restores the file's parameters
        assert all(np.array_equal(bits(r["reloaded"][k]), bits(r0["state"][k])) for k in r0["state"])
    # rank 0 wrote the checkpoint, rank 1 wrote nothing
    assert sorted(os.listdir(tmp_path / "logs_r0")) == [f"model_{ITERS}.pt"]
    assert not os.path.exists(tmp_path / "logs_r1") or not os.listdir(tmp_path / "logs_r1")
    from go2_sim2real_locomotion_rl_amd.eval_io import read_checkpoint

    ckpt = read_checkpoint(str(tmp_path / "logs_r0" / f"model_{ITERS}.pt"))
    assert ckpt["iter"] == ITERS and all(torch.equal(ckpt["model_state_dict"][k], v) for k, v in r0["state"].items())
    # the noise streams are per rank: the first actions differ, and on the same input after training the means agree bit for bit while the samples differ
    assert not torch.equal(r0["first"]["actions"] - r0["first"]["mean"], r1["first"]["actions"] - r1["first"]["mean"])
    assert not torch.equal(r0["first"]["actions"], r1["first"]["actions"])
    assert np.array_equal(bits(r0["probe_mean"]), bits(r1["probe_mean"])) and not torch.equal(r0["probe"], r1["probe"])
    # the gradient is the union's: rank 0's shard trained alone starts from the same weights and ends elsewhere
    for k in r0["state"]:
        assert np.array_equal(bits(solo["initial"][k]), bits(r0["initial"][k])), k
    assert all(not torch.equal(solo["state"][k], r0["state"][k]) for k in r0["state"])


if __name__ == "__main__":
    worker(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
