#!/usr/bin/env python3
"""Per-kernel ms/step in the landing window (steps W..W+K after the reset) for one or more builds of the library.
usage: transient_probe.py [--warm 5] [--steps 20] [--kind C] lib1.so [lib2.so ...]   (any builds, e.g. build.build_hip_variant(name, flags))"""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_actions
from go2_sim2real_locomotion_rl_amd import capi
from go2_sim2real_locomotion_rl_amd.configs import flatten_walk_cfg, get_walk_cfgs
from go2_sim2real_locomotion_rl_amd.model_blob import pack_model

args = sys.argv[1:]
W, N, kind, B = 5, 20, "C", 4096
while args and args[0].startswith("--"):
    k, v = args[0], args[1]; args = args[2:]
    if k == "--warm": W = int(v)
    elif k == "--steps": N = int(v)
    elif k == "--kind": kind = v
    elif k == "--envs": B = int(v)
dev = torch.device("cuda", 0)
act = make_actions(W + N, B, dev, kind=kind)
print("lib", "dyn collide solve integrate pre post misc total  (ms/step)")
for so in args:
    lib = capi.Go2SimLib(os.path.abspath(so), "go2sim_")
    for rep in range(2):
        sim = capi.Go2Sim(lib, pack_model(), B, 0, 1)
        f, i, _ = flatten_walk_cfg(B, *get_walk_cfgs(), freeze_curriculum=True)
        sim.env_configure(f, i); sim.env_reset()
        obs = torch.zeros(B, 49, device=dev); priv = torch.zeros(B, 104, device=dev); rew = torch.zeros(B, device=dev)
        rst = torch.zeros(B, dtype=torch.uint8, device=dev); to = torch.zeros(B, device=dev)
        sim.enable_timing(True)
        for s in range(W):
            sim.env_step(act[s], obs, priv, rew, rst, to)
        torch.cuda.synchronize(); sim.read_timing(reset=True)
        for s in range(W, W + N):
            sim.env_step(act[s], obs, priv, rew, rst, to)
        torch.cuda.synchronize()
        ms, cnt = sim.read_timing(reset=True)
        del sim
    print(os.path.basename(so), " ".join(f"{m / N:.4f}" for m in ms), "checksum", float(obs.double().sum()), flush=True)
