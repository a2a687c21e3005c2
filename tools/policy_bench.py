#!/usr/bin/env python3
"""Time of ActorCritic.act + evaluate (include/go2sim_policy.h) at the bench batch, next to a plain PyTorch fp32 implementation of the same modules.

    python tools/policy_bench.py [ROWS] [--activation NAME]"""
import argparse, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go2_sim2real_locomotion_rl_amd.capi import load_hip_lib
from go2_sim2real_locomotion_rl_amd.policy import Mlp, flatten_sequential, policy_act

TORCH_ACT = {"elu": torch.nn.ELU, "selu": torch.nn.SELU, "relu": torch.nn.ReLU, "lrelu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid,
             "identity": torch.nn.Identity}
ap = argparse.ArgumentParser()
ap.add_argument("rows", type=int, nargs="?", default=4096)
ap.add_argument("--activation", choices=sorted(TORCH_ACT), default="elu", help="the hidden layers' activation on both sides (include/go2sim_activation.h)")
args = ap.parse_args()

def torch_mlp(dims):
    layers = []
    for l in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[l], dims[l + 1]))
        if l < len(dims) - 2:
            layers.append(TORCH_ACT[args.activation]())
    return torch.nn.Sequential(*layers)

B = args.rows
lib = load_hip_lib()
A, C = [49, 512, 256, 128, 16], [104, 512, 256, 128, 1]
ta, tc = torch_mlp(A), torch_mlp(C)
pa, _ = flatten_sequential({f"n.{k}": v for k, v in ta.state_dict().items()}, "n", 4)
pc, _ = flatten_sequential({f"n.{k}": v for k, v in tc.state_dict().items()}, "n", 4)
ga, gc = Mlp(lib, A, pa, activation=args.activation), Mlp(lib, C, pc, activation=args.activation)
ta, tc = ta.cuda(), tc.cuda()
obs, cobs = torch.randn(B, 49, device="cuda"), torch.randn(B, 104, device="cuda")
std = torch.ones(16, device="cuda")
act = torch.zeros(B, 16, device="cuda"); mean = torch.zeros(B, 16, device="cuda"); val = torch.zeros(B, device="cuda"); lp = torch.zeros(B, device="cuda")
s = torch.cuda.current_stream().cuda_stream
def ours(step):
    policy_act(lib, ga, gc, obs, cobs, std, B, 1, step, False, act, mean, val, lp, stream=s)
def ref(step):
    with torch.no_grad():
        mu = ta(obs); v = tc(cobs)
        d = torch.distributions.Normal(mu, std.expand_as(mu)); a = d.sample(); l = d.log_prob(a).sum(-1)
    return a, v, l
for name, f in (("go2sim policy_act", ours), ("torch fp32 eager", ref)):
    for k in range(20): f(k)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    N = 200
    for k in range(N): f(k)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / N
    flops = 2 * B * (sum(a * b for a, b in zip(A[:-1], A[1:])) + sum(a * b for a, b in zip(C[:-1], C[1:])))
    print(f"{name:22s} {dt * 1e6:8.1f} us / call  ({flops / dt / 1e12:.2f} TFLOP/s fp32, B = {B}, {args.activation})", flush=True)
