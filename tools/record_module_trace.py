"""Records what the four policy modules compute under their algorithms, as SHA-256 digests: tests/golden/module_trace.json.

    python tools/record_module_trace.py --out tests/golden/module_trace.json      # needs the GPU; run it twice, the files must be equal

For each of the five pairings (ActorCritic + PPO, ActorCriticRecurrent + PPO, StudentTeacher + Distillation, StudentTeacherRecurrent + Distillation
without and with a recurrent teacher) and the seeds 1 and 7, `trace` drives a synthetic loop without an env: three rollouts of T = 4 steps at B = 3 with
an update after each, fixed rows, rewards and dones from a CPU generator, and between the second and the third rollout one act_inference, one evaluate,
one get_hidden_states, two reset(dones) and a state_dict() -> new module -> load_state_dict() round trip.  The recurrent pairings also run at B = 1.
tests/test_module_core_gpu.py calls `record` and compares every digest; tests/test_module_core.py compares the "init" digests with the pure
initial-state functions of module_core.py."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_OBS, N_PRIV, N_ACT, HIDDEN, H, HT = 5, 7, 3, [6, 4], 4, 5
T, ROLLOUTS, E, G, MINI_BATCHES = 4, 3, 2, 3, 3
SEEDS = (1, 7)
PAIRINGS = ("ActorCritic", "ActorCriticRecurrent", "StudentTeacher", "StudentTeacherRecurrent", "StudentTeacherRecurrent+teacher")


def tensor_digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def state_digest(sd):
    """keys in sorted order, each key's name and its tensor as contiguous bytes"""
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def build(pairing, seed, device):
    """-> (a fresh module, a function that builds its algorithm for B envs)"""
    import go2_sim2real_locomotion_rl_amd as pkg

    if pairing.startswith("ActorCritic"):
        kw = dict(rnn_hidden_size=H) if pairing == "ActorCriticRecurrent" else {}
        policy = getattr(pkg, pairing)(N_OBS, N_PRIV, N_ACT, HIDDEN, HIDDEN, device=device, seed=seed, **kw)
        # the recurrent update's mini-batches are env blocks: one block at B = 1
        alg = lambda B: pkg.PPO(policy, num_learning_epochs=E, num_mini_batches=MINI_BATCHES if B % MINI_BATCHES == 0 else 1, schedule="adaptive", device=device, seed=seed)
    else:
        kw = {}
        if pairing != "StudentTeacher":
            kw = dict(rnn_hidden_dim=H)
            if pairing.endswith("+teacher"):
                kw.update(teacher_recurrent=True, teacher_rnn_hidden_dim=HT)
        policy = getattr(pkg, pairing.split("+")[0])(N_OBS, N_PRIV, N_ACT, HIDDEN, HIDDEN, device=device, seed=seed, **kw)
        alg = lambda B: pkg.Distillation(policy, num_learning_epochs=E, gradient_length=G, device=device)
    return policy, alg


def dones_pattern(B, g):
    """[ROLLOUTS][T][B] float: a done in the last step of the first rollout (the next rollout's entering reset), a step where all are done, one where none
    are; the rest pseudo-random"""
    d = (torch.rand(ROLLOUTS, T, B, generator=g) < 0.3).float()
    d[0, T - 1] = 0.0; d[0, T - 1, 0] = 1.0
    d[1, 1] = 1.0
    d[1, 2] = 0.0
    return d


def trace(pairing, seed, B, device="cuda:0"):
    """-> {"init": digest, "actions": [...], "updates": [...], "between": {...}, "final": digest}"""
    device = torch.device(device)
    policy, make_alg = build(pairing, seed, device)
    out = {"init": state_digest(policy.state_dict()), "actions": [], "updates": [], "between": {}}
    alg = make_alg(B)
    alg.init_storage(B, T, [N_OBS], [N_PRIV], [N_ACT])
    g = torch.Generator().manual_seed(1000 + seed)
    obs = torch.randn(ROLLOUTS, T + 1, B, N_OBS, generator=g).to(device)
    priv = torch.randn(ROLLOUTS, T + 1, B, N_PRIV, generator=g).to(device)
    rewards = torch.randn(ROLLOUTS, T, B, generator=g).to(device)
    dones = dones_pattern(B, g).to(device)
    between = torch.randn(2, B, N_OBS + N_PRIV, generator=g).to(device)
    resets = (torch.rand(2, B, generator=g) < 0.5).float().to(device)
    for r in range(ROLLOUTS):
        if r == 2:
            o, p = between[0, :, :N_OBS].contiguous(), between[1, :, N_OBS:].contiguous()
            out["between"]["act_inference"] = tensor_digest(policy.act_inference(o), policy.action_mean)
            out["between"]["evaluate"] = tensor_digest(policy.evaluate(p))
            if policy.is_recurrent:
                hid = policy.get_hidden_states()
                out["between"]["hidden_states"] = tensor_digest(*[t for hc in hid if hc is not None for t in hc])
            policy.reset(resets[0]); policy.reset(resets[1])
            sd = policy.state_dict()
            twin, _ = build(pairing, seed + 100, device)
            twin.load_state_dict(sd)
            out["between"]["round_trip"] = state_digest(twin.state_dict())
            out["between"]["round_trip_act"] = tensor_digest(twin.act_inference(o))
            policy.load_state_dict(sd)                                         # the set path of a module whose handles exist
            out["between"]["reloaded"] = state_digest(policy.state_dict())
        for t in range(T):
            actions = alg.act(obs[r, t], priv[r, t])
            out["actions"].append(tensor_digest(actions))
            alg.process_env_step(rewards[r, t], dones[r, t], {})
        if hasattr(alg, "compute_returns"):
            alg.compute_returns(priv[r, T])
        ret = alg.update()
        ret = torch.tensor([ret] if isinstance(ret, float) else list(ret), dtype=torch.float64)
        out["updates"].append(tensor_digest(ret, alg.last_stats))
    out["final"] = state_digest(policy.state_dict())
    if policy.is_recurrent:
        hid = policy.get_hidden_states()
        out["final_hidden_states"] = tensor_digest(*[t for hc in hid if hc is not None for t in hc])
    return out


def record(device="cuda:0"):
    """every pairing at the seeds 1 and 7 and B = 3, the recurrent ones also at B = 1: -> {"<pairing>/seed<seed>/B<B>": trace}"""
    out = {}
    for pairing in PAIRINGS:
        for seed in SEEDS:
            for B in (3, 1) if "Recurrent" in pairing else (3,):
                out[f"{pairing}/seed{seed}/B{B}"] = trace(pairing, seed, B, device)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)
