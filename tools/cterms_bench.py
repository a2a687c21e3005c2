#!/usr/bin/env python
"""Times the contact-terms launch (include/go2sim_cterms.h) on the GPU, at the stair-info task's training shape.

    python tools/cterms_bench.py [--envs 4096] [--steps 24] [--rounds 10] [--calls 2000]

Two timings, both taken in one process with the variants alternating round by round, so that other work on the machine hits all alike:

  (a) the closed collection loop (act, env.step, process_env_step for --steps env steps of an OnPolicyRunner at --envs) on the stair-info env with
      the script's own values and body_contact on (`collect_ms_on`: one more launch per env step) and on the same env without the key
      (`collect_ms_off`: the launches the env ran before the term existed);
  (b) the call alone on the env's own contact-force field, --calls calls back to back: `cterms_step_us` with body_contact alone, and
      `cterms_step_both_us` with stumble on as well (nine more links read).

Device events bracket each round; every shape is warmed up first.  Prints one JSON line; the difference of (a) is reported next to the rounds' spread
(max - min of each variant), which says whether it can be told from noise."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from stairinfo_bench import collect, timed  # noqa: E402


def make_runner(body_contact, envs, steps, seed=3):
    from go2_sim2real_locomotion_rl_amd import Go2Env, OnPolicyRunner, get_stair_info_cfgs, init

    init(seed=seed)
    cfgs = copy.deepcopy(get_stair_info_cfgs(script_values=True))
    if not body_contact:
        del cfgs[2]["reward_scales"]["body_contact"]
    env = Go2Env(envs, *cfgs, seed=seed)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_cfgs_stairs.json")))["train_cfg"]
    cfg["num_steps_per_env"] = steps
    return OnPolicyRunner(env, cfg)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=10, help="timed rollouts per variant of (a) and timed rounds of (b)")
    ap.add_argument("--calls", type=int, default=2000, help="calls per round of (b)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cterms_bench.py needs a ROCm GPU (nothing is measured without one)")
    from go2_sim2real_locomotion_rl_amd.contact_terms import ContactTerms, resolve_body_links

    B, T = args.envs, args.steps
    med = lambda v: sorted(v)[len(v) // 2]
    mm = lambda v, nd: [round(min(v), nd), round(max(v), nd)]

    # (a) the closed collection loop
    runners = {"on": make_runner(True, B, T), "off": make_runner(False, B, T)}
    assert runners["on"].env._cterms is not None and runners["off"].env._cterms is None
    ms = {k: [] for k in runners}
    for r in runners.values():
        collect(r, T)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, r in runners.items():
            ms[k].append(timed(lambda: collect(r, T)))

    # (b) the call alone, on the env's own pool
    env = runners["on"].env
    both = ContactTerms(B, body_links=resolve_body_links(), body_contact_scale=-2.0, stumble_scale=-1.0, device=env.device)
    rew, count = torch.zeros(B, device=env.device), torch.zeros(B, device=env.device)
    a = (env._contact_force_ptr, (B, 3 * B, 1), env.reset_buf, rew, count)
    sides = {"body": lambda: env._cterms.step(*a), "both": lambda: both.step(*a)}
    us = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in sides.items():
            us[k].append(timed(lambda: [fn() for _ in range(args.calls)]) * 1e3 / args.calls)

    diff_us = (med(ms["on"]) - med(ms["off"])) * 1e3 / T
    spread_us = max(max(v) - min(v) for v in ms.values()) * 1e3 / T
    out = {"tool": "cterms_bench", "envs": B, "steps": T, "rounds": args.rounds, "calls_per_round": args.calls}
    for k in runners:
        out[f"collect_ms_{k}"], out[f"collect_ms_{k}_min_max"] = round(med(ms[k]), 3), mm(ms[k], 3)
    out.update({"on_minus_off_us_per_env_step": round(diff_us, 2), "rounds_spread_us_per_env_step": round(spread_us, 2),
                "difference_exceeds_spread": bool(abs(diff_us) > spread_us),
                "cterms_step_us": round(med(us["body"]), 2), "cterms_step_us_min_max": mm(us["body"], 2),
                "cterms_step_both_us": round(med(us["both"]), 2), "cterms_step_both_us_min_max": mm(us["both"], 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
