"""Records the bits tests/test_wells_env_gpu.py's "... keeps the parent build's bits" cases compare against (tests/wells_flag_off.py), with the library
of the tree this file lies in.

    python tools/record_wells_flag_off_golden.py [--out-dir DIR] [--check]

The files in tests/golden/ were recorded on an MI355X from the build of the commit before the stairwell env was added.  With --check the arrays are
compared with the existing files instead of written."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import wells_flag_off as FO
    from go2_sim2real_locomotion_rl_amd.capi import load_hip_lib
    from go2_sim2real_locomotion_rl_amd.model_blob import pack_model

    lib, blob = load_hip_lib(), pack_model()
    os.makedirs(args.out_dir, exist_ok=True)
    bad = []
    for task in FO.TASKS:
        out = FO.run_case(lib, blob, task)
        path = os.path.join(args.out_dir, f"wells_flag_off_{task}.npz")
        if args.check:
            ref = np.load(path)
            bad += [f"{task}:{k}" for k in out if not np.array_equal(out[k], ref[k])]
        else:
            np.savez_compressed(path, **out)
        print(json.dumps({"task": task, "resets": int(out["reset"].sum()), "file": path, "bytes": os.path.getsize(path)}))
    if bad:
        raise SystemExit(f"differs from the recorded bits: {bad}")


if __name__ == "__main__":
    main()
