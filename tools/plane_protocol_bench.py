"""FPS of the reference's `go2` and `anymal` rigid benchmarks (tests/test_rigid_benchmarks.py:316-412) run through the Genesis shim
(`import genesis as gs`) on gs.morphs.Plane() and on the plane.urdf box ground, in one process, alternating.  dt 0.01 with one substep per
scene.step, step-counted warm-up and record; FPS = steps x n_envs / elapsed.

    python tools/plane_protocol_bench.py [--envs 4096] [--warmup 200] [--steps 1000] [--repeats 2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_scene(gs, robot, ground, n_envs):
    import torch

    scene = gs.Scene(sim_options=gs.options.SimOptions(dt=0.01, substeps=1), rigid_options=gs.options.RigidOptions(dt=0.01), show_viewer=False)
    scene.add_entity(gs.morphs.Plane() if ground == "plane" else gs.morphs.URDF(file="urdf/plane/plane.urdf", fixed=True))
    if robot == "go2":
        r = scene.add_entity(gs.morphs.URDF(file="urdf/go2/urdf/go2.urdf"), vis_mode="collision")
        scene.build(n_envs=n_envs)
        ctrl_pos = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.8, 0.8, 1.0, 1.0, -1.5, -1.5, -1.5, -1.5], dtype=gs.tc_float, device=gs.device)
        r.control_dofs_position(ctrl_pos, dofs_idx_local=slice(6, None))
        init_qpos = torch.tensor([[0.0, 0.0, 0.42, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.8, 0.8, 1.0, 1.0, -1.5, -1.5, -1.5, -1.5]],
                                 dtype=gs.tc_float, device=gs.device).repeat((scene.n_envs, 1))
        lo, hi = r.get_dofs_limit()
        init_qpos[:, 7:] = lo[6:] + (hi[6:] - lo[6:]) * torch.rand((scene.n_envs, r.n_dofs - 6), dtype=gs.tc_float, device=gs.device)
        r.set_qpos(init_qpos)
    else:
        r = scene.add_entity(gs.morphs.URDF(file="urdf/anymal_c/urdf/anymal_c.urdf", pos=(0, 0, 0.8)))
        scene.build(n_envs=n_envs)
        r.set_dofs_kp(1000.0, slice(6, None))
        r.control_dofs_position(0.0, slice(6, None))
    return scene


def run(gs, robot, ground, n_envs, warm, steps):
    import torch

    scene = build_scene(gs, robot, ground, n_envs)
    for _ in range(warm):
        scene.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        scene.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    err = scene._sim.check_errno()
    del scene
    return n_envs * steps / dt, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    import torch

    import genesis as gs

    gs.init(backend=gs.gpu)
    out = {"n_envs": a.envs, "warmup_steps": a.warmup, "steps": a.steps, "unit": "FPS = scene steps (dt 0.01, 1 substep) x n_envs / s",
           "device": torch.cuda.get_device_name(0)}
    for robot in ("go2", "anymal_c"):
        res = {"plane": [], "plane_urdf": []}
        for _ in range(a.repeats):
            for ground in ("plane", "plane_urdf"):
                fps, err = run(gs, robot, ground, a.envs, a.warmup, a.steps)
                if err:
                    raise SystemExit(f"{robot} on {ground}: errno {err}")
                res[ground].append(round(fps, 1))
        out[robot] = {g: {"fps_runs": v, "fps_max": max(v)} for g, v in res.items()}
        print(f"{robot}: gs.morphs.Plane {max(res['plane']):,.0f} FPS | plane.urdf box {max(res['plane_urdf']):,.0f} FPS", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
