"""What mesh="triangles" costs next to mesh="hull" ("Cameras"): render(64 x 64) of the 4096-triangle torus scene of tests/trimesh_cases.py (without the mesh geom
the hull path refuses) at 4096 worlds, one camera above the torus, both paths in one process, alternating, device events around `reps` launches.  Also the triangle kernel's
A/B switches: a per-lane walk instead of the wave walk (GRX_TRIMESH_WALK=lane), and, on the 256-triangle torus, whose hierarchy fits the LDS window, global nodes instead
(GRX_TRIMESH_WINDOW=0).  The switches are read when a simulation's triangle handle is made, so each variant is a simulation of its own.

    python tools/trimesh_probe.py --out profiles/trimesh_render.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    import camera_cases as K
    import gymnasium_robotics_amd as grx
    import trimesh_cases as T
    from gymnasium_robotics_amd import _native

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    rng = np.random.default_rng(0)
    doc = dict(device=torch.cuda.get_device_name(0), build_id=_native.build_id(), worlds=a.worlds, image=[a.side, a.side], reps=a.reps, rounds=a.rounds,
               unit="microseconds per render() call: the median over the rounds of (device-event time of `reps` launches) / reps; spread: (max - min) / median over the rounds")

    def variants(name, kinds):
        sims = {}
        for kind, env in kinds:
            for k in ("GRX_TRIMESH_WALK", "GRX_TRIMESH_WINDOW"):
                os.environ.pop(k, None)
            os.environ.update(env)
            sim = grx.BatchedSim(T.model(name, spare=False), num_worlds=a.worlds, outputs=("xpos", "xquat"))
            q = np.tile(T.Q0[0, :7], (a.worlds, 1))
            q[:, :3] += rng.uniform(-0.1, 0.1, (a.worlds, 3))
            q[:, 3:7] += rng.uniform(-0.3, 0.3, (a.worlds, 4))      # every world its own pose
            sim.qpos.copy_(torch.from_numpy(q.astype(np.float32)))
            sim.forward()
            at = sim.xpos[:, 1].cpu().numpy().astype(np.float64)
            pos = (at + [0.15, -0.2, 0.9])[:, None]
            mat = np.array([K.look_at(p[0], c) for p, c in zip(pos, at)])[:, None]
            pos, mat = (torch.tensor(x, dtype=torch.float32, device=sim.device) for x in (pos, mat))
            out = (torch.empty((a.worlds, 1, a.side, a.side), device=sim.device), torch.empty((a.worlds, 1, a.side, a.side), dtype=torch.int32, device=sim.device))
            mesh = "hull" if kind == "hull" else "triangles"
            sims[kind] = (sim, lambda sim=sim, pos=pos, mat=mat, out=out, mesh=mesh: sim.render_pose(pos, mat, 60.0, a.side, a.side, segmentation=True, out=out, mesh=mesh))
            sims[kind][1]()      # warm-up: the code object, the planes / the triangle upload
        torch.cuda.synchronize()
        times = {k: [] for k in sims}
        for _ in range(a.rounds):      # alternating
            for k, (_, call) in sims.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.reps):
                    call()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(1e3 * t0.elapsed_time(t1) / a.reps)
        res = {k: dict(us=round(float(np.median(v)), 1), spread=round(float((max(v) - min(v)) / np.median(v)), 3)) for k, v in times.items()}
        seg = {k: int((sims[k][1]()[1] == 3).sum()) for k in sims}      # pixels that show the torus: the hull fills its hole
        torch.cuda.synchronize()
        for k in sims:
            res[k]["torus_pixels"] = seg[k]
            sims[k][0].close()
        return res

    doc["torus_64x32"] = variants("torus64", (("hull", {}), ("triangles", {}), ("triangles_lane_walk", {"GRX_TRIMESH_WALK": "lane"}), ("triangles_no_window", {"GRX_TRIMESH_WINDOW": "0"})))
    doc["torus_64x32"]["triangles_over_hull"] = round(doc["torus_64x32"]["triangles"]["us"] / doc["torus_64x32"]["hull"]["us"], 2)
    doc["torus_16x8"] = variants("torus16", (("hull", {}), ("triangles", {}), ("triangles_lane_walk", {"GRX_TRIMESH_WALK": "lane"}), ("triangles_no_window", {"GRX_TRIMESH_WINDOW": "0"})))
    doc["torus_16x8"]["triangles_over_hull"] = round(doc["torus_16x8"]["triangles"]["us"] / doc["torus_16x8"]["hull"]["us"], 2)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
