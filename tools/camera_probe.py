"""Depth-camera throughput of grx.BatchedSim at `--worlds` worlds, one camera, 64 x 64 and 16 x 16 pixels, on the AntMaze and the kitchen model: time per frame of
  (a) render_pose()                 the tile-binned kernel, in both tile shapes (8x8, the default; 16x4)
  (b) render_pose(binning=False)    the same kernel, every tile testing every geom
  (c) ray() on the same pixel fan   one origin and one direction per pixel, the ray tensors built once outside the timed window
  (d) ray() and building the fan    the torch ops that turn the camera pose into [N, H W, 3] origins and directions, every frame
(c) and (d) are the route to a depth image before the camera kernel existed.  With `--leg rgb` the jobs are instead
  (e) render_pose()                 depth alone, the depth kernel
  (f) render_pose(rgb=True)         colour and depth, the shading kernel with a sun
  (g) render_pose(rgb=True, normals=True)
so that (f) / (e) is what the SHADE phase and its stores cost.  The camera hangs above the mean body position of world 0, looks at it, fovy 60; it is placed
with render_pose, which differs from render() only in where thread 0 of a workgroup takes the pose from.  Each figure is the median over `--runs` alternating runs of
`--calls` back-to-back calls between two events, after a warm-up; the spread is (max - min) / median over the runs.  The images of (a) are compared with those of (b) (bits)
and of (c) (hit geoms, depth) before anything is timed.

    python tools/camera_probe.py > profiles/camera_probe.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ray_probe import timed  # noqa: E402


def probe(name, sim, a):
    import numpy as np
    import torch

    sim.step(5)
    torch.cuda.synchronize()
    n = sim.num_worlds
    c = sim.xpos[0].mean(dim=0).cpu().numpy().astype(np.float64)
    eye = c + np.array([1.5, -1.5, 2.0])
    back = (eye - c) / np.linalg.norm(eye - c)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    pos = torch.tensor(eye, dtype=torch.float32, device=sim.device).expand(n, 1, 3).contiguous()
    mat = torch.tensor(np.stack([right, np.cross(back, right), back], axis=1).reshape(9), dtype=torch.float32, device=sim.device).expand(n, 1, 9).contiguous()
    print(f"{name}: {n} worlds, {sim.model.dim('ngeom')} geoms, camera at {np.round(eye, 3).tolist()} looking at {np.round(c, 3).tolist()}, fovy 60; status {sim.status_counts()}")
    for h, w in ((64, 64), (16, 16)):
        t = float(np.tan(np.radians(60.0) / 2))
        rr, cc = torch.meshgrid(torch.arange(h, device=sim.device), torch.arange(w, device=sim.device), indexing="ij")
        local = torch.stack([(2 * (cc + 0.5) / w - 1) * t * w / h, (1 - 2 * (rr + 0.5) / h) * t, -torch.ones_like(rr, dtype=torch.float32)], dim=-1).reshape(-1, 3).float()

        def fan():
            return pos.expand(-1, h * w, -1).contiguous(), (mat.view(n, 1, 3, 3) @ local[None, :, :, None]).squeeze(-1).contiguous()

        out = (torch.empty((n, 1, h, w), device=sim.device), torch.empty((n, 1, h, w), dtype=torch.int32, device=sim.device))
        if a.leg == "rgb":      # what SHADE costs: the shading kernel against the depth kernel alone, on the same poses in the same process
            rgb, nrm = torch.empty((n, 1, h, w, 4), dtype=torch.uint8, device=sim.device), torch.empty((n, 1, h, w, 3), device=sim.device)
            # a palette by geom id (the packaged models were saved without colours), and a sun
            shade = dict(colors=torch.rand((sim.model.dim("ngeom"), 3), generator=torch.Generator().manual_seed(0)).to(sim.device), sun=(0.3, -0.5, -0.8))
            jobs = {"(e) depth alone": lambda: sim.render_pose(pos, mat, 60.0, h, w, out=out[0]),
                    "(f) rgb + depth": lambda: sim.render_pose(pos, mat, 60.0, h, w, rgb=True, out=(out[0], rgb), **shade),
                    "(g) rgb, depth, normal": lambda: sim.render_pose(pos, mat, 60.0, h, w, rgb=True, normals=True, out=(out[0], rgb, nrm), **shade)}
            depth = jobs["(e) depth alone"]().clone()
            same = all(torch.equal(depth, jobs[k]()[0]) for k in ("(f) rgb + depth", "(g) rgb, depth, normal"))
            print(f"  {h} x {w}: depth of (e), (f) and (g) bit-identical: {same}; alpha 255 in {float((rgb[..., 3] == 255).float().mean()):.0%} of the pixels")
        else:
            o, d = fan()
            rout = (torch.empty((n, h * w), device=sim.device), torch.empty((n, h * w), dtype=torch.int32, device=sim.device))
            jobs = {"(a) render 16x4": lambda: sim.render_pose(pos, mat, 60.0, h, w, segmentation=True, out=out, tile="16x4"),
                    "(a) render 8x8": lambda: sim.render_pose(pos, mat, 60.0, h, w, segmentation=True, out=out, tile="8x8"),
                    "(b) no binning": lambda: sim.render_pose(pos, mat, 60.0, h, w, segmentation=True, out=out, binning=False),
                    "(c) ray, fan prebuilt": lambda: sim.ray(o, d, out=rout),
                    "(d) ray + fan": lambda: sim.ray(*fan(), out=rout)}
            depth, seg = (x.clone() for x in jobs["(a) render 16x4"]())
            same = all(torch.equal(x, y) for k in ("(a) render 8x8", "(b) no binning") for x, y in zip((depth, seg), jobs[k]()))
            dist, geom = jobs["(c) ray, fan prebuilt"]()
            agree = geom.view_as(seg) == seg
            err = ((dist.view_as(depth) - depth).abs() / depth.abs().clamp(min=1.0))[agree]
            print(f"  {h} x {w}: (a) 16x4, (a) 8x8 and (b) bit-identical: {same}; (a) vs (c): same geom in {float(agree.float().mean()):.4%} of the pixels, worst relative depth difference there "
                  f"{float(err.max()):.2e}; a geom in {float((seg >= 0).float().mean()):.0%} of the pixels")
        for fn in jobs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in jobs}
        for _ in range(a.runs):
            for k, fn in jobs.items():
                runs[k].append(timed(fn, a.calls))
        for k, v in runs.items():
            v = sorted(v)
            med = v[len(v) // 2]
            print(f"    {k:24s} {med * 1e6:10.1f} us/frame  spread {(v[-1] - v[0]) / med:6.1%}  {n * h * w / med:12.3e} pixels/s")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg", choices=("depth", "rgb"), default="depth", help="depth: (a) - (d); rgb: (e) - (g), the colour kernel against the depth kernel")
    a = ap.parse_args()
    import gymnasium_robotics_amd as grx
    from gymnasium_robotics_amd import _native

    print(f"command: python tools/camera_probe.py --worlds {a.worlds} --calls {a.calls} --runs {a.runs} --warmup {a.warmup} --leg {a.leg}")
    print(f"build id: {_native.build_id()}   device: {torch.cuda.get_device_name(0)}   median of {a.runs} alternating runs of {a.calls} calls each")
    for env_id in ("AntMaze_UMaze-v5", "FrankaKitchen-v1"):
        env = grx.make_vec(env_id, num_envs=a.worlds)
        env.reset(seed=0)
        sim = grx.BatchedSim(env.model, num_worlds=a.worlds, outputs=("xpos", "xquat"))
        sim.qpos.copy_(env.qpos); sim.qvel.copy_(env.qvel)
        try:
            probe(f"{env_id} model", sim, a)
        except ValueError as e:      # a model the ray calls refuse (a mesh without a full hull) is refused here as well
            print(f"{env_id} model: {e}")
        sim.close()
        env.close()


if __name__ == "__main__":
    main()
