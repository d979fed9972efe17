"""Ray-casting throughput of grx.BatchedSim (ray / ray_sites) at `--worlds` worlds: time per call and rays per second for R in {1, 16, 64, 256} rays per world, on the arm
scene of tests/sim_cases.py (2 geoms) and on the AntMaze model tools/sim_probe.py uses (many wall boxes), next to the time of sim.step(nstep=5) on the same simulation --
what a scan costs relative to the step it follows.  Each figure is the median over `--runs` alternating runs (step, then each R in turn, again and again) of `--calls`
back-to-back calls between two events, after a warm-up; the spread is (max - min) / median over the runs.  There is no parent to compare the ray kernel with: the numbers
are recorded (profiles/ray_probe.txt), not bounded.

    python tools/ray_probe.py > profiles/ray_probe.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RS = (1, 16, 64, 256)


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def probe(name, sim, a):
    import numpy as np
    import torch

    # cast from a site on a moving body where the model has one (its own body is then skipped, the rangefinder rule); a model whose sites all sit on the world body casts
    # from one of those WITHOUT the exclusion, which would otherwise skip the floor and every wall: both kinds of call then scan every geom
    body = np.asarray(sim.model.tables["site_bodyid"]).reshape(-1)
    names = sorted(sim.model.names["site"], key=lambda n: (body[sim.model.names["site"][n]] == 0, n))
    site, own = names[0], bool(body[sim.model.names["site"][names[0]]] != 0)

    sim.step(5)
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(0)
    jobs = {"step(nstep=5)": lambda: sim.step(5)}
    for r in RS:
        # a fan about the site: directions in its horizontal plane and below, origins at the site (world rays: the same, built once from the current site frames)
        ang = torch.linspace(0, 2 * np.pi, r + 1)[:r]
        local = torch.stack([torch.cos(ang), torch.sin(ang), -0.3 * torch.rand(r, generator=g)], dim=1).to(sim.device)
        sid = sim.site_id(site)
        o = sim.site_xpos[:, sid:sid + 1].expand(-1, r, -1).contiguous()
        d = (sim.site_xmat[:, sid].view(-1, 1, 3, 3) @ local[None, :, :, None]).squeeze(-1).contiguous()
        out = (torch.empty((sim.num_worlds, r), device=sim.device), torch.empty((sim.num_worlds, r), dtype=torch.int32, device=sim.device))
        jobs[f"ray R={r}"] = lambda o=o, d=d, out=out: sim.ray(o, d, out=out)
        jobs[f"ray_sites R={r}"] = lambda local=local, out=out, r=r: sim.ray_sites([site] * r, local, exclude_own_body=own, out=out)
    for fn in jobs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in jobs}
    for _ in range(a.runs):
        for k, fn in jobs.items():
            runs[k].append(timed(fn, a.calls))
    _, geom = sim.ray_sites([site] * 64, exclude_own_body=own, local_dir=torch.stack([torch.cos(torch.linspace(0, 6.2, 64)), torch.sin(torch.linspace(0, 6.2, 64)), torch.zeros(64)], dim=1).to(sim.device))
    torch.cuda.synchronize()
    print(f"{name}: {sim.num_worlds} worlds, {sim.model.dim('ngeom')} geoms, site {site!r} on body {int(body[sim.model.names['site'][site]])}, exclude_own_body={own}; a level fan of 64 hits a geom in {float((geom >= 0).float().mean()):.0%} of its rays; status {sim.status_counts()}")
    for k, v in runs.items():
        v = sorted(v)
        med = v[len(v) // 2]
        r = int(k.split("=")[-1]) if k.startswith("ray") else 0
        rate = f"{sim.num_worlds * r / med:14.3e} rays/s" if r else " " * 21
        print(f"  {k:18s} {med * 1e6:10.1f} us/call  spread {(v[-1] - v[0]) / med:6.1%}  {rate}")


def main():
    import numpy as np
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import gymnasium_robotics_amd as grx
    import sim_cases as S
    from gymnasium_robotics_amd import _native

    print(f"command: python tools/ray_probe.py --worlds {a.worlds} --calls {a.calls} --runs {a.runs} --warmup {a.warmup}")
    print(f"build id: {_native.build_id()}   device: {torch.cuda.get_device_name(0)}   median of {a.runs} alternating runs of {a.calls} calls each")
    outputs = ("xpos", "xquat", "site_xpos", "site_xmat")
    sc = S.SCENES["arm"]
    st = sc.states(a.worlds)
    arm = grx.BatchedSim(sc.model, num_worlds=a.worlds, outputs=outputs)
    for k in ("qpos", "qvel", "ctrl"):
        getattr(arm, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)))
    probe("arm scene", arm, a)
    arm.close()
    env = grx.make_vec("AntMaze_UMaze-v5", num_envs=a.worlds)
    env.reset(seed=0)
    if not env.model.dim("nsite"):
        print("AntMaze_UMaze model: no site in the compiled model, nothing to cast from")
        return
    ant = grx.BatchedSim(env.model, num_worlds=a.worlds, outputs=outputs)
    ant.qpos.copy_(env.qpos); ant.qvel.copy_(env.qvel)
    ant.ctrl.copy_(torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (a.worlds, ant.nu)).astype(np.float32)))
    probe("AntMaze_UMaze model", ant, a)


if __name__ == "__main__":
    main()
