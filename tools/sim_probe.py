"""Throughput of grx.BatchedSim (the generic engine kernel behind grx_sim_step) in env-steps/s: the arm scene of tests/sim_cases.py at `--worlds` worlds, one env-step =
`--nstep` substeps, beside the AntMaze model stepped through the same door (same kernel, AntMaze's own table capacities and frame_skip).  One run, no repetition: a figure to
size expectations by, not a benchmark (bench.py measures the flagship workload).

    python tools/sim_probe.py --worlds 4096 --steps 200 --warmup 20 > profiles/sim_probe.txt

--outputs (comma-separated names of sim.OUTPUTS, or `all`) replaces the arm scene's default pair, --jac-sites names the sites of its Jacobian outputs:
profiles/sim_probe_dynamics.txt.  --model-params (comma-separated names of sim.PARAMS, or `all`) gives both simulations per-world model parameters, left at
their nominal values and committed: the launches then run the kernels that read each world's own descriptor and records (profiles/sim_probe_params.txt).
--contacts (comma-separated names of sim.CONTACTS, or `all`) makes both simulations write the contact list: the launches then run the kernels of the contact units
(profiles/sim_probe_contacts.txt).  --applied gives both simulations the applied-force block (qfrc_applied, xfrc_applied, xipos) and fills both input rows with small
non-zero values: the launches then run the kernels of the applied-force units (profiles/sim_probe_applied.txt).  --applied NAMES (comma-separated names of sim.APPLIED) names only
those: `--applied xipos` runs the same kernels with both input pointers null, which is what the kernels cost without the accumulation stage.  --applied-scale S (default 0.01: N, N m) scales the values: 0 runs the stage on zero rows, which leaves the
physics -- and with it the solver's iteration counts -- where it is without the block."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(sim, nstep, steps, warmup):
    import torch

    for _ in range(warmup):
        sim.step(nstep)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        sim.step(nstep)
    e1.record()
    torch.cuda.synchronize()
    return sim.num_worlds * steps / (e0.elapsed_time(e1) * 1e-3)


def main():
    import numpy as np
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--nstep", type=int, default=5)
    ap.add_argument("--outputs", default="site_xpos,site_xvelp")
    ap.add_argument("--jac-sites", default="")
    ap.add_argument("--model-params", default="")
    ap.add_argument("--contacts", default="")
    ap.add_argument("--applied", nargs="?", const="all", default="")
    ap.add_argument("--applied-scale", type=float, default=0.01)
    a = ap.parse_args()
    import gymnasium_robotics_amd as grx
    import sim_cases as S
    from gymnasium_robotics_amd import _native

    from gymnasium_robotics_amd.sim import APPLIED, CONTACTS, OUTPUTS, PARAMS

    params = PARAMS if a.model_params == "all" else tuple(p for p in a.model_params.split(",") if p)
    kw = dict(model_params=params) if params else {}
    contacts = CONTACTS if a.contacts == "all" else tuple(c for c in a.contacts.split(",") if c)
    if contacts:
        kw["contacts"] = contacts
    applied = APPLIED if a.applied == "all" else tuple(x for x in a.applied.split(",") if x)
    if applied:
        kw["applied"] = applied

    def fill_applied(sim):      # small against the weights and actuator forces of both models: the worlds stay where they are, the stage does real arithmetic
        g = torch.Generator(device="cpu").manual_seed(1)
        for k in ("qfrc_applied", "xfrc_applied"):
            if k in applied:
                getattr(sim, k).copy_(a.applied_scale * torch.randn(getattr(sim, k).shape, generator=g))

    outputs = OUTPUTS if a.outputs == "all" else tuple(o for o in a.outputs.split(",") if o)
    jac = tuple(s for s in a.jac_sites.split(",") if s) or None
    print(f"command: python tools/sim_probe.py --worlds {a.worlds} --steps {a.steps} --warmup {a.warmup} --nstep {a.nstep} --outputs {a.outputs}" + (f" --jac-sites {a.jac_sites}" if jac else "") +
          (f" --model-params {a.model_params}" if params else "") + (f" --contacts {a.contacts}" if contacts else "") + (f" --applied{'' if a.applied == 'all' else ' ' + a.applied}" + (f" --applied-scale {a.applied_scale:g}" if a.applied_scale != 0.01 else "") if applied else ""))
    print(f"build id: {_native.build_id()}   device: {torch.cuda.get_device_name(0)}   SINGLE RUN")
    sc = S.SCENES["arm"]
    st = sc.states(a.worlds)
    arm = grx.BatchedSim(sc.model, num_worlds=a.worlds, outputs=outputs, **(dict(jac_sites=jac) if jac else {}), **kw)
    for k in ("qpos", "qvel", "ctrl"):
        getattr(arm, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)))
    if params:
        arm.commit_params()
    if applied:
        fill_applied(arm)
    rate = timed(arm, a.nstep, a.steps, a.warmup)
    print(f"arm scene (nv 10, 4 plane contacts)   {a.worlds} worlds x {a.nstep} substeps: {rate:12.0f} env-steps/s   LDS/world {arm.lds_bytes} B   status {arm.status_counts()}")
    env = grx.make_vec("AntMaze_UMaze-v5", num_envs=a.worlds)
    env.reset(seed=0)
    ant = grx.BatchedSim(env.model, num_worlds=a.worlds, outputs=("site_xpos", "site_xvelp") if env.model.dim("nsite") else (), **kw)
    ant.qpos.copy_(env.qpos); ant.qvel.copy_(env.qvel)
    ant.ctrl.copy_(torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (a.worlds, ant.nu)).astype(np.float32)))
    if params:
        ant.commit_params()
    if applied:
        fill_applied(ant)
    rate = timed(ant, a.nstep, a.steps, a.warmup)
    print(f"AntMaze_UMaze model (RK4, generic kernel) {a.worlds} worlds x {a.nstep} substeps: {rate:12.0f} env-steps/s   LDS/world {ant.lds_bytes} B   status {ant.status_counts()}")


if __name__ == "__main__":
    main()
