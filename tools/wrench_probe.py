"""What the body-wrench block of grx.BatchedSim costs: sim.step(nstep) at `--worlds` worlds on the arm scene of tests/sensor_cases.py with the 10-sensor IMU block of
tools/sensor_probe.py, without the block (the launch of the sensor units, whose code objects a change of this block must leave byte-identical to the parent commit's:
tools/compare_code_objects.py) and with all four outputs (the launch of the wrench units), at 5 and at 20 substeps.  The block is paid once per launch, in its last pass, so the
added time should not depend on the substep count.  The legs alternate (without, with, without, ...); each figure is the median over `--runs` runs of `--calls` back-to-back
launches between two device events, after a warm-up; the spread is (max - min) / median.

    python tools/wrench_probe.py > profiles/sim_probe_wrench.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def main():
    import numpy as np
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import gymnasium_robotics_amd as grx
    import sensor_cases as SC
    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd.sim import BODY_DYNAMICS
    from sensor_probe import IMU, timed

    print(f"command: python tools/wrench_probe.py --worlds {a.worlds} --calls {a.calls} --runs {a.runs} --warmup {a.warmup}")
    print(f"build id: {_native.build_id()}   device: {torch.cuda.get_device_name(0)}")
    sc = SC.SCENES["arm"]
    st = sc.states(a.worlds)
    legs = {"sensors only (sensor units)": dict(sensors=IMU), "sensors + cfrc_ext, cfrc_int, cacc, subtree_com (wrench units)": dict(sensors=IMU, body_dynamics=BODY_DYNAMICS)}
    for nstep in (5, 20):
        sims = {}
        for name, kw in legs.items():
            sims[name] = sim = grx.BatchedSim(sc.model, num_worlds=a.worlds, **kw)
            for k in ("qpos", "qvel", "ctrl"):
                getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)))
            timed(lambda: sim.step(nstep), a.warmup)
        times = {name: [] for name in legs}
        for _ in range(a.runs):
            for name, sim in sims.items():
                times[name].append(timed(lambda: sim.step(nstep), a.calls))
        med = {name: float(np.median(t)) for name, t in times.items()}
        for name, t in times.items():
            print(f"step(nstep={nstep:2d}) {a.worlds} worlds  {name:66s} median {med[name] * 1e6:8.1f} us   spread {(max(t) - min(t)) / med[name] * 100:5.2f} %   status {sims[name].status_counts()}")
        base, full = (med[name] for name in legs)
        print(f"step(nstep={nstep:2d}) the block adds {(full - base) * 1e6:7.1f} us per launch ({(full / base - 1) * 100:5.2f} %)")
        for sim in sims.values():
            sim.close()


if __name__ == "__main__":
    main()
