"""What the sensor block of grx.BatchedSim costs: sim.step(nstep=5) at `--worlds` worlds on the arm scene of tests/sensor_cases.py (the arm scene of tests/sim_cases.py with a
sensor section), without a sensor and with a 10-sensor IMU block (two accelerometers, gyro, framequat, framepos, framelinvel, two joint sensors, actuatorfrc,
jointactuatorfrc: 23 columns).  The two legs alternate (without, with, without, ...); each figure is the median over `--runs` runs of `--calls` back-to-back launches between two
device events, after a warm-up; the spread is (max - min) / median.  There is no parent number for a new block: the figures are recorded (profiles/sim_probe_sensors.txt), not
bounded.  The resource figures of the kernels come from tools/kernel_resources.py.

    python tools/sensor_probe.py > profiles/sim_probe_sensors.txt
    python tools/sensor_probe.py --resources-only        # the table of resource figures alone (no GPU needed)"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
IMU = ("ee_acc", "box_gyro", "box_acc", "ee_quat", "ee_pos", "ee_vel", "j1_pos", "j2_vel", "a1_frc", "j1_afrc")


def timed(fn, calls):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def resources():
    from gymnasium_robotics_amd import _native
    from kernel_resources import kernel_resources

    print("kernel resources (vgpr / agpr / sgpr / scratch B per lane / vgpr spills / sgpr spills), from the library's code objects:")
    rows = []
    for r in kernel_resources(_native.LIB_PATH):
        m = re.search(r"grx_sim_(step|lane)_kernel", r["name"])      # (the names are mangled where the binutils are missing)
        if m:      # the two templates, one instance per unit: told apart by the block list among the template arguments and by the first argument
            blocks = [b for b in ("Dynamics", "Contacts", "Applied", "Sensors") if "GrxSim" + b in r["name"]]
            rows.append((len(blocks), m.group(0) + " <" + (", ".join(blocks) or "no block") + ">", "descriptors" if "GrxModel const*" in r["name"] or "PK8GrxModel" in r["name"] else "slot", r))
    for _, head, kind, r in sorted(rows, key=lambda x: (x[0], x[1].replace("lane", "step"), x[1], x[2])):
        print(f"  {head:66s} {kind:12s} {r['vgpr']:>4} / {r['agpr']:>3} / {r['sgpr']:>4} / {r['scratch']:>5} / {r['spill_v']:>4} / {r['spill_s']:>5}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.resources_only:
        return resources()
    import numpy as np
    import torch

    import gymnasium_robotics_amd as grx
    import sensor_cases as SC
    from gymnasium_robotics_amd import _native
    print(f"command: python tools/sensor_probe.py --worlds {a.worlds} --calls {a.calls} --runs {a.runs} --warmup {a.warmup}")
    print(f"build id: {_native.build_id()}   device: {torch.cuda.get_device_name(0)}   median of {a.runs} alternating runs of {a.calls} launches of step(nstep=5) each")
    sc = SC.SCENES["arm"]
    st = sc.states(a.worlds)
    sims = {"without sensors (grx_sim_step)": grx.BatchedSim(sc.model, a.worlds), f"with {len(IMU)} sensors (grx_sim_step_sns)": grx.BatchedSim(sc.model, a.worlds, sensors=IMU)}
    start = {k: torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).to("cuda") for k in ("qpos", "qvel", "ctrl")}

    def leg(sim):
        for k, v in start.items():      # every run starts from the same state: the two legs do the same physics
            getattr(sim, k).copy_(v.reshape(getattr(sim, k).shape))
        sim.qacc_warmstart.zero_()
        return timed(lambda: sim.step(5), a.calls)

    for sim in sims.values():
        for _ in range(a.warmup):
            sim.step(5)
    torch.cuda.synchronize()
    runs = {k: [] for k in sims}
    for _ in range(a.runs):
        for k, sim in sims.items():
            runs[k].append(leg(sim))
    med = {}
    for k, v in runs.items():
        v = sorted(v)
        med[k] = v[len(v) // 2]
        print(f"  {k:42s} {med[k] * 1e6:10.1f} us/launch  spread {(v[-1] - v[0]) / med[k]:6.1%}  {a.worlds * 5 / med[k]:12.4e} world-substeps/s   status {sims[k].status_counts()}")
    names = list(med)
    print(f"  the block costs {med[names[1]] / med[names[0]] - 1.0:+.1%} of a launch ({sims[names[1]].nsensordata} columns per world; LDS per world {sims[names[0]].lds_bytes} B without, {sims[names[1]].lds_bytes} B with)")
    resources()


if __name__ == "__main__":
    main()
