"""Writes tests/golden/dyn_tree_errors.json: per case of tests/dyn_tree_cases.py and per field the worst error of the oracle, the lane emulator and the MI355X against the
reference of tests/dyn_refs.py, next to the reference's own error estimate and its sensitivity to a one-ulp jitter of the start.  The figures are a record and never a bound:
the tests take their bounds from the reference's estimate, from engine_matrix_cases.BOUND and from tests/golden/sim_dynamics_errors.json.

    python tools/measure_dyn_trees.py                    # reference, oracle and emulator, here
    python tools/measure_dyn_trees.py --gpu LOG          # also the device's figures, read from the output of
                                                         # pytest -m gpu -s tests/test_gpu_dyn_trees.py (the "dyn-tree <case> n=<n>: field value ..." lines)
"""
import json
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

PATH = os.path.join(ROOT, "tests", "golden", "dyn_tree_errors.json")

import dyn_tree_cases as T  # noqa: E402
import engine_matrix_cases as C  # noqa: E402
from test_cpu_dyn_trees import CEILING, compare_oracle, emulate  # noqa: E402

r2 = lambda x: float("%.2e" % x)


def main(argv):
    gpu = {}
    if "--gpu" in argv:
        for line in open(argv[argv.index("--gpu") + 1]):
            m = re.search(r"dyn-tree ([\w-]+) n=(\d+): (.*)", line)
            if m:
                words = m.group(3).split()
                gpu[f"{m.group(1)}/{m.group(2)}"] = {k: r2(float(v)) for k, v in zip(words[0::2], words[1::2])}
    old = json.load(open(PATH))["cases"] if os.path.exists(PATH) else {}
    cases = {}
    for name, n in T.RUNS:
        key = f"{name}/{n}"
        case = T.CASES[name]
        fig = compare_oracle(name, n)
        rec = {"bodies": len(case.bodies), "compiled_bodies": case.model.dim("nbody"), "nv": case.model.dim("nv"),
               "reference_estimate": {k: r2(v[2]) for k, v in fig.items()}, "oracle": {k: r2(v[0]) for k, v in fig.items()},
               "oracle_share_of_bound": {k: r2(v[1]) for k, v in fig.items()}, "emulator": {k: r2(v) for k, v in emulate(name, n).items()},
               "reference_sensitivity": {k: r2(v.max()) for k, v in T.reference_sensitivity(name, n).items()}}
        if key in gpu:
            rec["mi355x"] = gpu[key]
        elif "mi355x" in old.get(key, {}):
            rec["mi355x"] = old[key]["mi355x"]
        cases[key] = rec
        print(key, rec, flush=True)
    with open(PATH, "w") as f:
        json.dump({"draws": T.DRAWS, "sens_max": C.SENS_MAX, "bound": C.BOUND, "oracle_ceiling": CEILING, "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
