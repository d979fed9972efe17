"""Writes tests/golden/engine_matrix.json, the record behind the caps of the engine-matrix tests (tests/engine_matrix_cases.py): per group the number of cases the
ORACLE ALONE classifies as well-posed (jitter sensitivity below SENS_MAX at DRAWS re-runs) and the worst error of the lane emulator on those.  The shares are
conditions of the tests; the errors are a record and never a bound.

    python tools/measure_engine_matrix.py                    # oracle + emulator, here
    python tools/measure_engine_matrix.py --gpu LOG          # also keep the worst GPU error per group, read from the output of
                                                             # pytest -m gpu -s tests/test_gpu_engine_matrix.py (the "name: compared a / b, worst error x" lines)
"""
import json
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

import numpy as np  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "engine_matrix.json")
if not os.path.exists(PATH):       # first run: the test module below reads the record when it is imported
    with open(PATH, "w") as f:
        json.dump({"groups": {}}, f)

import engine_matrix_cases as C  # noqa: E402
from test_cpu_engine_matrix import emulate  # noqa: E402


def main(argv):
    gpu = {}
    if "--gpu" in argv:
        for line in open(argv[argv.index("--gpu") + 1]):
            m = re.search(r"([\w-]+): compared (\d+) / (\d+), worst error ([0-9.e+-]+)", line)
            if m:
                gpu[m.group(1)] = float(m.group(4))
    old = json.load(open(PATH))["groups"] if os.path.exists(PATH) else {}
    groups = {}
    for name in C.NAMES:
        g = C.group(name)
        oracle = C.oracle_results(g)
        worst = 0.0
        for (xd, _), (xo, _, sens) in zip(emulate(g, oracle), oracle):
            m = sens < C.SENS_MAX
            worst = max(worst, float(np.abs(xd - xo).max(axis=1)[m].max()) if m.any() else 0.0)
        rec = {"family": g.family, "cases": g.n, "compared": sum(int((s < C.SENS_MAX).sum()) for _, _, s in oracle), "emu_worst": float("%.2e" % worst)}
        if name in gpu or "gpu_worst" in old.get(name, {}):
            rec["gpu_worst"] = float("%.2e" % gpu[name]) if name in gpu else old[name]["gpu_worst"]
        groups[name] = rec
        print(name, rec, flush=True)
    with open(PATH, "w") as f:
        json.dump({"draws": C.DRAWS, "sens_max": C.SENS_MAX, "bound": C.BOUND, "groups": groups}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
