"""Writes tests/golden/contact_matrix.json, the record behind the caps of the contact-matrix tests (tests/contact_matrix_cases.py): per group the number of cases the
ORACLE ALONE classifies as compared (its contact set is kept and dist / pos / normal move less than SENS_MAX over DRAWS one-ulp jitters), the multi-contact cases among
them, and the worst error of the lane emulator on those.  The shares are conditions of the tests; the errors are a record and never a bound.

    python tools/measure_contact_matrix.py                    # oracle + emulator, here
    python tools/measure_contact_matrix.py --gpu LOG          # also keep the worst GPU error per group, read from the output of
                                                              # pytest -m gpu -s tests/test_gpu_contact_matrix.py (the "name: compared a / b, worst error x" lines)
"""
import json
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

PATH = os.path.join(ROOT, "tests", "golden", "contact_matrix.json")
if not os.path.exists(PATH):       # first run: the test module below reads the record when it is imported
    with open(PATH, "w") as f:
        json.dump({"groups": {}}, f)

import contact_matrix_cases as M  # noqa: E402
import engine_matrix_cases as C  # noqa: E402
from test_cpu_contact_matrix import emulate  # noqa: E402


def main(argv):
    gpu = {}
    if "--gpu" in argv:
        for line in open(argv[argv.index("--gpu") + 1]):
            m = re.search(r"([\w-]+): compared (\d+) / (\d+), worst error ([0-9.e+-]+), tangents ([0-9.e+-]+)", line)
            if m:
                gpu[m.group(1)] = (float(m.group(4)), float(m.group(5)))
    old = json.load(open(PATH))["groups"]
    groups = {}
    for name in M.NAMES:
        g = M.group(name)
        compared, multi = M.counts(g)
        rec = {"family": g.family, "cases": g.n, "compared": compared, "multi": multi}
        try:      # the errors are a record: a group the emulator fails on keeps its shares and says so
            rec["emu_worst"] = float("%.2e" % M.accept(g, emulate(g), 0, tangents=False)[2])
        except AssertionError as e:
            rec["emu_worst"] = None
            print(name, "FAILS on the emulator:", str(e)[:300], flush=True)
        if name in gpu:
            rec["gpu_worst"], rec["gpu_worst_tangent"] = (float("%.2e" % x) for x in gpu[name])
        elif "gpu_worst" in old.get(name, {}):
            rec["gpu_worst"], rec["gpu_worst_tangent"] = old[name]["gpu_worst"], old[name].get("gpu_worst_tangent")
        groups[name] = rec
        print(name, rec, flush=True)
    with open(PATH, "w") as f:
        json.dump({"draws": C.DRAWS, "sens_max": C.SENS_MAX, "bound": C.BOUND, "groups": groups}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
