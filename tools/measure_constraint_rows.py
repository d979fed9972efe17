"""Writes tests/golden/constraint_rows_errors.json: per case of tests/constraint_cases.py the worst figures of the oracle, the lane emulator and the MI355X against the
reference of tests/constraint_refs.py, the worst precondition values of its worlds and, under "draws", the draw every world's start was accepted at (the device tests
take their starts from there; tests/test_cpu_constraint_rows.py asserts that the redraw loop gives the same).  The figures are a record and never a bound: the tests take
their bounds from tests/golden/sim_dynamics_errors.json and engine_matrix_cases.BOUND.

    python tools/measure_constraint_rows.py                    # reference, oracle and emulator, here
    python tools/measure_constraint_rows.py --gpu LOG          # also the device's figures, read from the output of
                                                               # pytest -m gpu -s tests/test_gpu_constraint_rows.py (the "constraint-rows <case> n=<n>: field value ..." lines)
"""
import json
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

import constraint_cases as CC  # noqa: E402
import engine_matrix_cases as C  # noqa: E402
from test_cpu_constraint_rows import ORACLE_TOL, compare_oracle, emulate  # noqa: E402

r2 = lambda x: float("%.2e" % x)
# what the first version of the cases found: kept with the record
FOUND = {"what": "qacc_smooth of mixed-8-rk4 as first generated: a light hinge without armature (M_dd 2.4e-3, (1/M)_dd up to 700) at the end of a chain",
         "before": {"mi355x_qacc_smooth": 1.76e-05, "bound": 1e-05, "emulator_M_carried_to_qacc_smooth": 4.6e-05, "fp64_engine_build": 1.2e-14, "fp32_storage_of_M": 8.4e-08,
                    "fp32_inertia_storage": 1.1e-04, "one_ulp_sensitivity": 9.3e-06},
         "cause": "fp32 rounding of the bodies' inertias about their tree's root body (2^-24 of m r^2, not of the link's own inertia); no wrong formula",
         "after": "precondition fp32_inertia_storage added, armature on every joint of the mixed cases: see cases/mixed-8-rk4/5"}


def main(argv):
    gpu = {}
    if "--gpu" in argv:
        for line in open(argv[argv.index("--gpu") + 1]):
            m = re.search(r"constraint-rows ([\w-]+) n=(\d+): (.*?) nefc", line)
            if m:
                words = m.group(3).split()
                gpu[f"{m.group(1)}/{m.group(2)}"] = {k: r2(float(v)) for k, v in zip(words[0::2], words[1::2])}
    old = json.load(open(CC.GOLDEN))["cases"] if os.path.exists(CC.GOLDEN) else {}
    cases, draws = {}, {}
    for name, n in CC.RUNS:
        key = f"{name}/{n}"
        case = CC.CASES[name]
        st = case.states(n)
        draws[name] = max(draws.get(name, []), [int(d) for d in st["draws"]], key=len)
        fig = st["figures"]
        pre = {k: r2((min if k in ("limit", "zone", "clamp") else max)(f[k] for f in fig)) for k in fig[0]}
        rec = {"nv": case.model.dim("nv"), "nefc": [r["nefc"] for r in CC.reference(name, n)], "preconditions": {k: (v if v != float("inf") else None) for k, v in pre.items()},
               "oracle": {k: r2(v) for k, v in compare_oracle(name, n).items()}, "emulator": {k: r2(v) for k, v in emulate(name, n).items()}}
        if key in gpu:
            rec["mi355x"] = gpu[key]
        elif "mi355x" in old.get(key, {}):
            rec["mi355x"] = old[key]["mi355x"]
        cases[key] = rec
        print(key, rec, flush=True)
    with open(CC.GOLDEN, "w") as f:
        json.dump({"jitter_draws": C.DRAWS, "sens_max": C.SENS_MAX, "bound": C.BOUND, "vector_bounds": CC.vector_bounds(), "oracle_tolerance": ORACLE_TOL, "limit_margin": CC.LIMIT_MARGIN,
                   "relative_margin": CC.REL_MARGIN, "rk4_steps": CC.RK4_STEPS, "found": FOUND, "draws": draws, "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
