"""Measure the body-wrench outputs of grx.BatchedSim against the fp64 reference (tests/wrench_refs.py) on a machine with a GPU and write tests/golden/wrench_errors.json:
per tree case of tests/test_cpu_wrench.RUNS the worst force figure |got - want|_inf / (1 + sum_b m_b |g| + max_b |want_b|_inf) over cfrc_int and cfrc_ext of the case's
worlds after forward(), which tests/test_cpu_wrench.py and tests/test_gpu_wrench.py assert twice of.  The figures of cacc and subtree_com, which have bounds of their own
(the acceleration rule of the sensor tests, engine_matrix_cases.BOUND), are recorded next to them for the reader.

    python tools/wrench_errors.py"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "wrench_errors.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import test_gpu_wrench as T
    from test_cpu_wrench import RUNS

    out = dict(measure="worst |got - want|_inf / (1 + sum_b m_b |g| + max_b |want_b|_inf) over cfrc_int and cfrc_ext of the case's worlds, forward() with xfrc_applied on two bodies",
               device={}, cacc={}, subtree_com={})
    for name, n in RUNS:
        fig = T.figures(name, n)
        out["device"][name] = max(out["device"].get(name, 0.0), fig["cfrc_int"], fig["cfrc_ext"])
        out["cacc"][name] = max(out["cacc"].get(name, 0.0), fig["cacc"])
        out["subtree_com"][name] = max(out["subtree_com"].get(name, 0.0), fig["subtree_com"])
        print(name, n, fig)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
