"""grx.BatchedSim on the MI355X (pytest -m gpu) against tests/constraint_refs.py on the cases of tests/constraint_cases.py: joint and tendon limits, friction loss, joint
equalities, actuators with their clamps, and both integrators, held to a reference that shares nothing with the compiler, the oracle or the engine.  N = 5 worlds per case,
13 once; the starts are the draws the committed record names, whose preconditions tests/test_cpu_constraint_rows.py asserts for every world compared here.

One BatchedSim per (case, n); outputs nefc, qfrc_actuator, qfrc_constraint, qacc, qacc_smooth, qfrc_smooth, pre-filled with NaN; qacc_warmstart zeroed; forward() and step(1)
from the same fp32 start, and step(RK4_STEPS) once per RK4 case.  nefc is exact; the vectors: sim_dyn_cases.error within test_gpu_sim_dynamics.vector_bounds() (these scenes
set no bound of their own); qpos and qvel after the steps: engine_matrix_cases.BOUND.  Every figure is printed before it is asserted
(tools/measure_constraint_rows.py reads the lines).

What it found: no defect, and a limit.  mixed-8-rk4 as first generated had a light hinge without armature at the end of a chain (M_dd = 2.4e-3, (M^-1)_dd up to 700): qacc_smooth
was off by 1.76e-5 of its scale (bound 1e-5) in worlds the reference called well posed; the fp64 build of the engine source gives 1.2e-14.  The engine holds the bodies'
inertias about their tree's root body, so M_dd carries 2^-24 of m r^2 and not of itself.  constraint_cases.fp32_inertia_storage is the precondition that was missing, and the
mixed cases carry armature on every joint: 4.1e-7 now (DESIGN.md 5 states the limit)."""
import numpy as np
import pytest

import constraint_cases as CC
import engine_matrix_cases as C
import sim_dyn_cases as D
import test_gpu_sim_dynamics as G

pytestmark = pytest.mark.gpu

OUTPUTS = ("nefc", "qfrc_actuator", "qfrc_constraint", "qacc", "qacc_smooth", "qfrc_smooth")
VECTORS = OUTPUTS[1:]
ROWS = ("qpos", "qvel", "ctrl")


def load(sim, st):
    import torch

    for k in ROWS:
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    for k in sim.dynamics:
        getattr(sim, k).fill_(float("nan"))      # the launch owes every element


def read(sim):
    import torch

    torch.cuda.synchronize()
    out = {k: getattr(sim, k).cpu().numpy().copy() for k in ("qpos", "qvel", "qacc_warmstart") + sim.outputs}
    out["status"], out["status_sticky"] = sim.status.cpu().numpy().copy(), sim.status_sticky.cpu().numpy().copy()
    return out


_RUNS = {}


def run(name, n, **kw):
    """(after forward(), after step(1), after step(RK4_STEPS) for an RK4 case else None), each from the same start, once per (case, n, handle options)"""
    key = (name, n, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RUNS:
        import torch

        import gymnasium_robotics_amd as grx

        assert torch.cuda.is_available(), "these tests need the GPU"
        case = CC.CASES[name]
        sim = grx.BatchedSim(case.model, num_worlds=n, outputs=OUTPUTS, **kw)
        st = case.states(n, recorded=True)
        out = []
        for nstep in (0, 1) + ((CC.RK4_STEPS,) if name in CC.RK4 else ()):
            load(sim, st)
            sim.step(nstep) if nstep else sim.forward()
            out.append(read(sim))
        sim.close()
        _RUNS[key] = tuple(out) + (None,) * (3 - len(out))
    return _RUNS[key]


@pytest.mark.parametrize("name,n", CC.RUNS)
def test_forward_and_step_equal_the_reference(name, n):
    case, ref = CC.CASES[name], CC.reference(name, n, recorded=True)
    st = case.states(n, recorded=True)
    fwd, stp, stpk = run(name, n)
    want = {k: CC.stacked(name, n, k) for k in VECTORS + ("qpos1", "qvel1") + (("qposk", "qvelk") if name in CC.RK4 else ())}
    fig = {k: float(D.error(k, fwd[k], want[k]).max()) for k in VECTORS}
    fig["qpos1"], fig["qvel1"] = float(np.abs(stp["qpos"].astype(np.float64) - want["qpos1"]).max()), float(np.abs(stp["qvel"].astype(np.float64) - want["qvel1"]).max())
    if stpk is not None:
        fig["qposk"], fig["qvelk"] = float(np.abs(stpk["qpos"].astype(np.float64) - want["qposk"]).max()), float(np.abs(stpk["qvel"].astype(np.float64) - want["qvelk"]).max())
    nefc = [r["nefc"] for r in ref]
    print(f"constraint-rows {name} n={n}:", " ".join(f"{k} {v:.2e}" for k, v in fig.items()), "nefc", " ".join(map(str, fwd["nefc"].reshape(-1))))
    bound = G.vector_bounds()
    assert list(fwd["nefc"].reshape(-1)) == nefc, (name, fwd["nefc"], nefc)
    for k in VECTORS:
        assert np.isfinite(fwd[k]).all(), (name, k, "non-finite (a NaN is an element the launch did not write)")
        assert fig[k] <= bound[k], (name, k, fig[k], bound[k])
    for k in fig:
        if k not in VECTORS:
            assert fig[k] < C.BOUND, (name, k, fig[k])
    for r in (fwd, stp) + ((stpk,) if stpk is not None else ()):
        assert (r["status"] == 0).all() and (r["status_sticky"] == 0).all(), (r["status"], r["status_sticky"])
    assert np.array_equal(fwd["qpos"], st["qpos"].astype(np.float32)) and np.array_equal(fwd["qvel"], st["qvel"].astype(np.float32))      # forward() leaves the state
    if not case.model.dim("nu"):
        assert not fwd["qfrc_actuator"].view(np.uint32).any()      # bit-zero, not merely small


def test_thirteen_worlds_equal_five_bit_for_bit():
    small, big = run(CC.RUN13, CC.N_WORLDS), run(CC.RUN13, 13)
    for a, b in zip(small[:2], big[:2]):
        G.same_bits(a, b, [k for k in a if a[k].size], slice(0, CC.N_WORLDS))


def test_rows_70_on_a_64_row_table_reruns_to_the_same_bits():
    """under capacity maxefc = 64 every world of rows-70 overflows the step launch's tables and is run again on the large ones: the same bits as on the default tables"""
    name = "rows-70"
    assert min(r["nefc"] for r in CC.reference(name, CC.N_WORLDS, recorded=True)) > 64
    wide, narrow = run(name, CC.N_WORLDS), run(name, CC.N_WORLDS, capacity=dict(maxefc=64))
    for a, b in zip(wide[:2], narrow[:2]):
        assert (b["status"] == 0).all() and (b["status_sticky"] == 0).all(), (b["status"], b["status_sticky"])
        G.same_bits(a, b, [k for k in a if a[k].size and k not in ("status", "status_sticky")])
