"""grx.BatchedSim on the MI355X (pytest -m gpu) against tests/dyn_refs.py on the trees of tests/dyn_tree_cases.py: kinematics, site frames and Jacobians, qM, the smooth
force and acceleration vectors and one Euler step, held to a reference that shares nothing with the compiler, the oracle or the engine.  N = 5 worlds per case, 13 once.
The precondition (the reference moves less than SENS_MAX under a one-ulp jitter of the start) is asserted in tests/test_cpu_dyn_trees.py for every world compared here.

Bounds.  Poses, site frames, qM and the Jacobians: engine_matrix_cases.BOUND, absolute.  Site velocities: BOUND (1 + |qvel|_1) -- each Jacobian entry is within BOUND.  The
vectors: sim_dyn_cases.error within the vector_bounds() of tests/golden/sim_dynamics_errors.json; these scenes set no bound of their own.  qpos and qvel after step(1):
BOUND.  Every figure is printed before it is asserted (tools/measure_dyn_trees.py reads the lines).

What it found: qfrc_bias of free-root-tree, world 6 of 13, was off by 3.03e-6 of its scale (bound 1e-6) on the MI355X and the emulator alike, on a world the reference calls
well posed (6.8e-7 under the one-ulp jitter, 3.8e-7 from fp32 storage of the inputs).  grx_velocity carried the free root's linear velocity through the recursive pass:
terms of m |omega| |v| (210 N) that cancel in a bias of 11 N.  The generic engine now leaves a free joint's linear dofs out of the spatial velocities (the bias does not
change under a constant linear velocity of the whole tree): 5.82e-7 on the MI355X and on the emulator.  tests/test_cpu_dyn_trees.py holds the emulator to the same bound."""
import numpy as np
import pytest

import dyn_refs as R
import dyn_tree_cases as T
import engine_matrix_cases as C
import sim_dyn_cases as D
import test_gpu_sim_dynamics as G

pytestmark = pytest.mark.gpu

ABSOLUTE = ("xpos", "xquat", "xipos", "site_xpos", "site_xmat", "qM", "site_jacp", "site_jacr")
ROWS = ("qpos", "qvel")


def outputs():
    from gymnasium_robotics_amd import sim as simmod

    return simmod.OUTPUTS      # no case has a touch sensor: sensordata is [N, 0], every other output applies


def load(sim, st):
    import torch

    for k in ROWS:
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)))
    sim.qacc_warmstart.zero_()
    for k in sim.dynamics:
        getattr(sim, k).fill_(float("nan"))      # the launch owes every element


def read(sim):
    import torch

    torch.cuda.synchronize()
    out = {k: getattr(sim, k).cpu().numpy().copy() for k in ROWS + ("qacc_warmstart",) + sim.outputs + ("xipos",)}
    out["status"], out["status_sticky"] = sim.status.cpu().numpy().copy(), sim.status_sticky.cpu().numpy().copy()
    return out


_RUNS = {}


def run(name, n):
    """(after forward(), after step(1) from the same start) of the n worlds of a case, once per (case, n)"""
    if (name, n) not in _RUNS:
        import torch

        import gymnasium_robotics_amd as grx

        assert torch.cuda.is_available(), "these tests need the GPU"
        case = T.CASES[name]
        sites = tuple(sorted(case.model.names["site"], key=case.model.names["site"].get))      # row = site id, as T.want orders them
        sim = grx.BatchedSim(case.model, num_worlds=n, outputs=outputs(), jac_sites=sites, applied=("xipos",))
        st = case.states(n)
        load(sim, st)
        sim.forward()
        fwd = read(sim)
        load(sim, st)
        sim.step(1)
        stp = read(sim)
        sim.close()
        _RUNS[(name, n)] = (fwd, stp)
    return _RUNS[(name, n)]


@pytest.mark.parametrize("name,n", T.RUNS)
def test_forward_and_step_equal_the_reference(name, n):
    case = T.CASES[name]
    want, _ = T.want(name, n)
    st = case.states(n)
    fwd, stp = run(name, n)
    nv = case.model.dim("nv")
    ref = dict(want, qM=want["M"], qfrc_constraint=np.zeros((n, nv)), qfrc_actuator=np.zeros((n, nv)))
    got = dict(fwd, xquat=R.sign_like(fwd["xquat"].astype(np.float64), want["xquat"]))
    fig = {}
    for k in ABSOLUTE:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        fig[k] = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
    vel_tol = C.BOUND * (1.0 + np.abs(st["qvel"]).sum(axis=1))
    for k in ("site_xvelp", "site_xvelr"):
        fig[k] = float((np.abs(got[k].astype(np.float64) - ref[k]).max(axis=(1, 2)) / vel_tol).max() * C.BOUND)      # in units in which BOUND is the tolerance
    for k in D.VECTORS:
        fig[k] = float(D.error(k, got[k], ref[k]).max())
    fig["qpos1"] = float(np.abs(stp["qpos"].astype(np.float64) - want["qpos1"]).max())
    fig["qvel1"] = float(np.abs(stp["qvel"].astype(np.float64) - want["qvel1"]).max())
    print(f"dyn-tree {name} n={n}:", " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    bound = G.vector_bounds()
    for k in ABSOLUTE + D.VECTORS + ("site_xvelp", "site_xvelr"):
        assert np.isfinite(got[k]).all(), (name, k, "non-finite (a NaN is an element the launch did not write)")
    for k in ABSOLUTE + ("site_xvelp", "site_xvelr", "qpos1", "qvel1"):
        assert fig[k] < C.BOUND, (name, k, fig[k])
    for k in D.VECTORS:
        assert fig[k] <= bound[k], (name, k, fig[k], bound[k])
    for r in (fwd, stp):
        assert (r["status"] == 0).all() and (r["status_sticky"] == 0).all(), (r["status"], r["status_sticky"])
        assert not r["ncon"].any() and not r["nefc"].any()
        assert not r["qfrc_constraint"].view(np.uint32).any() and not r["qfrc_actuator"].view(np.uint32).any()      # bit-zero, not merely small
    assert np.array_equal(fwd["qpos"], st["qpos"].astype(np.float32)) and np.array_equal(fwd["qvel"], st["qvel"].astype(np.float32))      # forward() leaves the state
    zeros = {k: G.zero_columns(ref[k]) for k in ("site_jacp", "site_jacr")}      # a dof that does not move a site (a free joint's linear dofs turn nothing): the column is bit-zero
    assert any(z.any() for z in zeros.values()), name
    for k, zero in zeros.items():
        assert not (np.ascontiguousarray(fwd[k]).view(np.uint32).any(axis=-2) & zero).any(), (name, k, "a zero column is not bit-zero")
    assert fwd["qM"].tobytes() == np.ascontiguousarray(fwd["qM"].transpose(0, 2, 1)).tobytes()


def test_thirteen_worlds_equal_five_bit_for_bit():
    small, big = run(T.RUN13, T.N_WORLDS), run(T.RUN13, 13)
    for a, b in zip(small, big):
        G.same_bits(a, b, [k for k in a if a[k].size], slice(0, T.N_WORLDS))


def test_one_dof_more_than_full_is_refused():
    """`full` has the engine's 64 dofs on 64 joints; the same tree with a second two-joint body has 65 of each and is refused when the model handle is made, before any launch"""
    import gymnasium_robotics_amd as grx

    case = T.CASES["full"]
    bodies = [dict(b, joints=list(b["joints"])) for b in case.bodies]
    rng = np.random.default_rng(3)
    next(b for b in bodies if b["name"] == "b7")["joints"].append(T._rand_joint(rng, "extra", "hinge"))
    more = T.Case("one-dof-more", 98, bodies)
    assert more.model.dim("nv") == T.MAX_DOFS + 1 and more.model.dim("nbody") == T.MAX_BODIES + 1
    sim = grx.BatchedSim(more.model, num_worlds=2, outputs=("xpos",))
    with pytest.raises(Exception, match="engine limit: at most 64 (joints|dofs)"):
        sim.forward()
