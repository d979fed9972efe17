"""Per-world model parameters of grx.BatchedSim on the GPU (pytest -m gpu), on the scenes and drawn rows of tests/sim_params_cases.py.  N = 5 worlds, 13 once.

The reference of an edited world is an OracleSim of its own with the same fp32 values written into its model (sim_params_cases.edited_oracle).  Floats agree within
engine_matrix_cases.BOUND (1e-4), the acceleration of the same pass within the qacc bound of tests/test_gpu_sim_dynamics.py, ncon / nefc exactly, the low status half is 0.
The preconditions -- every drawn world is well-posed for its oracle and differs from the nominal model by more than a hundred bounds -- are asserted in
tests/test_cpu_sim_params.py for every case compared here.  Where two simulations must agree, they agree bit for bit."""
import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S
import sim_dyn_cases as D
import sim_params_cases as P
import test_gpu_sim as G      # load / read / compare / same_bits
import test_gpu_sim_dynamics as GD      # vector_bounds

pytestmark = pytest.mark.gpu

N = P.N
ROWS = G.ROWS
WITH_QACC = S.ALL_OUTPUTS + ("qacc",)


def make(scene, n=N, outputs=S.ALL_OUTPUTS, **kw):
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sc = P.SCENES[scene]
    sim = grx.BatchedSim(sc.model, num_worlds=n, outputs=outputs, **kw)
    G.load(sim, sc.states(n))
    return sim


def run(sim, nstep):
    if nstep:
        sim.step(nstep)
    else:
        sim.forward()


def invalid(sim):
    import torch

    torch.cuda.synchronize()
    return sim.params_invalid.cpu().numpy().copy()


def against_the_oracle(tag, sim, got, want, nstep, worlds=None):
    G.compare(tag, got, want, G.DERIVED if nstep == 0 else S.FLOAT_FIELDS, worlds=worlds)
    sel = slice(None) if worlds is None else worlds
    if "qacc" in got:
        err = D.error("qacc", got["qacc"][sel], want["qacc"][sel])
        print(tag, "qacc", f"{err.max():.2e}", "bound", P.qacc_bound())
        assert (err < P.qacc_bound()).all(), (tag, "qacc", err)
    assert (got["status"][sel] == 0).all(), (tag, got["status"])


# 1 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,n", [("arm", N), ("mocap", N), ("rk4", N), ("pile", N), ("arm", 13)])
def test_nominal_parameters_are_invisible(scene, n):
    """every parameter named, left at its initial value and committed: the commit kernel rebuilds every private record from the world's rows, and the launches -- on kernels
    of their own, each world on a descriptor of its own -- give the bits of a plain BatchedSim, after forward(), step(1) and step(4), the pile's re-run included"""
    plain, prm = make(scene, n), make(scene, n, model_params=P.ALL)
    assert prm.param_names and prm._p is not None and plain._p is None
    for name in P.ALL:      # the rows start at the model's own fp32 values
        a = getattr(prm.params, name).cpu().numpy()
        assert a.shape == prm._param_shape(name) and (a == np.float32(P.nominal(P.SCENES[scene], name))[None]).all(), name
    prm.commit_params()
    assert (invalid(prm) == 0).all()
    names = ROWS + plain.outputs + ("status", "status_sticky")
    for nstep in (0, 1, 4):
        run(plain, nstep); run(prm, nstep)
        a, b = G.read(plain), G.read(prm)
        G.same_bits(a, b, names)
        assert (a["status"] == 0).all()
    if scene == "pile":
        assert sorted(prm.lane.entered_last_step().tolist()) == sorted(plain.lane.entered_last_step().tolist()) == list(range(1, n))
    plain.close(); prm.close()


# 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,scene", P.GROUP_CASES)
def test_edited_worlds_equal_the_edited_oracle(group, scene):
    sc = P.SCENES[scene]
    rows = P.draw(sc, P.GROUPS[group])
    sim = make(scene, outputs=WITH_QACC, model_params=P.GROUPS[group])
    P.load_params(sim, rows)
    sim.commit_params()
    assert (invalid(sim) == 0).all(), invalid(sim)
    for nstep in P.STEPS:
        G.load(sim, sc.states(N))
        run(sim, nstep)
        against_the_oracle(f"{group} {scene} {'forward' if nstep == 0 else f'step({nstep})'}", sim, G.read(sim), P.oracle_run(sc, group, rows, N, nstep, ()), nstep)
    sim.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------------------------------
DYN_PARAMS, DYN_FIELDS = P.DYN_PARAMS, P.DYN_FIELDS


@pytest.mark.parametrize("scene", ["armv", "rk4"])
def test_dynamics_block_of_edited_worlds(scene):
    sc = P.SCENES[scene]
    rows = P.draw(sc, DYN_PARAMS)
    bounds = dict(GD.vector_bounds(), qM=C.BOUND)
    assert all(bounds[k] == v for k, v in P.dyn_bounds().items())      # the bounds the CPU preconditions were measured against
    sim = make(scene, outputs=S.ALL_OUTPUTS + DYN_FIELDS, model_params=DYN_PARAMS)
    P.load_params(sim, rows)
    sim.commit_params()
    for nstep in (0, 1):
        G.load(sim, sc.states(N))
        for k in DYN_FIELDS:
            getattr(sim, k).fill_(float("nan"))
        run(sim, nstep)
        got, want = G.read(sim), P.oracle_run(sc, "dynamics", rows, N, nstep, ())
        worst = {k: float(D.error(k, got[k], want[k]).max()) for k in DYN_FIELDS}
        print(scene, nstep, " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert all(np.isfinite(got[k]).all() for k in DYN_FIELDS)
        assert all(worst[k] < bounds[k] for k in DYN_FIELDS), {k: (worst[k], bounds[k]) for k in DYN_FIELDS if not worst[k] < bounds[k]}
        assert (got["status"] == 0).all()
    sim.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_masked_commit():
    """all worlds edited, two committed: the others step with the bits of the plain simulation (their rows differ from what they run on until a commit selects them)"""
    sc = P.SCENES["armv"]
    rows = P.draw(sc, P.ALL)
    mask = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    out, on = np.nonzero(mask == 0)[0], np.nonzero(mask)[0]
    plain, prm = make("armv"), make("armv", model_params=P.ALL)
    P.load_params(prm, rows)
    prm.commit_params(mask=mask)
    assert (invalid(prm) == 0).all()
    plain.step(4); prm.step(4)
    a, b = G.read(plain), G.read(prm)
    G.same_bits(a, b, ROWS + plain.outputs + ("status", "status_sticky"), out)
    against_the_oracle("masked commit step(4)", prm, b, P.oracle_run(sc, "all", rows, N, 4, ()), 4, worlds=on)
    assert all((a["qvel"][w] != b["qvel"][w]).any() for w in on)
    plain.close(); prm.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_rows_keep_the_last_good_commit():
    import torch

    from gymnasium_robotics_amd.sim import PARAM_BAD

    sc = P.SCENES["armv"]
    names = ("body_mass", "dof_frictionloss", "dof_damping")
    rows = P.draw(sc, names)
    a, b = make("armv", model_params=names), make("armv", model_params=names)
    for sim in (a, b):
        P.load_params(sim, rows)
        sim.commit_params()
    assert (invalid(a) == 0).all()
    fl = int(np.nonzero(P.nominal(sc, "dof_frictionloss") > 0)[0][0])
    a.params.dof_damping[0, 1] = float("nan")
    a.params.dof_frictionloss[1, fl] = 0.0
    a.params.body_mass[3, 2] = -0.5
    for sim in (a, b):      # the clean worlds go back to the model's own values in both
        for name in names:
            getattr(sim.params, name)[[2, 4]] = torch.from_numpy(np.float32(P.nominal(sc, name))).to(sim.device)
    a.commit_params(); b.commit_params(mask=np.array([0, 0, 1, 0, 1], dtype=np.uint8))
    bad = invalid(a)
    print("params_invalid", bad)
    assert bad[0] & PARAM_BAD["nonfinite"] and not bad[0] & ~(PARAM_BAD["nonfinite"] | PARAM_BAD["damping"])      # (a NaN is not >= 0 either: the damping rule's bit may come with it)
    assert bad[1] == PARAM_BAD["frictionloss"] and bad[3] == PARAM_BAD["inertial"] and bad[2] == 0 and bad[4] == 0
    a.step(2); b.step(2)
    ra, rb = G.read(a), G.read(b)
    G.same_bits(ra, rb, ROWS + a.outputs + ("status", "status_sticky"))
    assert (ra["status"] == 0).all()
    # and the clean worlds run on their new rows: those of the plain simulation
    plain = make("armv")
    plain.step(2)
    G.same_bits(ra, G.read(plain), ROWS + a.outputs, [2, 4])
    assert all((ra["qvel"][w] != G.read(plain)["qvel"][w]).any() for w in (0, 1, 3))
    # a later good row is accepted and clears the world's bits
    a.params.dof_damping[0, 1] = 0.25
    a.commit_params(mask=np.array([1, 0, 0, 0, 0], dtype=np.uint8))
    assert invalid(a).tolist() == [0, PARAM_BAD["frictionloss"], 0, PARAM_BAD["inertial"], 0]
    a.close(); b.close(); plain.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstep", [1, 4])
def test_overflow_rerun_with_parameters(nstep):
    sc = P.SCENES["pile"]
    rows = P.draw(sc, P.PILE_PARAMS)
    want = P.oracle_run(sc, "pile", rows, N, nstep, ())
    assert (want["ncon"][1:] > S.PILE_MAXCON).all() and want["ncon"][0] <= S.PILE_MAXCON
    sim = make("pile", overflow="rerun", model_params=P.PILE_PARAMS)
    P.load_params(sim, rows)
    sim.commit_params()
    sim.step(nstep)
    got = G.read(sim)
    G.compare(f"pile rerun with parameters step({nstep})", got, want, S.FLOAT_FIELDS)
    assert (got["status"] == 0).all() and (got["status_sticky"] == 0).all(), (got["status"], got["status_sticky"])
    assert sorted(sim.lane.entered_last_step().tolist()) == [1, 2, 3, 4] and (invalid(sim) == 0).all()
    sim.close()


def test_overflow_flag_with_parameters():
    sc = P.SCENES["pile"]
    rows = P.draw(sc, P.PILE_PARAMS)
    sim = make("pile", overflow="flag", model_params=P.PILE_PARAMS)
    assert sim.lane is None
    P.load_params(sim, rows)
    sim.commit_params()
    sim.step(1)
    got = G.read(sim)
    assert ((got["status"][1:] & 6) != 0).all() and ((got["status_sticky"][1:] & 6) != 0).all(), got["status"]
    assert (got["ncon"][1:] == S.PILE_MAXCON).all() and got["status"][0] == 0
    G.compare("pile flag with parameters world 0", got, P.oracle_run(sc, "pile", rows, N, 1, ()), S.FLOAT_FIELDS, worlds=[0])
    sim.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_carries_the_parameters():
    sc = P.SCENES["armv"]
    rows = P.draw(sc, P.ALL)
    a = make("armv", model_params=P.ALL)
    P.load_params(a, rows)
    a.commit_params()
    a.step(2)
    saved = a.get_state()
    assert set(saved["params"]) == set(P.ALL) and all(isinstance(v, np.ndarray) and v.shape[0] == N for v in saved["params"].values())
    b = make("armv", model_params=P.ALL)      # fresh: nominal parameters
    b.set_state(saved)
    assert (invalid(b) == 0).all()
    a.step(1); b.step(1)
    names = ROWS + a.outputs + ("status", "status_sticky")
    G.same_bits(G.read(a), G.read(b), names)
    # a state without the key loads and leaves the parameters alone; reset() does not touch them either
    bare = {k: v for k, v in a.get_state().items() if k != "params"}
    b.set_state(bare)
    a.step(1); b.step(1)
    G.same_bits(G.read(a), G.read(b), names)
    a.reset(); b.reset()
    G.load(a, sc.states(N)); G.load(b, sc.states(N))
    a.step(1); b.step(1)
    G.same_bits(G.read(a), G.read(b), names)
    against_the_oracle("after reset step(1)", a, G.read(a), P.oracle_run(sc, "all", rows, N, 1, ()), 1)
    with pytest.raises(ValueError, match="gravity"):
        b.set_state(dict(saved, params={k: v for k, v in saved["params"].items() if k != "gravity"}))
    plain = make("armv")
    with pytest.raises(ValueError, match="names none"):
        plain.set_state(saved)
    a.close(); b.close(); plain.close()


# the argument checks of the C entry points that need a live object (the others: tests/test_cpu_sim_params.py) ------------------------------------------------------
def test_argument_checks_that_need_a_live_object():
    import ctypes

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    err = lambda: L.grx_last_error().decode()
    sim = make("armv", model_params=("gravity", "dof_damping"))
    sim.forward()
    H, I, F = P.SCENES["rk4"].model.pack()
    other = _native.acquire_model(H, I, F, 0)      # a model the object was not created for, with other table shapes
    try:
        b = sim._bufs
        assert L.grx_sim_step_params(other, sim._p, ctypes.byref(b), None, N, 1, 0, None) == -1 and "not created for this model handle" in err()
        for n in (N + 1, N - 1):
            assert L.grx_sim_step_params(sim._h, sim._p, ctypes.byref(b), None, n, 1, 0, None) == -1 and "n_worlds" in err() and str(N) in err()
        names = (ctypes.c_char_p * 1)(b"gravity")
        out = ctypes.c_void_p()
        assert L.grx_sim_params_create(sim._h, other, N, names, 1, ctypes.byref(out)) == -1 and "table shapes differ" in err() and out.value is None
        ptr, cnt = ctypes.c_void_p(), ctypes.c_int()
        assert L.grx_sim_params_row(sim._p, b"body_mass", ctypes.byref(ptr), ctypes.byref(cnt)) == -1 and "not a parameter of this object" in err()
        assert L.grx_sim_params_row(sim._p, b"dof_damping", ctypes.byref(ptr), ctypes.byref(cnt)) == 0 and cnt.value == sim.nv and ptr.value == sim.params.dof_damping.data_ptr()
        # what grx_sim_step refuses is refused here too, with the object in place
        bad = _native.SimBuffersStruct.from_buffer_copy(b)
        bad.status = None
        assert L.grx_sim_step_params(sim._h, sim._p, ctypes.byref(bad), None, N, 1, 0, None) == -1 and "status" in err()
    finally:
        import torch

        torch.cuda.synchronize()
        _native.release_model(other)
    before = G.read(sim)
    sim.forward()      # and the object still serves its own handle (a second forward() starts its solve from the first one's warm start: the state rows and the kinematics repeat)
    after = G.read(sim)
    G.same_bits(before, after, ("qpos", "qvel", "xpos", "xquat", "site_xpos", "site_xmat", "status"))
    assert (after["status"] == 0).all()
    sim.close()
