"""The dynamics outputs of grx.BatchedSim on the GPU (pytest -m gpu): qM, the seven force / acceleration vectors and the site Jacobians against the fp64 oracle on the
scenes of tests/sim_cases.py and tests/sim_dyn_cases.py.  N = 5 worlds, 13 once.  The precondition (every field of every world moves less than SENS_MAX under a one-ulp
jitter of the start, on the oracle alone) is asserted in tests/test_cpu_sim_dynamics.py for every case compared here.

Bounds.  qM, site_jacp and site_jacr: engine_matrix_cases.BOUND (1e-4) absolute -- entries are O(1) and they are the quantities behind site_xvelp, which meets it.  The
vectors: per world max |got - want| / max(1, max |want|) (sim_dyn_cases.error) within VECTOR_BOUND[field], the smallest power of ten >= 4 x the worst figure measured on the
MI355X over arm, mocap, rk4, anchor x nstep 0, 1, 4 (tests/golden/sim_dynamics_errors.json holds the table per scene, nstep and field; the margin of 4 covers summation-order
changes between compiler versions).  The rows scene (equality, tendon-limit and friction rows, clamped actuators, two actuators on one joint) sets no bound: it is held to these."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S
import sim_dyn_cases as D

pytestmark = pytest.mark.gpu

N = S.N_WORLDS
ROWS = ("qpos", "qvel", "qacc_warmstart")
EVERYTHING = S.ALL_OUTPUTS + D.DYNAMICS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim_dynamics_errors.json")
BOUND_CASES = [f"{s}/{k}/{N}" for s, k in D.CASES if s in D.BOUND_SCENES] + ["arm/1/13"]      # the rows of the table the bounds come from


def vector_bounds():
    """{field: bound} from the committed table"""
    with open(GOLDEN) as fh:
        table = json.load(fh)["worst_error"]
    out = {}
    for f in D.VECTORS:
        worst = max(table[c][f] for c in BOUND_CASES)
        out[f] = 10.0 ** math.ceil(math.log10(4.0 * worst)) if worst > 0.0 else 0.0
    return out


def make(scene, n=N, outputs=EVERYTHING, st=None, jac_sites="scene", **kw):
    """a BatchedSim of the scene with the scene's start rows loaded (zero warm start) and every requested dynamics output filled with NaN: the launch owes every element"""
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sc = D.SCENES[scene]
    if jac_sites == "scene":
        jac_sites = D.JAC_SITES[scene] if any(o in ("site_jacp", "site_jacr") for o in outputs) else None
    sim = grx.BatchedSim(sc.model, num_worlds=n, outputs=outputs, jac_sites=jac_sites, **kw)
    st = sc.states(n) if st is None else st
    for k in ("qpos", "qvel", "ctrl", "mocap_pos", "mocap_quat"):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    for k in sim.dynamics:
        getattr(sim, k).fill_(float("nan"))
    return sim


def read(sim, names=None):
    import torch

    torch.cuda.synchronize()
    names = ROWS + sim.outputs if names is None else names
    out = {k: getattr(sim, k).cpu().numpy().copy() for k in names}
    out["status"], out["status_sticky"] = sim.status.cpu().numpy().copy(), sim.status_sticky.cpu().numpy().copy()
    return out


def same_bits(a, b, names, worlds=None):
    sel = slice(None) if worlds is None else worlds
    for k in names:
        x, y = np.ascontiguousarray(a[k][sel]), np.ascontiguousarray(b[k][sel])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def errors(got, want, fields=D.DYNAMICS, worlds=None):
    """{field: worst error over the worlds} (sim_dyn_cases.error: absolute for the matrices, normalised for the vectors)"""
    sel = slice(None) if worlds is None else worlds
    return {k: float(D.error(k, got[k][sel], want[k][sel]).max()) for k in fields}


def zero_columns(jac):
    """[..., nv] bool: the columns of [..., 3, nv] Jacobians that are exact zeros"""
    return (jac == 0.0).all(axis=-2)


def check(tag, got, want, fields=D.DYNAMICS, worlds=None):
    """every figure is printed before it is asserted; a Jacobian column the oracle has as exact zeros (a dof that does not move the site) must be bit-zero"""
    sel = slice(None) if worlds is None else worlds
    worst, bound = errors(got, want, fields, worlds), vector_bounds()
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in fields:
        assert np.isfinite(got[k][sel]).all(), (tag, k, "non-finite (a NaN is an element the launch did not write)")
        lim = C.BOUND if k in D.MATRICES else bound[k]
        assert worst[k] < lim if k in D.MATRICES else worst[k] <= lim, (tag, k, worst[k], lim)
        if k in ("site_jacp", "site_jacr"):
            zero = zero_columns(np.asarray(want[k])[sel])
            assert zero.any() and not (np.ascontiguousarray(got[k][sel]).view(np.uint32).any(axis=-2) & zero).any(), (tag, k, "a zero column is not bit-zero")
    return worst


def run_case(scene, nstep, n):
    sim = make(scene, n)
    if nstep:
        sim.step(nstep)
    else:
        sim.forward()
    got = read(sim)
    sim.close()
    return got


# 1 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep,n", [(s, k, N) for s, k in D.CASES] + [("arm", 1, 13)])
def test_step_and_forward_equal_the_oracle(scene, nstep, n):
    got, want = run_case(scene, nstep, n), D.oracle_run(scene, n, nstep)
    check(f"{scene} nstep={nstep} n={n}", got, want)
    assert (got["status"] == 0).all(), got["status"]
    if scene == "anchor":
        row = D.JAC_SITES["anchor"].index("base")
        assert not got["site_jacp"][:, row].view(np.uint32).any() and not got["site_jacr"][:, row].view(np.uint32).any()      # a site on the world body: every column


# 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep", [("arm", 1), ("mocap", 4), ("rk4", 1), ("anchor", 0)])
def test_identities_from_the_device_outputs(scene, nstep):
    """In fp64 from the fp32 outputs.  With e(f) = VECTOR_BOUND[f] max(1, |f|_inf), the error item 1 allows a vector f of one world:
    J qvel = site_xvel .......... BOUND (1 + |qvel|_1): each Jacobian entry and each velocity component is within BOUND
    qM = qM' .................... bit for bit
    qfrc_smooth = passive - bias + actuator ........ e(smooth) + e(passive) + e(bias) + e(actuator)
    qM qacc = qfrc_smooth + qfrc_constraint ........ BOUND |qacc|_1 (the entries of qM) + |qM|_inf e(qacc) (its row sums times the error of qacc) + e(smooth) + e(constraint)"""
    got = run_case(scene, nstep, N)
    g = {k: np.asarray(v, dtype=np.float64) if v.dtype == np.float32 else v for k, v in got.items()}
    raw = got["qM"]
    assert raw.tobytes() == np.ascontiguousarray(raw.transpose(0, 2, 1)).tobytes()
    bound, ids = vector_bounds(), list(D.jac_ids(scene))
    e = lambda f, w: bound[f] * max(1.0, np.abs(g[f][w]).max())
    for w in range(N):
        v = g["qvel"][w]
        tol = C.BOUND * (1.0 + np.abs(v).sum())
        dp = np.abs(g["site_jacp"][w] @ v - g["site_xvelp"][w, ids]).max()
        dr = np.abs(g["site_jacr"][w] @ v - g["site_xvelr"][w, ids]).max()
        ds = np.abs(g["qfrc_smooth"][w] - (g["qfrc_passive"][w] - g["qfrc_bias"][w] + g["qfrc_actuator"][w])).max()
        tol_s = sum(e(f, w) for f in ("qfrc_smooth", "qfrc_passive", "qfrc_bias", "qfrc_actuator"))
        dm = np.abs(g["qM"][w] @ g["qacc"][w] - (g["qfrc_smooth"][w] + g["qfrc_constraint"][w])).max()
        tol_m = C.BOUND * np.abs(g["qacc"][w]).sum() + np.abs(g["qM"][w]).sum(axis=1).max() * e("qacc", w) + e("qfrc_smooth", w) + e("qfrc_constraint", w)
        print(f"{scene} nstep={nstep} world {w}: J v {dp:.2e} {dr:.2e} (tol {tol:.2e})  smooth {ds:.2e} (tol {tol_s:.2e})  M qacc {dm:.2e} (tol {tol_m:.2e})")
        assert dp <= tol and dr <= tol and ds <= tol_s and dm <= tol_m


# 3 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep", [("arm", 4), ("rk4", 1)])
def test_no_side_effects(scene, nstep):
    """the same start with none and with all ten: the state rows, the nine old outputs and the status agree bit for bit (the last pass of the second run is the sim-local one)"""
    old, new = make(scene, outputs=S.ALL_OUTPUTS), make(scene)
    assert old._dyn is None and new._dyn is not None
    old.step(nstep); new.step(nstep)
    a, b = read(old), read(new)
    same_bits(a, b, ROWS + S.ALL_OUTPUTS + ("status", "status_sticky"))
    old.forward(); new.forward()
    same_bits(read(old), read(new), ROWS + S.ALL_OUTPUTS + ("status", "status_sticky"))
    old.close(); new.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_jacobian_after_a_step_is_one_substep_stale():
    """the fast-joint case of test_gpu_sim.test_outputs_after_a_step_are_one_substep_stale: world 2 swings its first joint at 6 rad/s, site_jacp after step(1) is the Jacobian
    MjData holds (the position stage of that substep), not the Jacobian of the returned qpos"""
    sc, ids = D.SCENES["arm"], D.jac_ids("arm")
    st = {k: v.copy() for k, v in sc.states(N).items()}
    st["qvel"][2, 0] = 6.0
    want = [D.oracle_world(sc, st, i, 1, ids) for i in range(N)]
    want = {k: np.stack([np.asarray(r[k]) for r in want]) for k in want[0]}
    fresh = D.oracle_world(sc, dict(st, qpos=want["qpos"], qvel=want["qvel"]), 2, 0, ids)
    ee = D.JAC_SITES["arm"].index("ee")
    assert np.abs(fresh["site_jacp"][ee] - want["site_jacp"][2, ee]).max() > 10 * C.BOUND      # observable on the reference alone
    sim = make("arm", st=st, outputs=("site_jacp",))
    sim.step(1)
    stale = read(sim)
    check("arm stale", stale, want, ("site_jacp",))
    sim.forward()
    now = read(sim)
    d = np.abs(now["site_jacp"][2, ee].astype(np.float64) - stale["site_jacp"][2, ee]).max()
    print("stale vs fresh site_jacp of the fast world:", d)
    assert d > 10 * C.BOUND
    assert np.abs(now["site_jacp"][2, ee] - fresh["site_jacp"][ee]).max() < C.BOUND
    sim.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_masked_out_worlds_keep_everything():
    import torch

    sim = make("anchor")
    sim.step(1)
    base = read(sim)
    mask = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    out, run = np.nonzero(mask == 0)[0], np.nonzero(mask)[0]
    sim.step(2, mask=torch.from_numpy(mask).cuda())
    after = read(sim)
    same_bits(after, base, ROWS + sim.outputs + ("status", "status_sticky"), out)
    assert all((after[k][w] != base[k][w]).any() for w in run for k in ("qM", "qacc", "qfrc_bias", "site_jacp"))
    sim.forward(mask=mask)
    same_bits(read(sim), base, ROWS + sim.outputs + ("status", "status_sticky"), out)
    sim.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstep", [1, 4])
def test_overflow_rerun(nstep):
    """worlds 1 .. 4 exceed the fast tables and are run again on the large ones: their new outputs come from the re-run launch, which takes the same block"""
    want = D.oracle_run("pile", N, nstep)
    assert (want["ncon"][1:] > S.PILE_MAXCON).all() and want["ncon"][0] <= S.PILE_MAXCON
    sim = make("pile", overflow="rerun")
    sim.step(nstep)
    got = read(sim)
    check(f"pile rerun step({nstep})", got, want)
    assert (got["status"] == 0).all() and (got["status_sticky"] == 0).all(), (got["status"], got["status_sticky"])
    assert sorted(sim.lane.entered_last_step().tolist()) == [1, 2, 3, 4]
    sim.close()


def test_overflow_flag():
    sim = make("pile", overflow="flag")
    sim.step(1)
    got = read(sim)
    assert ((got["status"][1:] & 6) != 0).all() and got["status"][0] == 0
    assert all(np.isfinite(got[k]).all() for k in D.DYNAMICS)
    check("pile flag world 0", got, D.oracle_run("pile", N, 1), worlds=[0])
    sim.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_only_site_jacr_of_one_site():
    sim = make("arm", outputs=("site_jacr",), jac_sites=("pad",))
    sim.step(1)
    got = read(sim)
    want = D.oracle_run("arm", N, 1)
    row = D.JAC_SITES["arm"].index("pad")
    assert got["site_jacr"].shape == (N, 1, 3, sim.nv)
    check("arm site_jacr pad", got, dict(site_jacr=want["site_jacr"][:, row:row + 1]), ("site_jacr",))
    sim.close()


@pytest.mark.parametrize("scene,nstep", [("arm", 4), ("rk4", 1), ("mocap", 0)])
def test_only_qfrc_bias(scene, nstep):
    """the sim-local forward pass alone; the state it returns is the state of a launch without it"""
    plain, sim = make(scene, outputs=()), make(scene, outputs=("qfrc_bias",))
    for s in (plain, sim):
        s.step(nstep) if nstep else s.forward()
    got = read(sim)
    check(f"{scene} qfrc_bias nstep={nstep}", got, D.oracle_run(scene, N, nstep), ("qfrc_bias",))
    same_bits(got, read(plain), ROWS + ("status",))
    plain.close(); sim.close()


def test_sixteen_sites():
    sim = make("pile16", outputs=("site_jacp", "site_jacr", "site_xvelp"))
    assert sim._dyn.njac == 16 and sim.nv == 16
    sim.step(1)
    got = read(sim)
    check("pile16", got, D.oracle_run("pile16", N, 1), ("site_jacp", "site_jacr"))
    assert (got["status"] == 0).all()
    sim.close()


def test_model_dependent_argument_checks():
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    z = torch.zeros(4096, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, I, F = D.SCENES["rk4"].model.pack()      # two sites
    h = _native.acquire_model(H, I, F, 0)
    try:
        b = _native.SimBuffersStruct(**{k: z.data_ptr() for k in ("qpos", "qvel", "qacc_ws", "ctrl", "status")})
        call = lambda d: (L.grx_sim_step_dyn(h, ctypes.byref(b), ctypes.byref(d), 1, 1, 0, stream), L.grx_last_error().decode())
        for bad in (2, -1):
            d = _native.SimDynamicsStruct(site_jacp=z.data_ptr(), njac=2)
            d.jac_site[0], d.jac_site[1] = 1, bad
            rc, msg = call(d)
            assert rc == -1 and "jac_site[1]" in msg and "nsite" in msg, msg
        for k in ("site_jacp", "site_jacr"):
            rc, msg = call(_native.SimDynamicsStruct(**{k: z.data_ptr()}))
            assert rc == -1 and "njac == 0" in msg, msg
        assert (z == 0).all()      # nothing was launched
    finally:
        torch.cuda.synchronize()
        _native.release_model(h)
