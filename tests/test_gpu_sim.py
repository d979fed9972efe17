"""grx.BatchedSim on the GPU (pytest -m gpu): the task-free stepper against the fp64 oracle on the scenes of tests/sim_cases.py.  N = 5 worlds (not a multiple of 8: the
padded grid and the XCD slicing of the world <-> workgroup map), 13 once.  Floats agree within engine_matrix_cases.BOUND (1e-4), ncon / nefc exactly, the low status half
is 0, and no world is left out: the precondition -- every world's oracle answer moves less than SENS_MAX under a one-ulp jitter of its start -- is asserted here on the
oracle alone (and in tests/test_cpu_sim.py, where there is no GPU)."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S

pytestmark = pytest.mark.gpu

N = S.N_WORLDS
DERIVED = tuple(k for k in S.FLOAT_FIELDS if k not in ("qpos", "qvel"))
ROWS = ("qpos", "qvel", "qacc_warmstart")


def make(scene, n=N, outputs=S.ALL_OUTPUTS, st=None, **kw):
    """a BatchedSim of the scene with the scene's start rows loaded (zero warm start)"""
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sc = S.SCENES[scene]
    sim = grx.BatchedSim(sc.model, num_worlds=n, outputs=outputs, **kw)
    load(sim, sc.states(n) if st is None else st)
    return sim


def load(sim, st):
    import torch

    for k in ("qpos", "qvel", "ctrl", "mocap_pos", "mocap_quat"):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()


def read(sim, names=None):
    import torch

    torch.cuda.synchronize()
    names = ROWS + sim.outputs if names is None else names
    out = {k: getattr(sim, k).cpu().numpy().copy() for k in names}
    out["status"], out["status_sticky"] = sim.status.cpu().numpy().copy(), sim.status_sticky.cpu().numpy().copy()
    return out


def compare(tag, got, want, fields, worlds=None):
    """every float field within BOUND (each figure is printed before it is asserted), ncon / nefc equal"""
    sel = slice(None) if worlds is None else worlds
    worst = {}
    for k in fields:
        a, b = np.asarray(got[k], dtype=np.float64)[sel], np.asarray(want[k])[sel]
        assert a.shape == b.reshape(a.shape).shape
        worst[k] = float(np.abs(a - b.reshape(a.shape)).max()) if a.size else 0.0
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert np.all([np.isfinite(np.asarray(got[k])).all() for k in fields]), (tag, "non-finite output")
    assert all(v < C.BOUND for v in worst.values()), (tag, {k: v for k, v in worst.items() if not v < C.BOUND})
    for k in S.INT_FIELDS:
        if k in got:
            assert (np.asarray(got[k])[sel] == np.asarray(want[k])[sel]).all(), (tag, k, got[k], want[k])


def same_bits(a, b, names, worlds=None):
    sel = slice(None) if worlds is None else worlds
    for k in names:
        x, y = np.ascontiguousarray(a[k][sel]), np.ascontiguousarray(b[k][sel])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


# 1 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep,n", [(s, k, N) for s, k in S.STEP_CASES] + [("arm", 1, 13)])
def test_step_equals_the_oracle(scene, nstep, n):
    sc = S.SCENES[scene]
    sens = S.oracle_sensitivity(sc, n, nstep)
    assert (sens < C.SENS_MAX).all(), (scene, nstep, "a start the oracle itself is not sure of: replace it", sens)
    sim = make(scene, n)
    sim.step(nstep)
    got = read(sim)
    compare(f"{scene} step({nstep}) n={n}", got, S.oracle_run(sc, n, nstep), S.FLOAT_FIELDS)
    assert (got["status"] == 0).all(), got["status"]
    sim.close()


# 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["arm", "mocap", "rk4"])
def test_forward_equals_the_oracle(scene):
    sc = S.SCENES[scene]
    assert (S.oracle_sensitivity(sc, N, 0) < C.SENS_MAX).all()
    sim = make(scene)
    before = read(sim, ("qpos", "qvel"))
    sim.forward()
    got = read(sim)
    compare(f"{scene} forward", got, S.oracle_run(sc, N, 0), DERIVED)
    same_bits(got, before, ("qpos", "qvel"))
    st = sc.states(N)
    same_bits(got, {k: st[k].astype(np.float32) for k in ("qpos", "qvel")}, ("qpos", "qvel"))
    assert (got["status"] == 0).all()
    sim.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_outputs_after_a_step_are_one_substep_stale():
    """After step(1) site_xpos is the position stage of that substep, BEFORE its integration -- what MjData holds -- and not the kinematics of the returned qpos.  World 2
    swings its first joint at 6 rad/s: the end effector moves ~1.5 mm per substep."""
    sc = S.SCENES["arm"]
    st = {k: v.copy() for k, v in sc.states(N).items()}
    st["qvel"][2, 0] = 6.0
    want = [S.oracle_world(sc, st, i, 1) for i in range(N)]
    want = {k: np.stack([np.asarray(r[k]) for r in want]) for k in want[0]}
    fresh = S.oracle_world(sc, dict(st, qpos=want["qpos"], qvel=want["qvel"]), 2, 0)      # the oracle's own forward pass from its post-step state
    ee = sc.model.names["site"]["ee"]
    assert np.abs(fresh["site_xpos"][ee] - want["site_xpos"][2, ee]).max() > 10 * C.BOUND      # the rule is observable on the reference alone
    sim = make("arm", st=st)
    sim.step(1)
    stale = read(sim)
    compare("arm stale", stale, want, ("qpos", "qvel", "site_xpos", "site_xmat", "site_xvelp"))
    sim.forward()
    now = read(sim)
    d = np.abs(now["site_xpos"][2, ee] - stale["site_xpos"][2, ee]).max()
    print("stale vs fresh site_xpos of the fast world:", d)
    assert d > C.BOUND
    assert np.abs(now["site_xpos"][2, ee] - fresh["site_xpos"][ee]).max() < C.BOUND
    same_bits(now, stale, ("qpos", "qvel"))
    sim.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_masked_out_worlds_keep_everything():
    import torch

    sim = make("arm")
    sim.step(1)
    base = read(sim)
    mask = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    out, run = np.nonzero(mask == 0)[0], np.nonzero(mask)[0]
    sim.step(2, mask=torch.from_numpy(mask).cuda())
    after = read(sim)
    names = ROWS + sim.outputs + ("status", "status_sticky")
    same_bits(after, base, names, out)
    assert all((after["qpos"][w] != base["qpos"][w]).any() and (after["site_xpos"][w] != base["site_xpos"][w]).any() for w in run)
    sim.forward(mask=mask)      # a host array works as well
    fwd = read(sim)
    same_bits(fwd, base, names, out)
    assert all((fwd["site_xpos"][w] != after["site_xpos"][w]).any() for w in run)
    sim.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_outputs_are_optional():
    bare, full = make("arm", outputs=()), make("arm")
    for sim in (bare, full):
        sim.step(3)
    a, b = read(bare), read(full)
    same_bits(a, b, ROWS + ("status",))
    assert bare.outputs == () and set(a) == set(ROWS) | {"status", "status_sticky"}
    for k in S.ALL_OUTPUTS:
        assert not hasattr(bare, k) and k not in bare._t
        assert hasattr(full, k)
    bare.close(); full.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstep", [1, 4])
def test_overflow_rerun(nstep):
    sc = S.SCENES["pile"]
    want = S.oracle_run(sc, N, nstep)
    assert (want["ncon"][1:] > S.PILE_MAXCON).all() and want["ncon"][0] <= S.PILE_MAXCON      # worlds 1 .. overflow the fast tables, world 0 does not
    assert (S.oracle_sensitivity(sc, N, nstep) < C.SENS_MAX).all()
    sim = make("pile", overflow="rerun")
    sim.step(nstep)
    got = read(sim)
    compare(f"pile rerun step({nstep})", got, want, S.FLOAT_FIELDS)
    assert (got["status"] == 0).all() and (got["status_sticky"] == 0).all(), (got["status"], got["status_sticky"])
    assert sorted(sim.lane.entered_last_step().tolist()) == [1, 2, 3, 4]
    sim.close()


def test_overflow_flag():
    sc = S.SCENES["pile"]
    want = S.oracle_run(sc, N, 1)
    assert (want["ncon"][1:] > S.PILE_MAXCON).all()
    sim = make("pile", overflow="flag")
    assert sim.lane is None
    sim.step(1)
    got = read(sim)
    assert ((got["status"][1:] & 6) != 0).all() and ((got["status_sticky"][1:] & 6) != 0).all(), got["status"]
    assert (got["ncon"][1:] == S.PILE_MAXCON).all()
    assert got["status"][0] == 0
    compare("pile flag world 0", got, want, S.FLOAT_FIELDS, worlds=[0])
    assert sim.status_counts()["con_overflow"] + sim.status_counts()["efc_overflow"] >= N - 1
    sim.clear_status()
    assert sim.status_counts()["con_overflow"] == 0
    sim.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["arm", "mocap", "rk4"])
def test_four_substeps_are_four_launches(scene):
    one, four = make(scene), make(scene)
    four.step(4)
    for _ in range(4):
        one.step(1)
    a, b = read(one), read(four)
    same_bits(a, b, ROWS + one.outputs + ("status", "status_sticky"))
    one.close(); four.close()


# 8 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_round_trip():
    a = make("mocap")
    a.step(2)
    saved = a.get_state()
    assert set(saved) >= {"qpos", "qvel", "qacc_warmstart", "ctrl", "mocap_pos", "mocap_quat"} and all(isinstance(v, np.ndarray) for v in saved.values())
    b = make("mocap", st={k: np.zeros_like(v) + (1.0 if k in ("qpos", "mocap_quat") else 0.0) for k, v in S.SCENES["mocap"].states(N).items()})
    b.set_state(saved)
    a.step(1); b.step(1)
    same_bits(read(a), read(b), ROWS + a.outputs + ("status", "status_sticky"))
    with pytest.raises(ValueError, match="qvel"):
        b.set_state(dict(saved, qvel=saved["qvel"][:, :-1]))
    with pytest.raises(ValueError, match="qpos"):
        b.set_state(dict(saved, qpos=saved["qpos"][:-1]))
    a.close(); b.close()


# the argument checks of grx_sim_step that need a model (the others: tests/test_cpu_sim.py) ------------------------------------------------------------------
def test_model_dependent_argument_checks():
    import torch

    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd.mjcf import compile_mjcf

    L = _native.lib()
    z = torch.zeros(64, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(model, **null):
        H, I, F = model.pack()
        h = _native.acquire_model(H, I, F, 0)
        try:
            b = _native.SimBuffersStruct(**{k: z.data_ptr() for k in ("qpos", "qvel", "qacc_ws", "ctrl", "mocap_pos", "mocap_quat", "status")})
            for k in null:
                setattr(b, k, None)
            return L.grx_sim_step(h, ctypes.byref(b), 1, 1, 0, stream), L.grx_last_error().decode()
        finally:
            torch.cuda.synchronize()
            _native.release_model(h)

    rc, msg = call(S.SCENES["arm"].model, ctrl=True)
    assert rc == -1 and "ctrl" in msg
    for k in ("mocap_pos", "mocap_quat"):
        rc, msg = call(S.SCENES["mocap"].model, **{k: True})
        assert rc == -1 and "mocap" in msg
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.xml")
        with open(p, "w") as fh:
            fh.write(S.MOCAP_XML)
        moved = compile_mjcf(p, origin=(0.1, 0.0, 0.5))
    rc, msg = call(moved)
    assert rc == -1 and "origin" in msg
