"""Applied forces of grx.BatchedSim on the GPU (pytest -m gpu): qfrc_applied, xfrc_applied and xipos against the fp64 oracle through the three equivalences of
tests/sim_applied_cases.py (motor twin, gravity twin, closed form of one pass).  N = 5 worlds, 13 once.  The preconditions (every world of every case moves less than SENS_MAX
under a one-ulp jitter of the start, differs from its force-free twin by more than ten bounds, and has the contact state the case is for) are asserted on the oracle alone in
tests/test_cpu_sim_applied.py.  Every requested output starts as NaN: the launch owes every element.

Bounds, all the project's own: the float fields of sim_cases.FLOAT_FIELDS and xipos within engine_matrix_cases.BOUND (1e-4) absolute; ncon / nefc equal; the dynamics outputs
as tests/test_gpu_sim_dynamics.py holds them (qM and the Jacobians BOUND absolute, the vectors sim_dyn_cases.error within its vector_bounds(); these cases set no bound); the
contact outputs as tests/test_gpu_sim_contacts.py compares them.  Every figure is printed before it is asserted; tests/golden/sim_applied_errors.json holds the figures
measured on the MI355X (with GRX_APPLIED_ERRORS_OUT=<path> the module writes the table of its run there)."""
import ctypes
import json
import os

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_applied_cases as A
import sim_cases as S
import sim_contact_cases as K
import sim_dyn_cases as D
import sim_params_cases as P
import test_gpu_sim_contacts as GK
import test_gpu_sim_dynamics as G

pytestmark = pytest.mark.gpu

N = A.N
ROWS = G.ROWS
PLAIN = S.ALL_OUTPUTS                     # the nine plain outputs
EVERYTHING = S.ALL_OUTPUTS + D.DYNAMICS
BOTH = ("qfrc_applied", "xfrc_applied")
ALL_APPLIED = BOTH + ("xipos",)
FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    path = os.environ.get("GRX_APPLIED_ERRORS_OUT")
    if path:
        with open(path, "w") as fh:
            json.dump(FIGURES, fh, indent=1)


def make(scene, n=N, outputs=EVERYTHING, applied=ALL_APPLIED, st=None, rows=None, **kw):
    """a BatchedSim of the scene with the start rows loaded (zero warm start), the applied rows written and every requested output filled with NaN"""
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sc = A.SCENES[scene]
    jac = D.JAC_SITES[scene] if any(o in ("site_jacp", "site_jacr") for o in outputs) else None
    sim = grx.BatchedSim(sc.model, num_worlds=n, outputs=outputs, jac_sites=jac, applied=applied, **kw)
    st = sc.states(n) if st is None else st
    for k in ("qpos", "qvel", "ctrl", "mocap_pos", "mocap_quat"):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    load(sim, rows or {})
    for k in sim.outputs + tuple(a for a in sim.applied if a == "xipos"):
        t = getattr(sim, k)
        t.fill_(float("nan")) if t.dtype.is_floating_point else t.fill_(GK.SENTINEL)
    return sim


def load(sim, rows):
    import torch

    for k in BOTH:
        if k in rows:
            getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(rows[k], dtype=np.float32)).reshape(getattr(sim, k).shape))


def read(sim, names=None):
    import torch

    torch.cuda.synchronize()
    names = ROWS + sim.outputs + sim.contacts + sim.applied if names is None else names
    out = {k: getattr(sim, k).cpu().numpy().copy() for k in names}
    out["status"], out["status_sticky"] = sim.status.cpu().numpy().copy(), sim.status_sticky.cpu().numpy().copy()
    return out


def go(sim, nstep):
    sim.step(nstep) if nstep else sim.forward()
    return read(sim)


def check_fields(tag, got, want, nstep, worlds=None, fields=S.FLOAT_FIELDS + ("xipos",)):
    """the float fields within BOUND, the counts equal; returns {field: worst error}"""
    sel = slice(None) if worlds is None else list(worlds)
    worst = {}
    for k in fields:
        if k not in got or not np.asarray(want[k]).size or (k == "qpos" and nstep == 0):      # forward() leaves qpos as given
            continue
        assert np.isfinite(got[k][sel]).all(), (tag, k, "non-finite (a NaN is an element the launch did not write)")
        worst[k] = float(np.abs(got[k][sel].astype(np.float64) - np.asarray(want[k])[sel].reshape(got[k][sel].shape)).max())
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in worst.items()), f"(bound {C.BOUND:.0e})")
    for k in ("ncon", "nefc"):
        if k in got:
            assert (got[k][sel] == want[k][sel]).all(), (tag, k, got[k], want[k])
    for k, v in worst.items():
        assert v < C.BOUND, (tag, k, v)
    return worst


def record(tag, *parts):
    FIGURES[tag] = {k: float(f"{v:.3e}") for p in parts for k, v in p.items()}


def twin_sim(scene, n, **kw):
    sc = A.SCENES[scene]
    rows = A.twin_rows(sc, n)
    return make(scene, n, rows=rows, **kw)


# 1 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep,n", A.TWIN_CASES)
def test_motor_and_gravity_twins(scene, nstep, n):
    """device: ctrl = u1, qfrc_applied = u2, xfrc_applied = m_b a.  Oracle: ctrl = u1 + u2 / gear, gravity g + a.  All float fields, the counts, all ten dynamics outputs.
    Two of the ten need the twin's bookkeeping undone first: the twin books u2 under qfrc_actuator and the a-term under qfrc_bias, where MjData -- and the device --
    book the applied terms under neither.  sim_applied_cases.twin_world subtracts exactly those two terms from the twin's own last pass (checked on the oracle alone in
    tests/test_cpu_sim_applied.py test_twin_bookkeeping_is_exact); without that the first run of this test missed qfrc_bias by 0.8, the size of m a."""
    sim = twin_sim(scene, n)
    got, want = go(sim, nstep), A.twin_run(scene, n, nstep)
    sim.close()
    tag = f"{scene}/{nstep}/{n}"
    record(tag, check_fields(tag, got, want, nstep), G.check(tag, got, want))
    assert (got["status"] == 0).all(), got["status"]


# 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_closed_form_of_one_pass():
    """random forces and torques on every body, the box included, and random qfrc_applied, after forward(): qfrc_smooth and qacc_smooth everywhere, qacc where nefc == 0;
    qfrc_bias, qfrc_passive and qfrc_actuator are the force-free oracle's: none of them contains Q"""
    sim = make("push", rows=A.form_rows())
    got, want = go(sim, 0), A.form_run()
    sim.close()
    free = np.nonzero(want["nefc"] == 0)[0]
    assert len(free) >= 2 and (got["nefc"] == want["nefc"]).all()
    a = G.check("push closed form", got, want, ("qfrc_smooth", "qacc_smooth", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qM"))
    b = G.check("push closed form, nefc == 0", got, want, ("qacc",), worlds=free)
    record("push/closed-form/5", a, b, check_fields("push closed form", got, want, 0))
    assert (got["status"] == 0).all()


# 3 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_torque_through_the_chain_with_contacts_elsewhere():
    """forces and torques on the chain's bodies only; step(1) against the oracle with ctrl += Q"""
    sim = make("push", rows=A.form_rows(chain_only=True))
    got, want = go(sim, 1), A.chain_run()
    sim.close()
    assert (want["ncon"] == 4).sum() >= 3
    record("push/chain/5", check_fields("push chain", got, want, 1), G.check("push chain", got, want, ("qM", "qfrc_smooth", "qacc_smooth", "qacc", "qfrc_constraint", "qfrc_bias", "qfrc_passive")))
    assert (got["status"] == 0).all()


# 4 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("applied", [("qfrc_applied", "xfrc_applied", "xipos"), ("xipos",)])
def test_xipos(applied):
    """after forward() and after step(4) (one substep stale, as xpos); also as the only name of the block"""
    import torch

    sc = A.SCENES["push"]
    only = applied == ("xipos",)
    sim = make("push", outputs=("xpos",), applied=applied, rows=None if only else A.twin_rows(sc))
    assert sim._frc is not None
    for nstep in (0, 4):
        got = go(sim, nstep)
        want = A.twin_run("push", N, nstep, applied=not only)
        w = check_fields(f"push xipos{' alone' if only else ''} nstep={nstep}", got, want, nstep, fields=("xpos", "xipos"))
        record(f"push/xipos{'-alone' if only else ''}/{nstep}", w)
        assert (np.abs(got["xipos"][:, 1:] - got["xpos"][:, 1:]).max(axis=2) > 5e-3).all()      # not xpos: body_ipos != 0 in every movable body
        for k in ("qpos", "qvel", "ctrl"):      # the next launch starts where the case starts
            getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(sc.states(N)[k], dtype=np.float32)))
        sim.qacc_warmstart.zero_()
    sim.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_inputs_are_held_and_untouched():
    sim = twin_sim("push", N, outputs=PLAIN)
    before = read(sim, BOTH)
    sim.step(1); sim.step(1)
    got = read(sim)
    G.same_bits(got, before, BOTH)
    sc = A.SCENES["push"]
    st = sc.states(N)
    grav, ctrl = A.twin_reference_inputs(sc, A.twin_rows(sc), st)
    two = A._stack([_two_steps(sc, P.edited_oracle(sc, dict(gravity=grav), i), dict(st, ctrl=ctrl), i) for i in range(N)])
    record("push/two-steps/5", check_fields("push step(1); step(1)", got, two, 1))
    assert (np.abs(two["qvel"] - A.twin_run("push", N, 1)["qvel"]).max(axis=1) > 10 * C.BOUND).all()      # the second step did something in every world
    sim.close()


def _two_steps(sc, orc, st, i):
    """step(1); step(1) of the oracle: the warm start of the second launch is the first one's"""
    with P.standing_in(sc, orc):
        S.oracle_world(sc, st, i, 1)
        orc.step(1)
        out = S._read(orc)
    out["xipos"] = orc.xipos.reshape(-1, 3).copy()
    return out


# 6 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep", [("push", 4), ("rk4", 1), ("push", 0)])
def test_zero_rows_change_nothing(scene, nstep):
    """a simulation with the block and all-zero rows against one without: state rows, the nine plain outputs and the status are equal (only the sign of a zero may differ)"""
    old, new = make(scene, outputs=PLAIN, applied=()), make(scene, outputs=PLAIN)
    assert old._frc is None and new._frc is not None
    a, b = go(old, nstep), go(new, nstep)
    for k in ROWS + PLAIN + ("status", "status_sticky"):
        assert np.array_equal(a[k], b[k]), k
    old.close(); new.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_masks_reset_and_state():
    import torch

    sc = A.SCENES["push"]
    sim = twin_sim("push", N, outputs=PLAIN)
    sim.step(1)
    base = read(sim)
    mask = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    out, run = np.nonzero(mask == 0)[0], np.nonzero(mask)[0]
    keep = ROWS + sim.outputs + sim.applied + ("status", "status_sticky")
    sim.step(2, mask=torch.from_numpy(mask).cuda())
    after = read(sim)
    G.same_bits(after, base, keep, out)
    assert all((after[k][w] != base[k][w]).any() for w in run for k in ("qpos", "xipos"))
    sim.forward(mask=mask)
    G.same_bits(read(sim), base, keep, out)
    # get_state / set_state carry the named rows
    state = sim.get_state()
    assert set(BOTH) <= set(state) and "xipos" not in state
    sim.reset(mask=mask)
    now = read(sim, BOTH)
    for k in BOTH:
        assert not now[k][run].any() and now[k][out].tobytes() == base[k][out].tobytes(), k      # reset zeroes the selected worlds' rows only
    sim.set_state(state)
    G.same_bits(read(sim, BOTH + ROWS), state, BOTH + ROWS)
    bare = {k: v for k, v in state.items() if k not in BOTH}
    sim.qfrc_applied.fill_(0.25)
    sim.set_state(bare)      # a state without the keys leaves the rows alone
    assert (read(sim, ("qfrc_applied",))["qfrc_applied"] == 0.25).all()
    sim.close()
    plain = make("push", outputs=(), applied=())
    with pytest.raises(ValueError, match="applied"):
        plain.set_state(state)
    plain.set_state(bare)
    plain.close()
    one = make("push", outputs=(), applied=("qfrc_applied",))
    assert "qfrc_applied" in one.get_state() and "xfrc_applied" not in one.get_state()
    with pytest.raises(ValueError, match="xfrc_applied"):
        one.set_state(state)
    one.close()


# 8 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstep", [1, 4])
def test_overflow_rerun(nstep):
    """worlds 1 .. 4 exceed the fast tables and are run again on the large ones, with their applied rows"""
    want = A.twin_run("pile", N, nstep)
    sim = twin_sim("pile", N, overflow="rerun")
    got = go(sim, nstep)
    tag = f"pile/{nstep}/{N}"
    record(tag, check_fields(tag, got, want, nstep), G.check(tag, got, want))
    assert (got["status"] == 0).all() and (got["status_sticky"] == 0).all(), (got["status"], got["status_sticky"])
    assert sorted(sim.lane.entered_last_step().tolist()) == [1, 2, 3, 4]
    sim.close()


def test_overflow_flag():
    sim = twin_sim("pile", N, overflow="flag")
    got = go(sim, 1)
    assert ((got["status"][1:] & 6) != 0).all() and got["status"][0] == 0
    want = A.twin_run("pile", N, 1)
    check_fields("pile flag world 0", got, want, 1, worlds=[0])
    G.check("pile flag world 0", got, want, worlds=[0])
    sim.close()


# 9 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_with_per_world_parameters():
    """model_params = gravity and body_mass, two worlds edited: xfrc_applied = m_b^w a against the edited oracle with g^w + a, step(4)"""
    sim = make("push", rows=dict(xfrc_applied=A.param_applied()), model_params=A.PARAM_NAMES)
    P.load_params(sim, A.param_rows())
    sim.commit_params()
    got, want = go(sim, 4), A.param_run()
    assert not sim.params_invalid.any()
    sim.close()
    record("push/params/4", check_fields("push params", got, want, 4), G.check("push params", got, want))
    assert (got["status"] == 0).all()


# 10 -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_with_the_contact_block():
    names = ("contact_geom", "contact_pos", "contact_force")
    sim = twin_sim("push", N, outputs=("ncon", "nefc"), contacts=names)
    for k in names:
        getattr(sim, k).fill_(GK.SENTINEL if k in K.INTS else float("nan"))
    got = go(sim, 1)
    cap = sim.contact_capacity
    sim.close()
    sc = A.SCENES["push"]
    st = sc.states(N)
    grav, ctrl = A.twin_reference_inputs(sc, A.twin_rows(sc), st)
    worst = dict(pos=0.0, force=0.0)
    for w in range(N):
        with P.standing_in(sc, P.edited_oracle(sc, dict(gravity=grav), w)):
            want = K.oracle_world(sc, dict(st, ctrl=ctrl), w, 1)
        n = len(want["contact_dim"])
        assert got["ncon"][w] == n and got["nefc"][w] == want["nefc"], (w, got["ncon"][w], n)
        perm = K.match(got["contact_geom"][w, :n], got["contact_pos"][w, :n], want)
        assert (got["contact_geom"][w, perm] == want["contact_geom"]).all() and (got["contact_geom"][w, n:] == -1).all()
        assert np.isfinite(got["contact_pos"][w]).all() and np.isfinite(got["contact_force"][w]).all()
        assert not got["contact_force"][w, n:].view(np.uint32).any() and not got["contact_pos"][w, n:].view(np.uint32).any()
        if n:
            worst["pos"] = max(worst["pos"], float(np.abs(got["contact_pos"][w, perm].astype(np.float64) - want["contact_pos"]).max()))
            worst["force"] = max(worst["force"], K.force_error(got["contact_force"][w, perm], want["contact_force"]))
    print(f"push contacts: contact_pos {worst['pos']:.2e} (bound {C.BOUND:.0e})  contact_force {worst['force']:.2e} (bound {K.force_bound():.0e})")
    record("push/contacts/1", worst)
    assert got["contact_force"].shape == (N, cap, 6) and worst["pos"] < C.BOUND and worst["force"] <= K.force_bound()


# 11 -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_model_dependent_argument_checks():
    """every error of grx_sim_step / _dyn / _con that needs a handle still fires through the new entry; nothing was launched"""
    import torch

    from gymnasium_robotics_amd import _native

    L = _native.lib()
    z = torch.zeros(4096, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, I, F = A.SCENES["rk4"].model.pack()      # two sites, two actuators
    h = _native.acquire_model(H, I, F, 0)
    try:
        p = z.data_ptr()
        frc = _native.SimAppliedStruct(qfrc_applied=p, xfrc_applied=p, xipos=p)
        full = lambda **kw: _native.SimBuffersStruct(**dict({k: p for k in ("qpos", "qvel", "qacc_ws", "ctrl", "status")}, **kw))
        ref = lambda x: None if x is None else ctypes.byref(x)
        call = lambda b, d=None, c=None, f=frc: (L.grx_sim_step_frc(h, None, ref(b), ref(d), ref(c), ref(f), 1, 1, 0, stream), L.grx_last_error().decode())
        for bad in (2, -1):
            d = _native.SimDynamicsStruct(site_jacp=p, njac=2)
            d.jac_site[0], d.jac_site[1] = 1, bad
            rc, msg = call(full(), d)
            assert rc == -1 and "jac_site[1]" in msg and "nsite" in msg, msg
        for k in ("site_jacp", "site_jacr"):
            rc, msg = call(full(), _native.SimDynamicsStruct(**{k: p}))
            assert rc == -1 and "njac == 0" in msg, msg
        rc, msg = call(full(ctrl=None))
        assert rc == -1 and msg.startswith("grx_sim_step: null ctrl buffer"), msg
        rc, msg = call(full(), None, _native.SimContactsStruct(pos=p, ccap=0))
        assert rc == -1 and msg.startswith("grx_sim_step_con: ccap < 1"), msg
        rc, msg = call(full(), None, None, None)
        assert rc == -1 and msg.startswith("grx_sim_step_frc: null applied block"), msg
        torch.cuda.synchronize()
        assert (z == 0).all()      # nothing was launched
    finally:
        torch.cuda.synchronize()
        _native.release_model(h)
