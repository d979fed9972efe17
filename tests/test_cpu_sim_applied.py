"""Applied forces of grx.BatchedSim / grx_sim_step_frc without a GPU: the symbols and the layout of the fourth block, the argument checks that are decided before a launch,
the constructor rules, and -- on the oracle alone -- the preconditions of tests/test_gpu_sim_applied.py for every case it compares (tests/sim_applied_cases.py)."""
import ctypes

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_applied_cases as A
import sim_cases as S
import sim_dyn_cases as D
import sim_params_cases as P
from gymnasium_robotics_amd import _native


def test_symbols_exist():
    L = _native.lib()
    assert hasattr(L, "grx_sim_step_frc") and hasattr(L, "grx_sim_applied_layout")
    assert {"grx_sim_step_frc", "grx_sim_applied_layout"} <= set(_native.EXPORTED_SYMBOLS)


def test_struct_layout_matches_the_header():
    L = _native.lib()
    n = L.grx_sim_applied_layout(None, 0)
    out = (ctypes.c_longlong * n)()
    assert L.grx_sim_applied_layout(out, n) == n
    fields = [name for name, _ in _native.SimAppliedStruct._fields_]
    assert n == 1 + len(fields) and fields == ["qfrc_applied", "xfrc_applied", "xipos"]
    assert ctypes.sizeof(_native.SimAppliedStruct) == out[0]
    assert [getattr(_native.SimAppliedStruct, f).offset for f in fields] == list(out[1:])
    from gymnasium_robotics_amd import sim

    assert sim.APPLIED == tuple(fields)


def _call(model, buf, dyn, con, frc, n_worlds=1, nstep=1, forward_only=0, params=None):
    L = _native.lib()
    ref = lambda x: None if x is None else ctypes.byref(x)
    rc = L.grx_sim_step_frc(model, params, ref(buf), ref(dyn), ref(con), ref(frc), n_worlds, nstep, forward_only, None)
    return rc, L.grx_last_error().decode()


def test_argument_checks_before_the_launch():
    """the checks of the older entry points come first and keep their messages; the new one follows those that need no model"""
    dummy = ctypes.create_string_buffer(1 << 16)      # never read on these paths
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    words = (ctypes.c_float * 64)()
    p = ctypes.addressof(words)
    full = lambda: _native.SimBuffersStruct(qpos=p, qvel=p, qacc_ws=p, status=p)
    dyn, con, frc = (lambda **kw: _native.SimDynamicsStruct(**kw)), (lambda **kw: _native.SimContactsStruct(**kw)), (lambda **kw: _native.SimAppliedStruct(**kw))
    assert _call(None, full(), dyn(), con(), frc()) == (-1, "grx_sim_step: null model")
    assert _call(h, None, None, None, frc(xipos=p)) == (-1, "grx_sim_step: null buffers")
    b = full()
    b.qvel = None
    assert _call(h, b, None, None, frc()) == (-1, "grx_sim_step: null state buffer (qpos, qvel, qacc_ws)")
    b = full()
    b.status = None
    assert _call(h, b, None, None, frc(qfrc_applied=p)) == (-1, "grx_sim_step: null status buffer")
    assert _call(h, full(), None, None, frc(), n_worlds=0) == (-1, "grx_sim_step: n_worlds < 1")
    rc, msg = _call(h, full(), None, None, None, nstep=0)      # the older check wins over the null block
    assert rc == -1 and msg.startswith("grx_sim_step: nstep < 1")
    rc, msg = _call(h, full(), dyn(site_jacp=p, njac=-1), None, frc(xfrc_applied=p))
    assert rc == -1 and msg.startswith("grx_sim_step_dyn: njac outside"), msg
    rc, msg = _call(h, full(), None, con(force=p, ccap=0), frc(xfrc_applied=p))
    assert rc == -1 and msg.startswith("grx_sim_step_con: ccap < 1"), msg
    for d, c in ((None, None), (dyn(), con())):      # dyn and con may be null here; frc may not
        rc, msg = _call(h, full(), d, c, None)
        assert rc == -1 and msg.startswith("grx_sim_step_frc: null applied block"), msg
    assert _call(None, full(), None, None, frc(), params=h) == (-1, "grx_sim_step_params: null model")


def test_constructor_rules():
    import gymnasium_robotics_amd as grx
    from gymnasium_robotics_amd import sim as simmod

    m = A.SCENES["push"].model
    sim = grx.BatchedSim(m, num_worlds=3, applied=["xipos", "qfrc_applied"], outputs=("ncon",))
    assert sim.applied == ("qfrc_applied", "xipos") and sim.outputs == ("ncon",) and sim.contacts == () and sim.dynamics == ()
    assert grx.BatchedSim(m, num_worlds=3, applied="xfrc_applied").applied == ("xfrc_applied",)
    plain = grx.BatchedSim(m, num_worlds=3)
    assert plain.applied == () and plain._frc is None
    sh = sim._shapes()
    assert sh["qfrc_applied"] == (3, sim.nv) and sh["xfrc_applied"] == (3, sim.nbody, 6) and sh["xipos"] == (3, sim.nbody, 3)
    with pytest.raises(AttributeError, match=r"applied=.*xfrc_applied"):
        sim.xfrc_applied
    for k in simmod.APPLIED:
        with pytest.raises(AttributeError, match="applied="):
            getattr(plain, k)
    with pytest.raises(AttributeError, match="not requested"):
        sim.xpos
    for bad in (("cfrc_ext",), ("xipos", "ncon"), ("qfrc_bias",)):
        with pytest.raises(ValueError, match="xfrc_applied"):      # the message lists APPLIED
            grx.BatchedSim(m, num_worlds=3, applied=bad)
    with pytest.raises(ValueError, match="twice.*xfrc_applied"):
        grx.BatchedSim(m, num_worlds=3, applied=("xipos", "qfrc_applied", "xipos"))
    with pytest.raises(ValueError, match="unknown output"):
        grx.BatchedSim(m, num_worlds=3, outputs=("xipos",))      # the block has a keyword of its own
    assert sim.body_id("box") == m.names["body"]["box"] and sim.site_id("com_box") == m.names["site"]["com_box"]
    assert sim._t is None and plain._t is None      # none of this needs a device
    assert simmod.APPLIED == ("qfrc_applied", "xfrc_applied", "xipos") and not set(simmod.APPLIED) & (set(simmod.OUTPUTS) | set(simmod.STATE) | set(simmod.CONTACTS))


def test_state_and_outputs_are_unchanged():
    from gymnasium_robotics_amd import sim as simmod

    assert simmod.STATE == ("qpos", "qvel", "qacc_warmstart", "ctrl", "mocap_pos", "mocap_quat")
    assert simmod.OUTPUTS == S.ALL_OUTPUTS + D.DYNAMICS


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# on the oracle alone
def test_push_is_what_it_is_for():
    sc = A.SCENES["push"]
    m, names = sc.model, sc.model.names["body"]
    assert "lump" not in names and set(A.MOVABLE) <= set(names)      # the jointless child was merged ...
    assert abs(A.body_mass(sc)[names["l2"]] - 0.9) < 1e-6            # ... and its mass went to l2
    ipos = np.asarray(m.tables["body_ipos"], dtype=np.float64).reshape(-1, 3)
    assert all(np.abs(ipos[names[b]]).max() > 5e-3 for b in A.MOVABLE)      # body_ipos != 0 everywhere a force acts
    assert A.motors(sc) == [(0, 1.0), (1, 1.0), (2, 1.0)] and A.motors(A.SCENES["rk4"]) == [(6, 2.0), (8, 0.5)]
    assert not np.asarray(m.tables["act_ctrllimited"]).any()
    for n in (A.N, 13):
        up = np.array([i % 5 in A.UP for i in range(n)])
        assert up.sum() >= 2
        for nstep in (0, 1, 4) if n == A.N else (1,):
            run = A.twin_run("push", n, nstep)
            assert (run["nefc"][up] == 0).all() and (run["ncon"][up] == 0).all(), (n, nstep, run["nefc"])      # the box-up worlds have no rows at all
            assert (run["ncon"][~up] == 4).all(), (n, nstep, run["ncon"])
    for run in (A.form_run(), A.chain_run(), A.param_run()):
        up = np.array([i % 5 in A.UP for i in range(A.N)])
        assert (run["nefc"][up] == 0).all() and (run["ncon"][~up] == 4).all()
    rows = A.twin_rows(sc)
    g = np.linalg.norm(A.gravity(sc))
    lat = np.linalg.norm(rows["accel"][:, :2], axis=1) / g
    assert np.allclose(lat, A.LATERAL, atol=1e-6) and np.abs(rows["accel"][:, 2]).max() <= 3.0 and np.abs(rows["qfrc_applied"]).max() <= 1.0
    f = A.form_rows()
    assert np.abs(f["xfrc_applied"][:, :, 3:]).max() <= 0.5 and (f["xfrc_applied"][:, 0] == 0).all() and (np.abs(f["xfrc_applied"][:, 1:]).max(axis=2) > 0).all()


def test_the_two_forms_of_Q_agree():
    """generalized_any (any site of the subtree, shifted to xipos) against generalized (the centre-of-mass sites) on push, after forward() and after a step"""
    sc = A.SCENES["push"]
    orc, st, rows = S._oracle(sc), sc.states(A.N), A.form_rows()
    for i in range(A.N):
        for nstep in (0, 1):
            A.world(sc, orc, st, i, nstep)
            x = rows["xfrc_applied"][i]
            d = np.abs(A.generalized_any(orc, sc, x) - A.generalized(orc, sc, np.zeros(sc.model.dim("nv")), x)).max()
            assert d <= 1e-12, (i, nstep, d)


@pytest.mark.parametrize("scene", ["push", "rk4", "pile"])
def test_twin_bookkeeping_is_exact(scene):
    """after forward() the twin's qfrc_bias and qfrc_actuator, with the two applied terms moved back (twin_world), are those of the force-free model at the same state:
    on rk4 the sites sit on other bodies than the forces, so this is also the check of generalized_any's shift"""
    twin, free = A.twin_run(scene, A.N, 0), A.twin_run(scene, A.N, 0, applied=False)
    # the rows are fp32 values: each component of m_b a is rounded by at most 2^-24 of itself and enters Q through a Jacobian entry below 1 (lever arms under a metre)
    tol = 2.0 ** -24 * np.abs(A.twin_rows(A.SCENES[scene])["xfrc_applied"]).sum(axis=(1, 2)).max() + 1e-12
    for k in ("qfrc_bias", "qfrc_actuator", "qfrc_passive"):
        d = np.abs(twin[k] - free[k]).max() if twin[k].size else 0.0
        print(f"{scene} {k}: {d:.2e} (tol {tol:.2e})")
        assert d <= tol, (k, d, tol)


def test_each_site_sits_on_its_bodys_centre_of_mass():
    sc = A.SCENES["push"]
    body = [sc.model.names["body"][b] for b in A.MOVABLE]
    site = [sc.model.names["site"]["com_" + b] for b in A.MOVABLE]
    for nstep in (0, 4):
        run = A.twin_run("push", A.N, nstep)
        d = np.abs(run["site_xpos"][:, site] - run["xipos"][:, body]).max()
        print(f"push nstep={nstep}: |site - xipos| {d:.2e}")
        assert d <= 1e-12


@pytest.mark.parametrize("scene,nstep,n", A.TWIN_CASES + A.PILE_CASES)
def test_every_world_is_well_posed_for_the_oracle(scene, nstep, n):
    """the precondition of the GPU comparisons: the twin oracle's own answer moves less than SENS_MAX under the one-ulp jitter of the start, in every world"""
    sens = A.twin_sensitivity(scene, n, nstep)
    print(f"{scene} nstep={nstep} n={n}: sensitivity {np.array2string(sens, precision=2)}")
    assert sens.shape == (n,) and (sens < C.SENS_MAX).all(), sens


def test_closed_form_reproduces_the_gravity_twin():
    """(c) against (b) on the oracle: Q of xfrc_applied = m_b a through the centre-of-mass Jacobians, added to the force-free pass, is the pass under gravity g + a"""
    sc = A.SCENES["push"]
    st, mass = sc.states(A.N), np.asarray(sc.model.tables["body_mass"], dtype=np.float64).reshape(-1)      # the oracle's own fp64 masses: the identity is exact
    g64 = np.asarray(sc.model.tables["opt"], dtype=np.float64).reshape(-1)[1:4]
    acc = A.twin_rows(sc)["accel"]
    orc = S._oracle(sc)
    for i in range(A.N):
        free = A.world(sc, orc, st, i, 0)
        x = np.zeros((sc.model.dim("nbody"), 6))
        x[:, :3] = mass[:, None] * acc[i]
        Q = A.generalized(orc, sc, np.zeros(sc.model.dim("nv")), x)
        twin = A.world(sc, P.edited_oracle(sc, dict(gravity=g64 + acc), i), st, i, 0)
        ds = np.abs(free["qfrc_smooth"] + Q - twin["qfrc_smooth"]).max()
        da = np.abs(free["qacc_smooth"] + np.linalg.solve(free["qM"], Q) - twin["qacc_smooth"]).max()
        print(f"world {i}: qfrc_smooth {ds:.2e} qacc_smooth {da:.2e}")
        assert ds <= 1e-12 and da <= 1e-12
        if twin["nefc"] == 0:
            assert np.abs(twin["qacc"] - twin["qacc_smooth"]).max() <= 1e-12


@pytest.mark.parametrize("scene,nstep,n", A.TWIN_CASES)
def test_every_world_differs_from_its_force_free_twin(scene, nstep, n):
    """more than ten bounds in at least one compared field: a kernel that ignored the applied rows would fail every world of item 1"""
    got, free = A.twin_run(scene, n, nstep), A.twin_run(scene, n, nstep, applied=False)
    ratio = np.zeros(n)
    for k in S.FLOAT_FIELDS:
        if got[k].size and not (k == "qpos" and nstep == 0):
            ratio = np.maximum(ratio, np.abs(got[k] - free[k]).reshape(n, -1).max(axis=1) / C.BOUND)
    for k, lim in P.dyn_bounds().items():
        if k not in D.MATRICES:
            ratio = np.maximum(ratio, D.error(k, got[k], free[k]) / lim)
    print(f"{scene} nstep={nstep} n={n}: distance in bounds {np.array2string(ratio, precision=1)}")
    assert (ratio > 10.0).all(), ratio


def test_closed_form_worlds_differ_from_the_force_free_pass():
    form = A.form_run()
    sc = A.SCENES["push"]
    free = A._stack([A.world(sc, S._oracle(sc), sc.states(A.N), i, 0) for i in range(A.N)])
    lim = P.dyn_bounds()["qacc"]
    assert (D.error("qfrc_smooth", form["qfrc_smooth"], free["qfrc_smooth"]) > 10 * lim).all()
    chain, plain = A.chain_run(), A.twin_run("push", A.N, 1, applied=False)
    assert (np.abs(chain["qvel"] - plain["qvel"]).max(axis=1) > 10 * C.BOUND).all()


@pytest.mark.parametrize("nstep", [1, 4])
def test_pile_keeps_its_contact_counts_under_the_applied_rows(nstep):
    want = A.twin_run("pile", A.N, nstep)
    assert (want["ncon"][1:] > S.PILE_MAXCON).all() and want["ncon"][0] <= S.PILE_MAXCON, want["ncon"]


def test_parameter_case_worlds_differ():
    """item 9: the edited worlds differ from the nominal gravity twin by more than ten bounds"""
    got, nominal = A.param_run(), A.param_run(edited=False)
    d = np.abs(got["qvel"] - nominal["qvel"]).max(axis=1)
    print("parameter case: |qvel - nominal|", d)
    assert (d[list(A.PARAM_WORLDS)] > 10 * C.BOUND).all() and (np.delete(d, A.PARAM_WORLDS) < 1e-6).all(), d      # the others: the nominal masses as fp32 holds them
