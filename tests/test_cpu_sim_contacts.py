"""The contact outputs of grx.BatchedSim / grx_sim_step_con without a GPU: the symbols and the layout of the third block, the argument checks that are decided before a
launch, the constructor rules, and -- on the oracle alone -- the preconditions of tests/test_gpu_sim_contacts.py for every case it compares (tests/sim_contact_cases.py)."""
import ctypes

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S
import sim_contact_cases as K
from gymnasium_robotics_amd import _native


def test_symbols_exist():
    L = _native.lib()
    assert hasattr(L, "grx_sim_step_con") and hasattr(L, "grx_sim_contacts_layout")
    assert {"grx_sim_step_con", "grx_sim_contacts_layout"} <= set(_native.EXPORTED_SYMBOLS)


def test_struct_layout_matches_the_header():
    """sizeof and every member offset of _native.SimContactsStruct against what the compiled header reports (grx_sim_contacts_layout)"""
    L = _native.lib()
    n = L.grx_sim_contacts_layout(None, 0)
    out = (ctypes.c_longlong * n)()
    assert L.grx_sim_contacts_layout(out, n) == n
    fields = [name for name, _ in _native.SimContactsStruct._fields_]
    assert n == 1 + len(fields)
    assert fields == ["geom", "dim", "efc_address", "dist", "pos", "frame", "force", "ccap"]
    assert ctypes.sizeof(_native.SimContactsStruct) == out[0]
    assert [getattr(_native.SimContactsStruct, f).offset for f in fields] == list(out[1:])
    from gymnasium_robotics_amd import sim

    assert sim.CONTACTS == K.CONTACTS == tuple("contact_" + f for f in fields[:7])      # the order BatchedSim fills the block in


def _call(model, buf, dyn, con, n_worlds=1, nstep=1, forward_only=0, params=None):
    L = _native.lib()
    ref = lambda x: None if x is None else ctypes.byref(x)
    rc = L.grx_sim_step_con(model, params, ref(buf), ref(dyn), ref(con), n_worlds, nstep, forward_only, None)
    return rc, L.grx_last_error().decode()


def test_argument_checks_before_the_launch():
    """the checks of grx_sim_step_dyn come first and keep their messages; the two new ones follow those that need no model"""
    dummy = ctypes.create_string_buffer(1 << 16)      # never read on these paths
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    words = (ctypes.c_float * 64)()
    p = ctypes.addressof(words)
    full = lambda: _native.SimBuffersStruct(qpos=p, qvel=p, qacc_ws=p, status=p)
    dyn, con = (lambda **kw: _native.SimDynamicsStruct(**kw)), (lambda **kw: _native.SimContactsStruct(**kw))
    assert _call(None, full(), dyn(), con()) == (-1, "grx_sim_step: null model")
    assert _call(h, None, dyn(), con()) == (-1, "grx_sim_step: null buffers")
    b = full()
    b.qacc_ws = None
    assert _call(h, b, None, con()) == (-1, "grx_sim_step: null state buffer (qpos, qvel, qacc_ws)")
    b = full()
    b.status = None
    assert _call(h, b, None, con(force=p, ccap=4)) == (-1, "grx_sim_step: null status buffer")
    assert _call(h, full(), None, con(), n_worlds=0) == (-1, "grx_sim_step: n_worlds < 1")
    rc, msg = _call(h, full(), dyn(), None, nstep=0)      # the older check wins over the null block
    assert rc == -1 and msg.startswith("grx_sim_step: nstep < 1")
    rc, msg = _call(h, full(), dyn(site_jacp=p, njac=-1), con(force=p, ccap=0))
    assert rc == -1 and msg.startswith("grx_sim_step_dyn: njac outside"), msg
    rc, msg = _call(h, full(), dyn(qM=p, njac=2), None)
    assert rc == -1 and msg.startswith("grx_sim_step_dyn: njac > 0 with site_jacp and site_jacr both null"), msg
    for d in (None, dyn()):
        rc, msg = _call(h, full(), d, None)
        assert rc == -1 and msg.startswith("grx_sim_step_con: null contact block"), msg
    for k in K.CONTACTS:
        for bad in (0, -3):
            rc, msg = _call(h, full(), None, con(ccap=bad, **{k[len("contact_"):]: p}))
            assert rc == -1 and msg.startswith("grx_sim_step_con: ccap < 1"), (k, msg)
    assert _call(None, full(), None, con(), params=h) == (-1, "grx_sim_step_params: null model")


def test_constructor_rules():
    import gymnasium_robotics_amd as grx
    from gymnasium_robotics_amd import sim as simmod
    from gymnasium_robotics_amd.core import RERUN_CAPACITY

    m = K.SCENES["cones"].model
    sim = grx.BatchedSim(m, num_worlds=3, contacts=["contact_force", "contact_geom"], outputs=("ncon",))
    assert sim.contacts == ("contact_geom", "contact_force") and sim.outputs == ("ncon",) and sim.dynamics == ()
    assert grx.BatchedSim(m, num_worlds=3, contacts="contact_pos").contacts == ("contact_pos",)
    assert grx.BatchedSim(m, num_worlds=3).contacts == ()
    cap = sim.contact_capacity
    assert cap == RERUN_CAPACITY["maxcon"] == 64      # the default: a re-run handle on the large tables
    sh = sim._shapes()
    assert sh["contact_geom"] == (3, cap, 2) and sh["contact_dim"] == sh["contact_efc_address"] == sh["contact_dist"] == (3, cap)
    assert sh["contact_pos"] == (3, cap, 3) and sh["contact_frame"] == (3, cap, 9) and sh["contact_force"] == (3, cap, 6)
    assert grx.BatchedSim(m, num_worlds=3, overflow="flag").contact_capacity == 32      # the compiler's default tables
    pile = K.SCENES["pile"].model
    assert grx.BatchedSim(pile, num_worlds=3, overflow="flag").contact_capacity == S.PILE_MAXCON
    assert grx.BatchedSim(pile, num_worlds=3, overflow="rerun").contact_capacity == 64
    assert grx.BatchedSim(m, num_worlds=3, overflow="flag", capacity=dict(maxcon=12)).contact_capacity == 12
    with pytest.raises(AttributeError, match="not requested"):
        sim.contact_pos
    with pytest.raises(AttributeError, match="not requested"):
        sim.xpos
    for bad in (("contact_wrench",), ("contact_force", "ncon"), ("qM",)):
        with pytest.raises(ValueError, match="contact_efc_address"):      # the message lists CONTACTS
            grx.BatchedSim(m, num_worlds=3, contacts=bad)
    with pytest.raises(ValueError, match="twice.*contact_efc_address"):
        grx.BatchedSim(m, num_worlds=3, contacts=("contact_pos", "contact_dim", "contact_pos"))
    with pytest.raises(ValueError, match="unknown output"):
        grx.BatchedSim(m, num_worlds=3, outputs=("contact_force",))      # the contact outputs have a keyword of their own
    names = m.names["geom"]
    assert {"floor", "g1", "g4", "g6"} <= set(names) and all(sim.geom_id(k) == names[k] for k in names)
    g1, g2 = (np.asarray(m.tables[k]).reshape(-1) for k in ("pair_geom1", "pair_geom2"))
    assert {sim.geom_id("floor"), sim.geom_id("g6")} == {int(g1[sim.pair_ids("g6")[0]]), int(g2[sim.pair_ids("g6")[0]])}      # the ids contact_geom holds
    with pytest.raises(KeyError, match="geom"):
        sim.geom_id("nope")
    assert sim._t is None      # none of this needs a device
    assert len(simmod.CONTACTS) == 7 and not set(simmod.CONTACTS) & set(simmod.OUTPUTS)


def test_outputs_are_unchanged():
    from gymnasium_robotics_amd import sim as simmod

    assert len(simmod.OUTPUTS) == 19 and simmod.OUTPUTS[:9] == S.ALL_OUTPUTS and simmod.OUTPUTS[9:] == simmod.DYNAMICS
    assert simmod.STATE == ("qpos", "qvel", "qacc_warmstart", "ctrl", "mocap_pos", "mocap_quat")      # contacts are not state


def test_restated_decode_and_matching_rule():
    """the helpers the GPU file relies on, on hand-made data"""
    f = np.array([9.0, 1.0, 2.0, 3.0, 5.0, 7.0, 4.0])
    mu = np.array([0.5, 0.25, 0.1, 0.01, 0.02])
    assert K.decode_force(f, 0, 1, mu).tolist() == [9.0, 0, 0, 0, 0, 0]
    assert K.decode_force(f, 1, 3, mu).tolist() == [11.0, 0.5 * (1.0 - 2.0), 0.25 * (3.0 - 5.0), 0, 0, 0]
    assert K.decode_force(f, 1, 4, mu).tolist() == [22.0, -0.5, -0.5, 0.1 * (7.0 - 4.0), 0, 0]
    assert not K.decode_force(f, -1, 4, mu).any()
    assert [K.rows_of(d, 0) for d in (1, 3, 4, 6)] == [1, 4, 6, 10] and K.rows_of(6, -1) == 0
    for nrm in ([0, 0, 1.0], [0, 1.0, 0], [0.6, 0.48, 0.64], [0.0, -0.6, 0.8]):
        fr = K.make_frame(nrm).reshape(3, 3)
        assert np.abs(fr @ fr.T - np.eye(3)).max() < 1e-12 and np.linalg.det(fr) > 0.999 and (fr[0] == nrm).all()
    want = dict(contact_dim=np.array([3, 3, 1]), contact_geom=np.array([[0, 2], [0, 2], [0, 1]]), contact_pos=np.array([[0, 0, 0.0], [1, 0, 0], [5, 5, 5]]))
    dev_geom, dev_pos = np.array([[0, 1], [0, 2], [0, 2]]), np.array([[5, 5, 5.0], [1.01, 0, 0], [0.01, 0, 0]])
    assert K.match(dev_geom, dev_pos, want).tolist() == [2, 1, 0]
    with pytest.raises(AssertionError):
        K.match(dev_geom[:2], dev_pos[:2], want)      # a contact short
    with pytest.raises(AssertionError):
        K.match(np.array([[0, 1], [0, 1], [0, 2]]), dev_pos, want)      # the same count, another pair


ALL_CASES = K.CASES + K.PILE_CASES + [("pile", 0, K.N)]


@pytest.mark.parametrize("scene,nstep,n", ALL_CASES)
def test_every_world_is_well_posed_for_the_oracle(scene, nstep, n):
    """the precondition of the GPU comparisons: under the one-ulp jitter every world keeps its contact set, and the compared floats move less than SENS_MAX"""
    sens = K.oracle_sensitivity(scene, n, nstep)
    print(scene, nstep, n, "contact set kept", sens["same"].all(), f"geometric {sens['geometric'].max():.1e} force {sens['force'].max():.1e}")
    assert sens["same"].all(), (scene, nstep, np.nonzero(~sens["same"])[0])
    assert (sens["geometric"] < C.SENS_MAX).all() and (sens["force"] < C.SENS_MAX).all(), (scene, nstep, sens)


@pytest.mark.parametrize("scene,nstep,n", K.FRICTION_CASES)
def test_doubled_friction_worlds_are_well_posed_and_differ(scene, nstep, n):
    """the per-world parameter case: the same precondition on the edited oracles, and the edit moves the forces of the edited worlds by more than a hundred bounds"""
    sens = K.oracle_sensitivity(scene, n, nstep, edit=True)
    print(scene, nstep, "friction x 2: contact set kept", sens["same"].all(), f"geometric {sens['geometric'].max():.1e} force {sens['force'].max():.1e}")
    assert sens["same"].all() and (sens["geometric"] < C.SENS_MAX).all() and (sens["force"] < C.SENS_MAX).all(), sens
    want, base = K.oracle_run(scene, n, nstep, edit=True), K.oracle_run(scene, n, nstep)
    for w in range(n):
        d = K.force_error(want[w]["contact_force"], base[w]["contact_force"])
        assert (d > 100 * K.force_bound()) if w in K.FRICTION_WORLDS else d < C.SENS_MAX, (w, d)      # (the other worlds: the table as fp32 holds it against the fp64 one)


def test_scenes_are_what_they_are_for():
    bound = K.force_bound()
    for nstep in (0, 1, 4):
        runs = K.oracle_run("cones", K.N, nstep)
        for r in runs:
            assert sorted(r["contact_dim"].tolist()) == [1, 4, 4, 4, 4, 6] and 36 <= r["nefc"] <= 37
            assert r["contact_efc_address"].min() >= 1      # friction-loss and limit rows in front of the contacts' rows
            rows = [K.rows_of(d, a) for d, a in zip(r["contact_dim"], r["contact_efc_address"])]
            assert sum(rows) + r["contact_efc_address"].min() == r["nefc"]
        top = np.abs(np.concatenate([r["contact_force"] for r in runs])).max(axis=0)
        print("cones nstep", nstep, "largest |force component|", top, "100 x bound", 100 * bound)
        assert (top > 100 * bound).all(), (nstep, top, bound)
        mocap = K.oracle_run("mocap", K.N, nstep)
        assert all(len(r["contact_dim"]) == 1 for r in mocap) or nstep == 4      # (after four substeps the peg has left the hand in some worlds)
        assert sum(len(r["contact_dim"]) for r in mocap) >= 1 and all(r["contact_efc_address"].min() >= 6 for r in mocap if len(r["contact_dim"]))      # the weld's six rows come first
    pile = K.oracle_run("pile", K.N, 1)
    assert [len(r["contact_dim"]) for r in pile] == [4, 14, 14, 14, 14]
