"""grx.BatchedSim and grx_sim_step without a GPU: the symbol and the struct layout, the argument checks of the C entry point that are decided before a launch, the name
lookups and the constructor's checks, and -- on the oracle alone -- the preconditions of tests/test_gpu_sim.py: every world of every compared scene is well-posed for
the oracle (sensitivity below SENS_MAX), and the pile's worlds hold the contact counts the overflow test relies on."""
import ctypes

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S
from gymnasium_robotics_amd import _native


def test_symbols_exist():
    L = _native.lib()
    assert hasattr(L, "grx_sim_step") and hasattr(L, "grx_sim_layout")
    assert {"grx_sim_step", "grx_sim_layout"} <= set(_native.EXPORTED_SYMBOLS)


def test_struct_layout_matches_the_header():
    """sizeof and every member offset of _native.SimBuffersStruct against what the compiled header reports (grx_sim_layout)"""
    L = _native.lib()
    n = L.grx_sim_layout(None, 0)
    out = (ctypes.c_longlong * n)()
    assert L.grx_sim_layout(out, n) == n
    fields = [name for name, _ in _native.SimBuffersStruct._fields_]
    assert n == 1 + len(fields)
    assert fields == ["qpos", "qvel", "qacc_ws", "ctrl", "mocap_pos", "mocap_quat", "xpos", "xquat", "site_xpos", "site_xmat", "site_xvelp", "site_xvelr", "sensordata",
                      "ncon", "nefc", "status", "mask", "lane"]
    assert ctypes.sizeof(_native.SimBuffersStruct) == out[0]
    assert [getattr(_native.SimBuffersStruct, f).offset for f in fields] == list(out[1:])
    assert ctypes.sizeof(_native.OverflowLaneStruct) == out[0] - out[len(fields)]      # the lane is the last member and fills the rest


def _call(model, buf, n_worlds=1, nstep=1, forward_only=0):
    L = _native.lib()
    rc = L.grx_sim_step(model, None if buf is None else ctypes.byref(buf), n_worlds, nstep, forward_only, None)
    return rc, L.grx_last_error().decode()


def test_argument_checks_before_the_launch():
    """The checks that do not need the model come first and read nothing of it (include/grx_capi.h), so a dummy non-NULL handle reaches them on a machine without a device.
    The model-dependent ones (ctrl, mocap, origin) are in tests/test_gpu_sim.py."""
    dummy = ctypes.create_string_buffer(1 << 16)      # never read on these paths
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    words = (ctypes.c_float * 64)()
    p = ctypes.addressof(words)
    full = lambda: _native.SimBuffersStruct(qpos=p, qvel=p, qacc_ws=p, status=p)
    assert _call(None, full()) == (-1, "grx_sim_step: null model")
    assert _call(h, None) == (-1, "grx_sim_step: null buffers")
    for name in ("qpos", "qvel", "qacc_ws"):
        b = full()
        setattr(b, name, None)
        assert _call(h, b) == (-1, "grx_sim_step: null state buffer (qpos, qvel, qacc_ws)")
    b = full()
    b.status = None
    assert _call(h, b) == (-1, "grx_sim_step: null status buffer")
    for n in (0, -3):
        assert _call(h, full(), n_worlds=n) == (-1, "grx_sim_step: n_worlds < 1")
    for k in (0, -1):
        rc, msg = _call(h, full(), nstep=k)
        assert rc == -1 and msg.startswith("grx_sim_step: nstep < 1")


def test_name_lookups_without_a_device():
    import gymnasium_robotics_amd as grx

    sc = S.SCENES["arm"]
    sim = grx.BatchedSim(sc.model, num_worlds=4, outputs=("site_xpos", "sensordata"))
    assert sim._t is None      # nothing allocated, no library loaded
    t = sc.model.tables
    assert (sim.nq, sim.nv, sim.nu, sim.nsite, sim.nmocap, sim.ntouch) == (11, 10, 4, 2, 0, 1)
    assert sim.site_id("ee") == sc.model.names["site"]["ee"] and sim.site_id("pad") != sim.site_id("ee")
    assert sim.body_id("link4") == sc.model.names["body"]["link4"] and sim.body_id("world") == 0
    assert [sim.actuator_id(f"a{k}") for k in (1, 2, 3, 4)] == [0, 1, 2, 3]
    assert [sim.joint_qposadr(f"j{k}") for k in (1, 2, 3, 4)] == [0, 1, 2, 3] and sim.joint_qposadr("boxj") == 4
    assert sim.joint_dofadr("boxj") == 4 and sim.joint_dofadr("j3") == int(np.asarray(t["jnt_dofadr"]).reshape(-1)[sc.model.names["joint"]["j3"]])
    with pytest.raises(KeyError, match="pedestal") as e:      # a static child of the world: merged, no row of its own
        sim.body_id("pedestal")
    assert "body" in str(e.value) and "link1" in str(e.value)
    for fn, kind in ((sim.site_id, "site"), (sim.actuator_id, "actuator"), (sim.mocap_id, "mocap"), (sim.joint_qposadr, "joint"), (sim.joint_dofadr, "joint")):
        with pytest.raises(KeyError, match=kind):
            fn("nope")
    with pytest.raises(AttributeError, match="not requested"):
        sim.xpos
    mo = grx.BatchedSim(S.SCENES["mocap"].model, num_worlds=2)
    assert mo.mocap_id("target") == 0 and mo.nmocap == 1
    assert sim._t is None and mo._t is None


def test_constructor_argument_checks():
    import gymnasium_robotics_amd as grx

    m = S.SCENES["rk4"].model
    with pytest.raises(ValueError, match="site_xvel"):
        grx.BatchedSim(m, num_worlds=2, outputs=("site_xpos", "site_xvel"))
    with pytest.raises(ValueError, match="overflow"):
        grx.BatchedSim(m, num_worlds=2, overflow="drop")
    with pytest.raises(ValueError, match="num_worlds"):
        grx.BatchedSim(m, num_worlds=0)
    with pytest.raises(ValueError, match="capacity"):
        grx.BatchedSim(m, num_worlds=2, capacity=dict(rows=3))
    with pytest.raises(ValueError, match="compile_kwargs"):
        grx.BatchedSim(m, num_worlds=2, compile_kwargs=dict(keep_sites=("tip",)))
    with pytest.raises(ValueError, match="origin"):
        grx.BatchedSim("unused.xml", num_worlds=2, compile_kwargs=dict(origin=(1.0, 0.0, 0.0)))
    sim = grx.BatchedSim(m, num_worlds=2, capacity=dict(maxcon=16), outputs=["nefc", "xpos"])
    assert sim.outputs == ("xpos", "nefc") and sim.model.dim("maxcon_req") == 16 and m.dim("maxcon_req") == 0


@pytest.mark.parametrize("scene,nstep", S.STEP_CASES + [(s, 0) for s in ("arm", "mocap", "rk4")])
@pytest.mark.parametrize("n", [S.N_WORLDS, 13])
def test_every_world_is_well_posed_for_the_oracle(scene, nstep, n):
    """the precondition of the GPU comparisons, where there is no GPU: no world is excluded, so every start has to pass"""
    sens = S.oracle_sensitivity(S.SCENES[scene], n, nstep)
    print(scene, nstep, n, "oracle sensitivity", sens)
    assert (sens < C.SENS_MAX).all(), (scene, nstep, [(i, float(s)) for i, s in enumerate(sens) if not s < C.SENS_MAX])


def test_scenes_exercise_what_they_are_for():
    arm = S.oracle_run(S.SCENES["arm"], S.N_WORLDS, 1)
    assert (arm["ncon"] == 4).all() and (arm["sensordata"] > 0.5).all()      # the box rests on the plane and the touch zone reads its weight
    ctrl = S.SCENES["arm"].states(S.N_WORLDS)["ctrl"]
    lo, hi = np.array([-1.0, -1.0, -0.3, -0.5]), np.array([1.0, 1.0, 1.0, 0.5])
    assert ((ctrl < lo) | (ctrl > hi)).any()      # some controls lie outside their ctrlrange: the actuation stage's clamp is compared
    mo = S.oracle_run(S.SCENES["mocap"], S.N_WORLDS, 1)
    assert (mo["ncon"] >= 1).all() and (mo["nefc"] >= 6 + 4).all()      # the weld's six rows and the peg's contact
    mp = S.SCENES["mocap"].states(S.N_WORLDS)["mocap_pos"]
    assert len({tuple(r) for r in mp[:, 0]}) == S.N_WORLDS      # the mocap pose differs per world
    rk = S.oracle_run(S.SCENES["rk4"], S.N_WORLDS, 1)
    assert S.SCENES["rk4"].model.dim("integrator") == 1 and (rk["ncon"] == 0).all()


@pytest.mark.parametrize("n", [S.N_WORLDS])
def test_pile_contact_counts(n):
    """world 0 fits the fast tables, every other world exceeds the 8-contact list and fits core.RERUN_CAPACITY"""
    from gymnasium_robotics_amd.core import RERUN_CAPACITY

    sc = S.SCENES["pile"]
    assert sc.model.dim("maxcon_req") == S.PILE_MAXCON == 8
    for nstep in (0, 1, 4):
        r = S.oracle_run(sc, n, nstep)
        assert r["ncon"][0] == 4 and r["nefc"][0] <= sc.model.dim("maxefc_req")
        assert (r["ncon"][1:] == 14).all() and (r["ncon"][1:] > S.PILE_MAXCON).all()
        assert (r["ncon"] <= RERUN_CAPACITY["maxcon"]).all() and (r["nefc"] <= RERUN_CAPACITY["maxefc"]).all()
        assert (S.oracle_sensitivity(sc, n, nstep) < C.SENS_MAX).all()
