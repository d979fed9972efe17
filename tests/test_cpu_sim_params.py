"""Per-world model parameters of grx.BatchedSim without a GPU: the symbols, the argument checks of the C entry points that are decided before anything touches a device, the
constructor's checks and pair_ids, the record-fill functions of the commit kernel against the model creation's own record builder (byte for byte, through the host-only
entry grx_sim_params_records), and -- on the oracle alone -- the preconditions of tests/test_gpu_sim_params.py: every drawn world is well-posed for its edited oracle
(sensitivity below SENS_MAX) and differs from the nominal model by more than a hundred bounds in a compared field.  No world is left out of either."""
import ctypes

import numpy as np
import pytest

import engine_matrix_cases as C
import sim_params_cases as P
from gymnasium_robotics_amd import _native
from gymnasium_robotics_amd import sim as sim_module

NEW = ("grx_sim_params_create", "grx_sim_params_destroy", "grx_sim_params_row", "grx_sim_params_commit", "grx_sim_step_params", "grx_sim_params_names", "grx_sim_params_records")


def test_symbols_and_names():
    L = _native.lib()
    assert all(hasattr(L, s) for s in NEW) and set(NEW) <= set(_native.EXPORTED_SYMBOLS)
    n = L.grx_sim_params_names(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    assert L.grx_sim_params_names(buf, n + 1) == n
    names = buf.value.decode().split(", ")
    assert sorted(names) == sorted(sim_module.PARAMS) == sorted(P.ALL) and names[-1] == "gravity" and len(set(names)) == 17
    # the bits of params_invalid as the header defines them
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grx_capi.h")).read()
    bits = {k.lower(): int(v) for k, v in re.findall(r"#define GRX_PARAM_BAD_(\w+) (\d+)", header)}
    assert bits == sim_module.PARAM_BAD


def test_argument_checks_before_any_launch():
    """none of these paths reads the handles: dummy non-NULL pointers reach them on a machine without a device"""
    L = _native.lib()
    err = lambda: L.grx_last_error().decode()
    dummy = ctypes.create_string_buffer(1 << 16)
    h = ctypes.c_void_p(ctypes.addressof(dummy))
    out = ctypes.c_void_p()
    arr = lambda *names: (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
    assert L.grx_sim_params_create(None, None, 4, arr("gravity"), 1, ctypes.byref(out)) == -1 and "null argument" in err()
    assert L.grx_sim_params_create(h, None, 4, arr("gravity"), 1, None) == -1 and "null argument" in err()
    assert L.grx_sim_params_create(h, None, 4, None, 1, ctypes.byref(out)) == -1 and "null names" in err()
    assert L.grx_sim_params_create(h, None, 0, arr("gravity"), 1, ctypes.byref(out)) == -1 and "n_worlds < 1" in err()
    assert L.grx_sim_params_create(h, None, 4, arr("gravity", "geom_size"), 2, ctypes.byref(out)) == -1
    assert "geom_size" in err() and all(name in err() for name in P.ALL)      # the message lists the names
    assert L.grx_sim_params_create(h, None, 4, arr("body_mass", "gravity", "body_mass"), 3, ctypes.byref(out)) == -1 and "named twice" in err()
    assert L.grx_sim_params_create(h, h, 4, arr("gravity"), 1, ctypes.byref(out)) == -1 and "large-table handle" in err()
    assert out.value is None
    ptr, cnt = ctypes.c_void_p(), ctypes.c_int()
    assert L.grx_sim_params_row(None, b"gravity", ctypes.byref(ptr), ctypes.byref(cnt)) == -1 and "null argument" in err()
    assert L.grx_sim_params_row(h, None, ctypes.byref(ptr), ctypes.byref(cnt)) == -1 and "null argument" in err()
    assert L.grx_sim_params_commit(None, None, None, None) == -1 and "null object" in err()
    b = _native.SimBuffersStruct()
    assert L.grx_sim_step_params(None, h, ctypes.byref(b), None, 4, 1, 0, None) == -1 and "null model" in err()
    assert L.grx_sim_step_params(h, None, ctypes.byref(b), None, 4, 1, 0, None) == -1 and "null parameter object" in err()
    assert L.grx_sim_params_destroy(None) == 0
    H, I, F = P.SCENES["armv"].model.pack()
    v = np.zeros(4, dtype=np.float32)
    assert L.grx_sim_params_records(H.ctypes.data, I.ctypes.data, F.ctypes.data, b"geom_size", v.ctypes.data, 4, None, None, 0) == -1 and "geom_size" in err()
    assert L.grx_sim_params_records(H.ctypes.data, I.ctypes.data, F.ctypes.data, b"dof_damping", v.ctypes.data, 4, None, None, 0) == -1 and "10 words" in err()
    assert L.grx_sim_params_records(None, I.ctypes.data, F.ctypes.data, b"dof_damping", v.ctypes.data, 4, None, None, 0) == -1 and "null argument" in err()


def test_constructor_checks_and_pair_ids():
    import gymnasium_robotics_amd as grx

    m = P.SCENES["armv"].model
    with pytest.raises(ValueError, match="geom_size") as e:
        grx.BatchedSim(m, num_worlds=2, model_params=("body_mass", "geom_size"))
    assert all(name in str(e.value) for name in P.ALL)
    with pytest.raises(ValueError, match="twice") as e:
        grx.BatchedSim(m, num_worlds=2, model_params=("gravity", "body_mass", "gravity"))
    assert all(name in str(e.value) for name in P.ALL)
    sim = grx.BatchedSim(m, num_worlds=2, model_params="gravity")
    assert sim.param_names == ("gravity",) and sim._t is None
    plain = grx.BatchedSim(m, num_worlds=2)
    assert plain.param_names == ()
    with pytest.raises(AttributeError, match="model_params"):
        plain.params
    with pytest.raises(AttributeError, match="model_params"):
        plain.params_invalid
    with pytest.raises(RuntimeError, match="model_params"):
        plain.commit_params()
    assert plain._t is None      # nothing was allocated, no library loaded
    # the arm: one candidate pair, the box on the floor
    assert sim.pair_ids("boxg") == [0] and sim.pair_ids("floor") == [0] and sim.pair_ids("boxg", "floor") == [0] and sim.pair_ids("boxg", "boxg") == [0]
    with pytest.raises(KeyError, match="geom"):
        sim.pair_ids("nope")
    # the pile: fourteen spheres against the floor and the neighbouring spheres against each other
    pile = grx.BatchedSim(P.SCENES["pile"].model, num_worlds=2)
    t = pile.model.tables
    g1, g2 = np.asarray(t["pair_geom1"]).reshape(-1), np.asarray(t["pair_geom2"]).reshape(-1)
    floor = pile.model.names["geom"]["floor"]
    ids = pile.pair_ids("floor")
    assert ids == sorted(ids) and len(ids) >= 14 and all(floor in (g1[p], g2[p]) for p in ids) and all(floor not in (g1[p], g2[p]) for p in range(len(g1)) if p not in ids)
    other = next(name for name, g in pile.model.names["geom"].items() if g != floor)
    both = pile.pair_ids(other, "floor")
    assert len(both) == 1 and {g1[both[0]], g2[both[0]]} == {floor, pile.model.names["geom"][other]}
    assert sim._param_shape("jnt_range") == (2, 5, 2) and sim._param_shape("jnt_stiffness") == (2, 5) and sim._param_shape("pair_friction") == (2, 1, 5)
    assert sim._param_shape("gravity") == (2, 3) and sim._param_shape("act_gainprm") == (2, 4, 3) and sim._param_shape("body_inertia") == (2, 6, 6)


def _records(model, name, values):
    L = _native.lib()
    H, I, F = model.pack()
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    n = L.grx_sim_params_records(H.ctypes.data, I.ctypes.data, F.ctypes.data, name.encode(), v.ctypes.data, v.size, None, None, 0)
    assert n >= 0, L.grx_last_error().decode()
    a, b = np.full(max(n, 1), np.nan, dtype=np.float32), np.full(max(n, 1), np.nan, dtype=np.float32)
    assert L.grx_sim_params_records(H.ctypes.data, I.ctypes.data, F.ctypes.data, name.encode(), v.ctypes.data, v.size, a.ctypes.data, b.ctypes.data, n) == n
    return n, a[:n], b[:n]


DEPENDENT_WORDS = dict(body_mass=0, body_inertia=0, gravity=None)      # tables no record is gathered from (gravity is no table at all)


@pytest.mark.parametrize("scene", ["armv", "pile"])
@pytest.mark.parametrize("name", [n for n in P.ALL if n != "gravity"])
def test_record_fill_equals_the_record_builder(scene, name):
    """the records the commit kernel's fill functions give are byte for byte those of grx_build_records with the same edit: for the nominal row (so a record built from
    nominal values IS the shared one) and for every drawn world's row"""
    sc = P.SCENES[scene]
    nom = P.nominal(sc, name)
    rows = [nom] + list(P.draw(sc, (name,))[name])
    total = 0
    for k, row in enumerate(rows):
        n, fill, build = _records(sc.model, name, row)
        assert fill.tobytes() == build.tobytes(), (scene, name, k)
        if name in DEPENDENT_WORDS:
            assert n == 0
            continue
        if row.size == 0:
            continue
        assert n > 0 and np.isfinite(build).all()
        total += n
        if k == 0:
            first = build.copy()
        else:      # the edit is visible in the records: every drawn value that differs from the nominal one appears
            changed = np.unique(np.float32(row).reshape(-1)[np.float32(row).reshape(-1) != np.float32(nom).reshape(-1)])
            assert np.isin(changed, build).all() and (changed.size == 0 or build.tobytes() != first.tobytes()), (scene, name, k)
    print(scene, name, "record words compared:", total)


@pytest.mark.parametrize("group,scene", P.GROUP_CASES)
def test_every_drawn_world_is_well_posed_and_differs_from_the_nominal_model(group, scene):
    sc = P.SCENES[scene]
    rows = P.draw(sc, P.GROUPS[group])
    for name, a in rows.items():
        own = len({r.tobytes() for r in a}) == P.N or not P.nominal(sc, name).any()      # (a table of zeros stays one: frictionloss of rk4, the force ranges)
        assert a.shape[0] == P.N and own, (name, "every world has its own row")
        assert (C.f32(a) == a).all()
    for nstep in P.STEPS:
        run = P.oracle_run(sc, group, rows, P.N, nstep, ())
        sens = P.oracle_sensitivity(sc, group, rows, P.N, nstep)
        ratio = P.distance_from_nominal(sc, run, P.N, nstep)
        print(group, scene, nstep, "sensitivity", sens, "distance / (100 x bound)", ratio)
        assert (sens < C.SENS_MAX).all(), (group, scene, nstep, "a world its own oracle is not sure of: replace the draw", sens)
        assert (ratio > 1.0).all(), (group, scene, nstep, "a world within a hundred bounds of the nominal model: replace the draw", ratio)


@pytest.mark.parametrize("scene", ["armv", "rk4"])
def test_dynamics_block_draws_are_well_posed_and_differ(scene):
    """the preconditions of the dynamics-block comparison on the GPU, for ITS combination of parameters and ITS fields: every compared field of every world moves less
    than SENS_MAX under the jitter, and every world differs from the nominal model by more than a hundred bounds in one of them"""
    sc = P.SCENES[scene]
    rows = P.draw(sc, P.DYN_PARAMS)
    for nstep in (0, 1):
        run = P.oracle_run(sc, "dynamics", rows, P.N, nstep, ())
        sens = P.oracle_sensitivity(sc, "dynamics", rows, P.N, nstep, dyn_fields=P.DYN_FIELDS)
        ratio = P.distance_from_nominal(sc, run, P.N, nstep, dyn_fields=P.DYN_FIELDS, dyn_bounds=P.dyn_bounds())
        print(scene, nstep, "sensitivity", sens, "distance / (100 x bound)", ratio)
        assert (sens < C.SENS_MAX).all(), (scene, nstep, sens)
        assert (ratio > 1.0).all(), (scene, nstep, ratio)


def test_pile_draws_keep_the_overflow():
    """the pile with per-world gravity and pair friction: world 0 still fits the 8-contact list, the others still exceed it, and every world is well-posed and differs"""
    import sim_cases as S

    sc = P.SCENES["pile"]
    rows = P.draw(sc, P.PILE_PARAMS)
    for nstep in (1, 4):
        run = P.oracle_run(sc, "pile", rows, P.N, nstep, ())
        assert run["ncon"][0] <= S.PILE_MAXCON and (run["ncon"][1:] > S.PILE_MAXCON).all()
        assert (P.oracle_sensitivity(sc, "pile", rows, P.N, nstep) < C.SENS_MAX).all()
        assert (P.distance_from_nominal(sc, run, P.N, nstep) > 1.0).all()
