"""The generated scenes of tests/engine_matrix_cases.py on the DEVICE ENGINE SOURCE (lane emulator, fp32) against the live fp64 oracle, one step from the same state:
narrow-phase pairs at random and hand-placed poses, random hinge / slide trees, every size class of the symmetric solve.  The same tables run on the GPU in
tests/test_gpu_engine_matrix.py; this file shows the engine source right where the emulator can (it has no v_readlane solve, MFMA Hessian or DPP reduction)."""
import json
import os

import numpy as np
import pytest

import engine_matrix_cases as C
from gymnasium_robotics_amd.mjcf.compiler import OPTS as C_OPTS

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_matrix.json")))


def emulate(group, oracle):
    """every case of the group through EmuSim: physics_steps for the Euler models -- there (ncon, nefc) must equal the oracle's -- and point_step (agent = 1, one
    substep) for the RK4 ones, which physics_steps does not integrate"""
    from emu_sim import EmuSim

    from gymnasium_robotics_amd import _native

    out = []
    for var, (_, cnt, _) in zip(group.variants, oracle):
        e = EmuSim(var.model, _native.PointTaskStruct(1, 1, 1, 1, 0.45, 5.0))
        n = len(var.idx)
        x, st = np.zeros((n, var.nq + var.nv)), np.zeros(n, dtype=np.int64)
        for i in range(n):
            e.qpos[:], e.qvel[:], e.qacc_ws[:] = var.q0[i], var.v0[i], 0.0
            e.status.value = 0
            if var.rk4:
                e.point_step(var.ctrl[i])
            else:
                got = e.physics_steps(1, var.ctrl[i])
                assert got == tuple(cnt[i]), (group.name, var.idx[i], "(ncon, nefc)", got, tuple(cnt[i]))
            x[i], st[i] = np.r_[e.qpos, e.qvel], e.status.value
        out.append((x, st))
    return out


@pytest.mark.parametrize("name", C.NAMES)
def test_emulated_engine_equals_the_oracle(name):
    group = C.group(name)
    oracle = C.oracle_results(group)
    C.accept(group, emulate(group, oracle), oracle, C.min_share(group, RECORD))


def test_case_tables_are_what_they_claim():
    """seven plane groups, fifteen primitive pairs static and free, five mesh groups; 40 random cases (64 where a cylinder's flat face can be hit) plus the hand-placed
    ones; the two meshes compile to 12 and 42 hull vertices (the plane routine's two paths); half of the trees integrate with RK4, half hang on a free joint"""
    pairs = [n for n in C.NAMES if not n.startswith(("tree", "solve", "rows"))]
    assert len(pairs) == 7 + 2 * 15 + 5 and len(set(C.NAMES)) == len(C.NAMES)
    g = C.group("ico12-ico42-fixed")
    assert sorted(int(k) for k in np.asarray(g.variants[0].model.tables["geom_meshnum"]).reshape(-1) if k) == [12, 42]
    assert C.group("capsule-capsule-fixed").n == 44 and C.group("box-cylinder-free").n == 64 and C.group("sphere-plane").n == 40
    assert sorted(len(v.idx) for v in C.group("sphere-plane").variants) == [2, 2, 3, 3, 7, 7, 8, 8]      # launches that are no multiple of 8 worlds
    trees = [C.group(n).variants[0] for n in C.NAMES if n.startswith("tree")]
    assert sum(v.rk4 for v in trees) == 4 and sum(int(np.asarray(v.model.tables["jnt_type"]).reshape(-1)[0] == 0) for v in trees) == 4
    rows = [n for n in C.NAMES if n.startswith("rows")]
    assert tuple(rows) == C.ROWS_GROUPS and len(rows) == 7
    for n in rows:
        g = C.group(n)
        assert g.kind == "rows" and 6 <= g.n <= 8 and all(len(v.idx) % 8 and v.nq >= 2 for v in g.variants), n
        assert len(g.variants) == (2 if n == "rows-options" else 1), n
        for v in g.variants:      # only the groups that say so have a pair of geoms that can collide
            assert (v.model.dim("npair") > 0) == (n.startswith("rows-mixed") or n == "rows-options"), n
            assert np.count_nonzero(np.asarray(v.model.tables["opt"]).reshape(-1)[1:3]) == 2, (n, "gravity along an axis")
    assert sorted(len(v.idx) for v in C.group("rows-options").variants) == [3, 4]
    assert C.group("rows-mixed-rk4").variants[0].rk4 and not C.group("rows-mixed-euler").variants[0].rk4


def _rows(name):
    """[(variant, oracle_rows of its cases)] of a row group"""
    return [(v, C.oracle_rows(v)) for v in C.group(name).variants]


def test_row_groups_test_what_they_claim():
    """From the oracle and the model tables alone: the rows a group is named after are in its worlds, on both sides of every switch."""
    # rows-weld: two welds, twelve equality rows and nothing else; the six rows of the first span both free bodies' dofs
    (var, rows), = _rows("rows-weld")
    t = var.model.tables
    assert len(np.asarray(t["weld_eq"]).reshape(-1)) == 2 and [int(x) >> 20 for x in np.asarray(t["weld_row"]).reshape(-1)] == [12, 3]
    assert all(r["nefc"] == r["ne"] == 12 for r in rows)
    eq_data = np.asarray(t["eq_data"], dtype=np.float64).reshape(-1, 11)
    assert eq_data[0, 10] == 0.7 and eq_data[0, :3].any() and eq_data[1, 10] == 1.0 and (np.asarray(t["eq_solref"]).reshape(-1, 2)[1] < 0).all()
    assert all(3e-4 < np.abs(r["pos"][:3]).max() < 6e-3 and 3e-4 < np.abs(r["pos"][6:9]).max() < 3e-2 for r in rows)      # millimetres off the welded poses, not decimetres
    # rows-jeq: three equalities in the model, two rows in the oracle; the clamp applies; all five polycoef and solimp count
    (var, rows), = _rows("rows-jeq")
    t = var.model.tables
    assert var.model.dim("neq") == 3 and np.asarray(t["eq_active"]).reshape(-1).tolist() == [1, 1, 0]
    assert all(r["nefc"] == r["ne"] == 2 for r in rows)
    assert np.count_nonzero(np.asarray(t["eq_data"]).reshape(-1, 11)[0, :5]) == 5 and np.asarray(t["eq_solimp"]).reshape(-1, 5)[0, 4] == 3.0
    assert np.asarray(t["eq_solref"]).reshape(-1, 2)[1, 0] < 2 * np.asarray(t["opt"]).reshape(-1)[0]
    d = np.asarray(t["jeq_dof"]).reshape(-1, 2)
    chain = np.asarray(t["dof_chainmask"]).reshape(-1, 2)[:, 0]
    body = np.asarray(t["dof_bodyid"]).reshape(-1)
    assert not (chain[body[d[0, 0]]] >> d[0, 1]) & 1 and not (chain[body[d[0, 1]]] >> d[0, 0]) & 1      # neither joint is an ancestor of the other: different branches
    # rows-tendon: only tendon rows; every tendon below, above and inside its range, each in at least one case; the residuals are the oracle's
    (var, rows), = _rows("rows-tendon")
    t = var.model.tables
    num, qa = np.asarray(t["tendon_num"]).reshape(-1), np.asarray(t["wrap_qadr"]).reshape(-1)
    assert num.tolist() == [2, 2, 3] and qa[5] == qa[6] and np.asarray(t["tendon_margin"]).reshape(-1)[1] > 0 and (np.asarray(t["tendon_solref"]).reshape(-1, 2)[1] < 0).all()
    assert [int(x) >> 8 for x in np.asarray(t["tendon_span"]).reshape(-1)] == [3, 5, 4]      # every row spans several dofs
    seen = np.zeros((3, 3), dtype=int)      # [tendon, lower / upper / neither]
    for i, r in enumerate(rows):
        sides, pos = C.tendon_sides(var, i)
        assert r["nefc"] == r["nl"] == r["ntl"] == len(pos) and np.abs(r["pos"] - pos).max() < 1e-12, i
        for k, (lo, hi) in enumerate(sides):
            seen[k] += (lo, hi, not (lo or hi))
    assert (seen >= 1).all(), seen
    # rows-actuator: both clamps are hit from both sides, and the shared joint has two live actuators
    (var, rows), = _rows("rows-actuator")
    assert all(r["nefc"] == 0 for r in rows)
    acts = [C.actuator_forces(var, i) for i in range(C.ROWS_N)]
    g = lambda k: np.asarray(var.model.tables[k]).reshape(-1)
    assert g("act_gaintype").tolist() == [1, 0, 0, 0, 0] and g("act_biastype").tolist() == [1, 1, 0, 1, 1] and g("act_gear")[:3].tolist() == [2.0, 1.0, 3.0]
    limited = [a for a in range(var.nu) if acts[0][a][1] is not None]
    assert limited == [0, 2]
    for a in limited:
        assert sum(c[a][0] < c[a][1][0] for c in acts) >= 2 and sum(c[a][0] > c[a][1][1] for c in acts) >= 2, a
    assert sum(not c[0][3][0] <= c[0][2] <= c[0][3][1] for c in acts) >= 2
    assert all(c[3][4] == c[4][4] and min(abs(c[3][5]), abs(c[4][5])) > 0.05 for c in acts)      # one dof, two forces
    # the oracle's qfrc_actuator is the SUM on that dof
    sim = C._oracle(var.model)
    for i, c in enumerate(acts):
        sim.reset_data()
        sim.qpos[:], sim.qvel[:], sim.ctrl[:] = var.q0[i], var.v0[i], var.ctrl[i]
        sim.forward()
        want = np.zeros(var.nv)
        for a in c:
            want[a[4]] += a[5]
        assert np.abs(sim.qfrc_actuator - want).max() < 1e-12, i
    # rows-mixed: all five row kinds in one world, in at least two cases (here: in every case), behind a trailing free object
    for name in ("rows-mixed-euler", "rows-mixed-rk4"):
        (var, rows), = _rows(name)
        assert 16 <= var.nv <= 24 and C.trailing_free_object(var.model), name
        full = [r for r in rows if r["ncon"] >= 1 and r["ne"] == 14 and r["nf"] >= 1 and r["nl"] - r["ntl"] >= 1 and r["ntl"] >= 1 and r["nefc"] - r["ne"] - r["nf"] - r["nl"] >= 1]
        assert len(full) >= 2, (name, len(full))
        acts = [C.actuator_forces(var, i) for i in range(C.ROWS_N)]
        assert all(c[3][4] == c[4][4] and min(abs(c[3][5]), abs(c[4][5])) > 0.05 for c in acts), name
        assert np.asarray(var.model.tables["jnt_margin"]).reshape(-1).max() > 0
    # rows-options: condim 4, impratio off 1, and the noslip sweeps run on the second variant only
    (va, ra), (vb, rb) = _rows("rows-options")
    opt = lambda v: float(np.asarray(v.model.tables["opt"]).reshape(-1)[C_OPTS.index("impratio")])
    assert opt(va) == 4.0 and opt(vb) == 0.5 and va.model.dim("noslip_iterations") == 0 and vb.model.dim("noslip_iterations") == 3
    assert all(r["noslip_iter"] == 0 and r["ncon"] >= 1 and r["nefc"] == 6 * r["ncon"] for r in ra)
    assert all(r["noslip_iter"] > 0 and r["ncon"] >= 1 and r["nefc"] == 6 * r["ncon"] for r in rb)


def test_what_neither_side_implements_is_refused():
    """An elliptic cone used to run pyramidal on both sides (two condim-4 contacts gave twelve rows), the implicit integrators were parsed and then stepped as Euler, and an
    actuator with a dyntype would have run without its activation state.  The refusals the compiler already had are asserted here too."""
    body = '<body><joint name="j" type="hinge"/><geom type="sphere" size="0.1"/></body>'
    two = body + '<body pos="1 0 0"><joint name="k" type="hinge"/><geom type="sphere" size="0.1"/></body>'
    model = lambda opt="", world=body, more="": f"<mujoco>{opt}<worldbody>{world}</worldbody>{more}</mujoco>"
    for xml, match in ((model('<option cone="elliptic"/>'), "elliptic"),
                       (model('<option integrator="implicit"/>'), "implicit"),
                       (model('<option integrator="implicitfast"/>'), "implicitfast"),
                       (model(more='<actuator><general joint="j" dyntype="integrator"/></actuator>'), "dyntype"),
                       (model(more='<actuator><general joint="j" dyntype="filter" dynprm="0.1"/></actuator>'), "dyntype"),
                       (model(more='<tendon><fixed stiffness="1"><joint joint="j" coef="1"/></fixed></tendon>'), "tendon stiffness"),
                       (model(more='<tendon><fixed damping="1"><joint joint="j" coef="1"/></fixed></tendon>'), "tendon stiffness"),
                       (model(more='<tendon><fixed frictionloss="1"><joint joint="j" coef="1"/></fixed></tendon>'), "tendon stiffness"),
                       (model(more='<tendon><fixed name="t"><joint joint="j" coef="1"/></fixed></tendon><actuator><motor tendon="t"/></actuator>'), "joint transmissions"),
                       (model(world=body.replace("<geom", '<site name="s"/><geom'), more='<actuator><motor site="s"/></actuator>'), "joint transmissions"),
                       (model(world=body.replace("<geom", '<site name="a"/><geom') + '<site name="b" pos="1 0 0"/>', more='<tendon><spatial><site site="a"/><site site="b"/></spatial></tendon>'), "fixed tendons"),
                       (model(world=body.replace("<body>", '<body name="p">'), more='<equality><connect body1="p" anchor="0 0 0"/></equality>'), "equality type connect"),
                       (model(world=two, more='<tendon><fixed name="t"><joint joint="j" coef="1"/></fixed><fixed name="u"><joint joint="k" coef="1"/></fixed></tendon>'
                                             '<equality><tendon tendon1="t" tendon2="u"/></equality>'), "equality type tendon"),
                       (model(world=two.replace("<body>", '<body name="p">', 1), more='<equality><joint joint1="j" joint2="k"/><weld body1="p"/></equality>'), "welds listed after")):
        with pytest.raises(NotImplementedError, match=match):
            C.compile_xml(xml)
    for ok in ('<option cone="pyramidal" integrator="RK4"/>', '<option integrator="Euler"/>'):
        C.compile_xml(model(ok, more='<actuator><general joint="j" dyntype="none"/></actuator>'))


def test_ball_joints_are_refused():
    """A ball joint used to compile (4 qpos, 3 dofs) although neither the engine nor the oracle has one: both moved the quaternion's first word like a slide coordinate
    and agreed with each other on it.  A missing routine is an error, not another motion."""
    with pytest.raises(NotImplementedError, match="ball"):
        C.compile_xml('<mujoco><worldbody><body><joint type="ball"/><geom type="sphere" size="0.1"/></body></worldbody></mujoco>')


def test_most_pair_cases_are_well_posed_for_the_oracle():
    """over all pair groups at least 80 % of the cases are compared (from the oracle alone), and the record holds every group"""
    compared = total = 0
    for name in C.NAMES:
        group = C.group(name)
        assert name in RECORD["groups"] and RECORD["groups"][name]["cases"] == group.n, name
        if group.kind == "pair":
            compared += sum(int((sens < C.SENS_MAX).sum()) for _, _, sens in C.oracle_results(group))
            total += group.n
    assert compared >= 0.8 * total, (compared, total)
