"""The generated scenes of tests/engine_matrix_cases.py on the DEVICE ENGINE SOURCE (lane emulator, fp32) against the live fp64 oracle, one step from the same state:
narrow-phase pairs at random and hand-placed poses, random hinge / slide trees, every size class of the symmetric solve.  The same tables run on the GPU in
tests/test_gpu_engine_matrix.py; this file shows the engine source right where the emulator can (it has no v_readlane solve, MFMA Hessian or DPP reduction)."""
import json
import os

import numpy as np
import pytest

import engine_matrix_cases as C

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
    pairs = [n for n in C.NAMES if not n.startswith(("tree", "solve"))]
    assert len(pairs) == 7 + 2 * 15 + 5 and len(set(C.NAMES)) == len(C.NAMES)
    g = C.group("ico12-ico42-fixed")
    assert sorted(int(k) for k in np.asarray(g.variants[0].model.tables["geom_meshnum"]).reshape(-1) if k) == [12, 42]
    assert C.group("capsule-capsule-fixed").n == 44 and C.group("box-cylinder-free").n == 64 and C.group("sphere-plane").n == 40
    assert sorted(len(v.idx) for v in C.group("sphere-plane").variants) == [2, 2, 3, 3, 7, 7, 8, 8]      # launches that are no multiple of 8 worlds
    trees = [C.group(n).variants[0] for n in C.NAMES if n.startswith("tree")]
    assert sum(v.rk4 for v in trees) == 4 and sum(int(np.asarray(v.model.tables["jnt_type"]).reshape(-1)[0] == 0) for v in trees) == 4


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
