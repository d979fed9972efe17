"""The narrow phase contact by contact on the GPU (pytest -m gpu): the case tables of tests/contact_matrix_cases.py through the contact outputs of grx.BatchedSim.  Each
variant is one BatchedSim with one world per case (a crowd scene: 5 and 13 worlds), the state rows loaded, every requested buffer filled with NaN / SENTINEL, one
forward(), then read.  The same tables run on the lane emulator in tests/test_cpu_contact_matrix.py, which also asserts the preconditions and the caps from the oracle
alone; the device code differs from the emulator exactly where this file looks: DPP reductions in the box-box octets, wave ballots, the cooperative hull scan.

Every case: clean status, finite floats, the slots past ncon hold the fill values bit for bit, the list is in non-decreasing candidate-pair order.  Every compared case
(contact_matrix_cases.accept): equal ncon; after matching equal geom pairs and contact_dim; contact_dist / contact_pos / the normal within engine_matrix_cases.BOUND
(1e-4) of the oracle; the tangents within BOUND of K.make_frame of the device's own normal.

MEASURED (tests/golden/contact_matrix.json, a record and never a bound).  Worst error of the compared cases on the lane emulator: 9.2e-06 (box-cylinder-fixed); on the
MI355X: 8.0e-06 (box-cylinder-fixed), tangents 1.5e-07 (sphere-ellipsoid-free).  Before grx_plane_cylinder placed the rim vector's component along the plane normal by
its identity, rest-cylinder stood at 9.9e-05 on the emulator (a cylinder flat on its cap); it is at 8.5e-08 on both now."""
import json
import os

import numpy as np
import pytest

import contact_matrix_cases as M
import sim_contact_cases as K
import test_gpu_sim_contacts as GK

pytestmark = pytest.mark.gpu

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_matrix.json")))
CONTACTS = ("contact_geom", "contact_dim", "contact_dist", "contact_pos", "contact_frame")


def forward_on_gpu(group, var):
    """one forward() of a BatchedSim of the variant's model, one world per case; returns the list over the cases that M.accept takes.  Asserts the fill values here."""
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    n = len(var.idx)
    sim = grx.BatchedSim(var.model, num_worlds=n, outputs=("ncon",), contacts=CONTACTS)
    try:
        for k, rows in (("qpos", var.q0), ("qvel", var.v0)):
            getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).reshape(getattr(sim, k).shape))
        sim.qacc_warmstart.zero_()
        sim.ctrl.zero_()
        sim.ncon.fill_(GK.SENTINEL)
        for k in sim.contacts:
            getattr(sim, k).fill_(GK.SENTINEL if k in K.INTS else float("nan"))
        sim.forward()
        got = GK.read(sim, ("ncon",) + sim.contacts)
        cap = sim.contact_capacity
    finally:
        sim.close()
    out = []
    for w in range(n):
        tag = (group.name, var.idx[w])
        nc = int(got["ncon"][w])
        assert 0 <= nc <= cap, (tag, "ncon", nc)
        for k in CONTACTS:      # the slots past ncon hold the fill values (floats: 0.0f bit for bit)
            tail = np.ascontiguousarray(got[k][w, nc:])
            assert tail.shape[0] == cap - nc and ((tail == K.FILL[k]).all() if k in K.INTS else not tail.view(np.uint32).any()), (tag, k, "fill")
        frame = got["contact_frame"][w, :nc]
        out.append(dict(status=int(got["status"][w]) | int(got["status_sticky"][w]), ncon=nc, contact_geom=got["contact_geom"][w, :nc].astype(np.int64),
                        contact_dim=got["contact_dim"][w, :nc].astype(np.int64), contact_dist=got["contact_dist"][w, :nc], contact_pos=got["contact_pos"][w, :nc],
                        normal=frame[:, :3], tangents=frame[:, 3:]))
    return out


@pytest.mark.parametrize("name", M.NAMES)
def test_gpu_contact_list_equals_the_oracle(name):
    group = M.group(name)
    M.accept(group, [forward_on_gpu(group, var) for var in group.variants], M.min_share(group, RECORD), tangents=True)


@pytest.mark.parametrize("name", M.CROWD_NAMES)
def test_crowd_contact_forces_add_up_per_body(name):
    """The outputs are ranked by pair on the way out, so where the engine's list is not in pair order (crowd-mixed: the late queues) contact_force has to follow the same
    permutation as contact_geom and contact_frame.  From the device outputs alone, in fp64, after one forward(): a free body's three translational dofs are world-aligned,
    so its entries of qfrc_constraint are the sum over the contacts of its geom of +- frame' force[:3] (+ where it is the pair's second geom).  The allowance is that of
    tests/test_gpu_sim_contacts.py item 2: every force component within force_bound max(1, |force|_inf of the world), every frame entry within BOUND, qfrc_constraint
    within its own bound."""
    import torch

    import engine_matrix_cases as C
    import gymnasium_robotics_amd as grx
    import sim_params_cases as P

    var = M.group(name).variants[0]
    n = len(var.idx)
    sim = grx.BatchedSim(var.model, num_worlds=n, outputs=("ncon", "qfrc_constraint"), contacts=("contact_geom", "contact_frame", "contact_force"))
    try:
        for k, rows in (("qpos", var.q0), ("qvel", var.v0)):
            getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).reshape(getattr(sim, k).shape))
        sim.qacc_warmstart.zero_()
        for k in sim.contacts:
            getattr(sim, k).fill_(GK.SENTINEL if k in K.INTS else float("nan"))
        sim.forward()
        got = GK.read(sim, ("ncon", "qfrc_constraint") + sim.contacts)
    finally:
        sim.close()
    assert (got["status"] == 0).all() and (got["status_sticky"] == 0).all(), (got["status"], got["status_sticky"])
    t = var.model.tables
    gbody, dbody = np.asarray(t["geom_bodyid"]).reshape(-1), np.asarray(t["dof_bodyid"]).reshape(-1)
    fb, qb = K.force_bound(), P.vector_bound("qfrc_constraint")
    worst = 0.0
    for w in range(n):
        nc = int(got["ncon"][w])
        geom = got["contact_geom"][w, :nc]
        frame, force = got["contact_frame"][w, :nc].astype(np.float64).reshape(-1, 3, 3), got["contact_force"][w, :nc, :3].astype(np.float64)
        assert np.isfinite(got["contact_force"][w]).all() and np.abs(force[:, 0]).max() > 0.1, (name, w)
        world = np.einsum("kji,kj->ki", frame, force)      # the force on each pair's second geom
        q = got["qfrc_constraint"][w].astype(np.float64)
        e_f = fb * max(1.0, np.abs(got["contact_force"][w, :nc]).max())
        for b in sorted(set(gbody[gbody > 0].tolist())):
            dof = int(np.nonzero(dbody == b)[0][0])
            sign = np.where(gbody[geom[:, 1]] == b, 1.0, 0.0) - np.where(gbody[geom[:, 0]] == b, 1.0, 0.0)
            sel = np.nonzero(sign)[0]
            assert len(sel) >= 1, (name, w, b)
            total = (sign[sel, None] * world[sel]).sum(axis=0)
            tol = len(sel) * np.sqrt(3.0) * e_f + C.BOUND * np.abs(force[sel]).sum() + qb * max(1.0, np.abs(q).max())
            d = np.abs(total - q[dof:dof + 3]).max()
            worst = max(worst, d / tol)
            assert d <= tol, (name, w, b, d, tol, total, q[dof:dof + 3])
    print(f"{name}: worst |sum frame' force - qfrc_constraint| / allowance {worst:.2e}")
