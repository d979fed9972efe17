"""The contact outputs of grx.BatchedSim on the GPU (pytest -m gpu): the contact list and mj_contactForce against the fp64 oracle on the scenes of tests/sim_contact_cases.py.
N = 5 worlds, 13 once.  The preconditions (every world keeps its contact set and moves less than SENS_MAX under a one-ulp jitter of the start, on the oracle alone) are
asserted in tests/test_cpu_sim_contacts.py for every case compared here.  Every requested float buffer starts as NaN and every int buffer as SENTINEL: the launch owes
every element.

Bounds.  contact_geom, contact_dim: equal.  contact_dist / pos / frame: engine_matrix_cases.BOUND (1e-4) absolute.  contact_force: per world
max |got - want| / max(1, max |want|) within sim_contact_cases.force_bound(), the smallest power of ten >= 4 x the worst figure measured on the MI355X over arm, mocap, cones x
nstep 0, 1, 4 and arm at 13 worlds (tests/golden/sim_contact_errors.json).  Device and oracle contacts are matched per world by geom pair and nearest position."""
import numpy as np
import pytest

import engine_matrix_cases as C
import sim_cases as S
import sim_contact_cases as K

pytestmark = pytest.mark.gpu

N = K.N
ROWS = ("qpos", "qvel", "qacc_warmstart")
SENTINEL = -12345
EXTRA = ("ncon", "nefc", "qfrc_constraint")


def make(scene, n=N, contacts=K.CONTACTS, outputs=EXTRA, st=None, **kw):
    """a BatchedSim of the scene with the scene's start rows loaded (zero warm start), every requested contact buffer filled with NaN / SENTINEL"""
    import torch

    import gymnasium_robotics_amd as grx

    assert torch.cuda.is_available(), "these tests need the GPU"
    sc = K.SCENES[scene]
    sim = grx.BatchedSim(sc.model, num_worlds=n, outputs=outputs, contacts=contacts, **kw)
    st = sc.states(n) if st is None else st
    for k in ("qpos", "qvel", "ctrl", "mocap_pos", "mocap_quat"):
        getattr(sim, k).copy_(torch.from_numpy(np.ascontiguousarray(st[k], dtype=np.float32)).reshape(getattr(sim, k).shape))
    sim.qacc_warmstart.zero_()
    for k in sim.contacts:
        getattr(sim, k).fill_(SENTINEL if k in K.INTS else float("nan"))
    return sim


def read(sim, names=None):
    import torch

    torch.cuda.synchronize()
    names = ROWS + sim.outputs + sim.contacts if names is None else names
    out = {k: getattr(sim, k).cpu().numpy().copy() for k in names}
    out["status"], out["status_sticky"] = sim.status.cpu().numpy().copy(), sim.status_sticky.cpu().numpy().copy()
    return out


def same_bits(a, b, names, worlds=None):
    sel = slice(None) if worlds is None else worlds
    for k in names:
        x, y = np.ascontiguousarray(a[k][sel]), np.ascontiguousarray(b[k][sel])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def run_case(scene, nstep, n, **kw):
    sim = make(scene, n, **kw)
    if nstep:
        sim.step(nstep)
    else:
        sim.forward()
    got = read(sim)
    sim.close()
    return got


def compare_world(tag, got, w, want, cap):
    """one world against the oracle's list after matching; returns dict(geometric=, force=) of the world's errors, printed before they are asserted by the caller"""
    n = len(want["contact_dim"])
    assert got["ncon"][w] == n, (tag, w, "ncon", got["ncon"][w], n)
    perm = K.match(got["contact_geom"][w, :n], got["contact_pos"][w, :n], want)
    assert (got["contact_geom"][w, perm] == want["contact_geom"]).all() and (got["contact_dim"][w, perm] == want["contact_dim"]).all(), (tag, w)
    for k in K.CONTACTS:      # the slots past ncon hold the fill values (floats: 0.0f bit for bit)
        tail = np.ascontiguousarray(got[k][w, n:])
        assert tail.shape[0] == cap - n and ((tail == K.FILL[k]).all() if k in K.INTS else not tail.view(np.uint32).any()), (tag, w, k, "fill")
    # efc_address: sorted, with each contact's row count, the addresses tile [nefc - rows, nefc) exactly
    adr, dim = got["contact_efc_address"][w, :n], got["contact_dim"][w, :n]
    assert ((adr >= 0) == (want["contact_efc_address"][np.argsort(perm)] >= 0)).all(), (tag, w, "which contacts have rows")
    rows = np.array([K.rows_of(d, a) for d, a in zip(dim, adr)])
    order = np.argsort(adr[adr >= 0], kind="stable")
    a_s, r_s = adr[adr >= 0][order], rows[adr >= 0][order]
    nefc = int(got["nefc"][w])
    assert nefc == want["nefc"], (tag, w, "nefc", nefc, want["nefc"])
    if len(a_s):
        assert a_s[0] == nefc - r_s.sum() and (a_s[1:] == a_s[:-1] + r_s[:-1]).all() and a_s[-1] + r_s[-1] == nefc, (tag, w, "addresses", a_s, r_s, nefc)
    for k in K.GEOMETRIC + ("contact_force",):
        assert np.isfinite(got[k][w]).all(), (tag, w, k, "non-finite (a NaN is an element the launch did not write)")
    geo = max([float(np.abs(got[k][w, perm].astype(np.float64) - want[k]).max()) for k in K.GEOMETRIC if want[k].size] or [0.0])
    return dict(geometric=geo, force=K.force_error(got["contact_force"][w, perm], want["contact_force"]))


def check(tag, got, want, cap, worlds=None):
    """every figure is printed before it is asserted; returns the worst errors over the worlds"""
    worlds = range(len(want)) if worlds is None else worlds
    errs = [compare_world(tag, got, w, want[w], cap) for w in worlds]
    worst = {k: max(e[k] for e in errs) for k in ("geometric", "force")}
    bound = K.force_bound()
    print(tag, f"geometric {worst['geometric']:.2e} (bound {C.BOUND:.0e})  contact_force {worst['force']:.2e} (bound {bound:.0e})")
    assert worst["geometric"] < C.BOUND, (tag, worst)
    assert worst["force"] <= bound, (tag, worst, bound)
    return worst


# 1 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep,n", K.CASES)
def test_step_and_forward_equal_the_oracle(scene, nstep, n):
    got, want = run_case(scene, nstep, n), K.oracle_run(scene, n, nstep)
    assert got["contact_force"].shape == (n, 64, 6)
    check(f"{scene} nstep={nstep} n={n}", got, want, 64)
    assert (got["status"] == 0).all(), got["status"]


# 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep", [("arm", 1), ("cones", 0), ("cones", 4)])
def test_contact_forces_add_up_to_qfrc_constraint(scene, nstep):
    """From the device outputs alone, in fp64.  A free body that touches only the plane is the second body of its contacts and its translational dofs are world-aligned, so
    entry i of its three translational entries of qfrc_constraint is sum_k sum_j frame_k[j, i] force_k[j], j < 3.  Allowances summed: item 1 holds each force component
    within e_f = force_bound max(1, |force|_inf of the world) and each frame entry within BOUND, so contact k adds |frame_k[:, i]|_1 e_f <= sqrt(3) e_f and BOUND |force_k[:3]|_1;
    qfrc_constraint is within its bound of tests/test_gpu_sim_dynamics.py times max(1, |qfrc_constraint|_inf)."""
    import sim_params_cases as P

    got = run_case(scene, nstep, N)
    sc = K.SCENES[scene]
    fb, qb = K.force_bound(), P.vector_bound("qfrc_constraint")
    for geom, dof in K.FREE_BODIES[scene]:
        gid = int(sc.model.names["geom"][geom])
        for w in range(N):
            n = int(got["ncon"][w])
            sel = np.nonzero((got["contact_geom"][w, :n] == gid).any(axis=1))[0]
            assert len(sel) >= 1 and (got["contact_geom"][w, sel, 1] == gid).all(), (geom, w, got["contact_geom"][w, :n])
            frame = got["contact_frame"][w, sel].astype(np.float64).reshape(-1, 3, 3)
            force = got["contact_force"][w, sel, :3].astype(np.float64)
            total = np.einsum("kji,kj->i", frame, force)
            q = got["qfrc_constraint"][w].astype(np.float64)
            e_f = fb * max(1.0, np.abs(got["contact_force"][w, :n]).max())
            tol = len(sel) * np.sqrt(3.0) * e_f + C.BOUND * np.abs(force).sum() + qb * max(1.0, np.abs(q).max())
            d = np.abs(total - q[dof:dof + 3]).max()
            print(f"{scene} nstep={nstep} {geom} world {w}: {len(sel)} contacts, |sum frame^T force - qfrc_constraint| {d:.2e} (tol {tol:.2e}, |force| {np.abs(force).max():.2f})")
            assert d <= tol


# 3 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep", [("arm", 4), ("cones", 1)])
def test_no_side_effects(scene, nstep):
    """the same start without and with the block: the state rows, the status and the nineteen old outputs agree bit for bit, for step and for forward"""
    import sim_dyn_cases as D

    jac = D.JAC_SITES[scene] if scene in D.JAC_SITES else None
    outs = S.ALL_OUTPUTS + tuple(k for k in D.DYNAMICS if jac is not None or k not in ("site_jacp", "site_jacr"))
    old, new = make(scene, contacts=(), outputs=outs, jac_sites=jac), make(scene, outputs=outs, jac_sites=jac)
    assert old._con is None and new._con is not None and len(outs) == (19 if jac is not None else 17)
    old.step(nstep); new.step(nstep)
    same_bits(read(old), read(new), ROWS + outs + ("status", "status_sticky"))
    old.forward(); new.forward()
    same_bits(read(old), read(new), ROWS + outs + ("status", "status_sticky"))
    old.close(); new.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_masked_out_worlds_keep_everything():
    import torch

    sim = make("cones")
    sim.step(1)
    base = read(sim)
    mask = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    out, run = np.nonzero(mask == 0)[0], np.nonzero(mask)[0]
    sim.step(2, mask=torch.from_numpy(mask).cuda())
    after = read(sim)
    same_bits(after, base, ROWS + sim.outputs + sim.contacts + ("status", "status_sticky"), out)
    assert all((after[k][w] != base[k][w]).any() for w in run for k in ("contact_dist", "contact_pos", "contact_force"))
    sim.forward(mask=mask)
    same_bits(read(sim), base, ROWS + sim.outputs + sim.contacts + ("status", "status_sticky"), out)
    sim.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep,n", K.PILE_CASES)
def test_overflow_rerun(scene, nstep, n):
    """worlds 1 .. 4 exceed the 8-contact list of the fast tables: the re-run launch takes the same block and lists all fourteen contacts"""
    want = K.oracle_run(scene, n, nstep)
    assert [len(r["contact_dim"]) for r in want] == [4, 14, 14, 14, 14]
    sim = make(scene, overflow="rerun")
    assert sim.contact_capacity == 64 and sim.contact_pos.shape == (n, 64, 3)
    sim.step(nstep)
    got = read(sim)
    check(f"pile rerun step({nstep})", got, want, 64)
    assert (got["status"] == 0).all() and (got["status_sticky"] == 0).all(), (got["status"], got["status_sticky"])
    assert sorted(sim.lane.entered_last_step().tolist()) == [1, 2, 3, 4]
    sim.close()


def test_overflow_flag():
    sim = make("pile", overflow="flag")
    assert sim.contact_capacity == S.PILE_MAXCON
    sim.step(1)
    got = read(sim)
    assert ((got["status"][1:] & 6) != 0).all() and got["status"][0] == 0
    assert all(np.isfinite(got[k]).all() for k in K.GEOMETRIC + ("contact_force",)) and all((got[k] != SENTINEL).all() for k in K.INTS)
    check("pile flag world 0", got, K.oracle_run("pile", N, 1), S.PILE_MAXCON, worlds=[0])
    sim.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,nstep,n", K.FRICTION_CASES)
def test_per_world_pair_friction(scene, nstep, n):
    """pair_friction doubled in worlds 1 and 3 (the kernels with per-world model parameters): the forces follow the oracle with the same table edit, whose mu decodes them;
    tests/test_cpu_sim_contacts.py shows on the oracle alone that the edit moves those worlds' forces by more than a hundred bounds"""
    import sim_params_cases as P

    want = K.oracle_run(scene, n, nstep, edit=True)
    sim = make(scene, n, model_params=("pair_friction",))
    P.load_params(sim, K.friction_rows(n))
    sim.commit_params()
    sim.step(nstep) if nstep else sim.forward()
    got = read(sim)
    assert not sim.params_invalid.any()
    check(f"{scene} friction x2 nstep={nstep}", got, want, 64)
    assert (got["status"] == 0).all()
    sim.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_only_contact_force():
    """a single member (every other pointer of the block is null): bit for bit the forces of the launch that requests all seven, which item 1 holds to the oracle"""
    sim = make("cones", contacts=("contact_force",), outputs=("ncon",))
    sim.step(1)
    got = read(sim)
    full = run_case("cones", 1, N)
    same_bits(got, full, ("contact_force", "ncon") + ROWS)
    with pytest.raises(AttributeError, match="not requested"):
        sim.contact_geom
    sim.close()
