"""The narrow phase contact by contact on the DEVICE ENGINE SOURCE (lane emulator, fp32) against the fp64 oracle's list: the case tables of tests/contact_matrix_cases.py --
the 42 pair groups of the engine matrix at their start poses, seven rest-* groups of multi-contact poses and two crowd-* scenes for the driver of grx_collision (queues of
more than one entry, the compaction sweep, the order of the list).  The emulator copies the list out between grx_make_constraint and grx_velocity (emu_contact_list), where
grx_sim_contacts_p1 reads it on the device; tests/test_gpu_contact_matrix.py runs the same tables through grx.BatchedSim.  Also here, from the oracle and the model
tables alone: the preconditions of the new groups and the caps."""
import json
import os

import numpy as np
import pytest

import contact_matrix_cases as M
import engine_matrix_cases as C

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_matrix.json")))


def emulate(group):
    """per variant a list over its cases of the emulator's contact list, in the form M.accept takes; a crowd scene runs on the re-run tables (the emulator has no overflow
    lane: it runs the engine on the tables the device's re-run launch has)"""
    from emu_sim import EmuSim

    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd.core import RERUN_CAPACITY

    out = []
    for var in group.variants:
        model = var.model.with_capacity(**RERUN_CAPACITY) if group.kind == "crowd" else var.model
        e = EmuSim(model, _native.PointTaskStruct(1, 1, 1, 1, 0.45, 5.0))
        t = model.tables
        g1, g2, cd = (np.asarray(t[k]).reshape(-1) for k in ("pair_geom1", "pair_geom2", "pair_condim"))
        rows = []
        for i in range(len(var.idx)):
            e.qpos[:], e.qvel[:] = var.q0[i], var.v0[i]
            got = e.contact_list(M.RERUN_MAXCON)
            p = got["pair"]
            assert got["ncon"] == len(p), (group.name, var.idx[i], "the list is cut", got["ncon"], len(p))
            rows.append(dict(status=got["status"], ncon=got["ncon"], contact_geom=np.stack([g1[p], g2[p]], axis=1).astype(np.int64).reshape(-1, 2), contact_dim=cd[p].astype(np.int64),
                             contact_dist=got["dist"], contact_pos=got["pos"], normal=got["normal"]))
        out.append(rows)
    return out


@pytest.mark.parametrize("name", M.NAMES)
def test_emulated_contact_list_equals_the_oracle(name):
    group = M.group(name)
    M.accept(group, emulate(group), M.min_share(group, RECORD), tangents=False)


def test_record_and_caps():
    """from the oracle alone: the record holds every group with its case count and its compared share; at least 80 % of the cases of the pair groups are compared"""
    from gymnasium_robotics_amd.core import RERUN_CAPACITY

    assert (RERUN_CAPACITY["maxcon"], RERUN_CAPACITY["maxefc"]) == (M.RERUN_MAXCON, M.RERUN_MAXEFC)
    assert len(M.PAIR_NAMES) == 42 and len(M.REST_NAMES) == 7 and len(set(M.NAMES)) == len(M.NAMES) == 51
    assert sum(C.group(n).n for n in M.PAIR_NAMES) == 1858
    compared = total = 0
    for name in M.NAMES:
        group = M.group(name)
        got = M.counts(group)
        rec = RECORD["groups"][name]
        assert (rec["cases"], rec["compared"], rec["multi"]) == (group.n,) + got, (name, rec, group.n, got)
        if name in M.PAIR_NAMES:
            compared, total = compared + got[0], total + group.n
    print("pair groups: compared", compared, "of", total)
    assert compared >= 0.8 * total, (compared, total)
    assert sorted(n for n in M.PAIR_NAMES if C.group(n).cylinder_face) == sorted(n for n, r in RECORD["groups"].items() if r["family"] == "cylinder-face") and \
        sum(C.group(n).cylinder_face for n in M.PAIR_NAMES) == 6


# what each pose class of a rest group has to show at least once, and the fewest contacts any of its cases may have
_REST_COUNTS = {"rest-box": dict(face=4, edge=2), "rest-capsule": dict(lying=2), "rest-cylinder": dict(cap=3, side=2), "rest-ico12": dict(face=3, edge=2),
                "rest-ico42": dict(face=3), "rest-box-box": {"aligned": 4, "turned": 6, "edge-face": 2, "edge-edge": 1}, "rest-ellipsoid": dict(axis=1, between=1)}
_ONE_CONTACT = {"rest-ellipsoid": ("axis", "between"), "rest-box-box": ("edge-edge",)}      # one contact by geometry: a smooth body on a plane, two crossing edges


@pytest.mark.parametrize("name", M.REST_NAMES)
def test_rest_groups_hold_multi_contact_poses(name):
    """From the oracle alone: at least 8 cases; every case has at least two contacts -- but for the two pose classes that have one by geometry, an ellipsoid on a plane and an
    edge laid across an edge, which must have exactly one; each pose class reaches its contact count in every one of its cases; condim cycles over 1 / 3 / 4 / 6; 90 % of
    the cases are compared."""
    group = M.group(name)
    assert group.n >= 8 and group.kind == "rest"
    dims = set()
    for var in group.variants:
        for i in range(len(var.idx)):
            want = M.oracle_list(var, i)
            label, n = group.labels[var.idx[i]], len(want["contact_dim"])
            dims |= set(want["contact_dim"].tolist())
            assert n == _REST_COUNTS[name][label], (name, var.idx[i], label, n)
            assert n >= 2 or label in _ONE_CONTACT.get(name, ()), (name, var.idx[i], label, n)
            assert (want["contact_dist"] < 0.004).all() and want["contact_dist"].min() > -3.5e-3, (name, var.idx[i], want["contact_dist"])
        margin = float(np.asarray(var.model.tables["pair_margin"]).reshape(-1)[0])
        assert name != "rest-ico42" or margin > 0, (name, margin)
    assert set(group.labels.values()) == set(_REST_COUNTS[name]) and dims == {1, 3, 4, 6}, (name, dims)
    compared, multi = M.counts(group)
    print(name, "compared", compared, "of", group.n, "multi-contact", multi)
    assert compared >= 0.9 * group.n


@pytest.mark.parametrize("name", M.CROWD_NAMES)
def test_crowd_scenes_load_the_driver(name):
    """From the model tables and the oracle alone, in every world: the list fits the re-run tables (64 contacts, 256 rows); crowd-boxes has at least nine box-box pairs in
    contact -- more than one pass of the eight-pair queue -- next to plane contacts, and more contacts than the default tables hold; crowd-mixed has more than 64 candidate pairs,
    all seven geom types free and static, and at least one contact from each class of the driver.  90 % of the worlds are compared."""
    group = M.group(name)
    assert [len(v.idx) for v in group.variants] == list(M.CROWD_WORLDS) and group.n == 18
    for var in group.variants:
        t = var.model.tables
        ty, body = np.asarray(t["geom_type"]).reshape(-1), np.asarray(t["geom_bodyid"]).reshape(-1)
        npair = var.model.dim("npair")
        assert len(np.asarray(t["pair_geom1"]).reshape(-1)) == npair > 64, (name, npair)      # the sweep compacts more than one round of candidates
        if name == "crowd-mixed":
            assert {int(x) for x in ty[body == 0]} == {0, 2, 3, 4, 5, 6, 7} and {int(x) for x in ty[body > 0]} == {2, 3, 4, 5, 6, 7}
            assert sorted(int(k) for k in np.asarray(t["geom_meshnum"]).reshape(-1) if k) == [12, 12, 42, 42, 42]
        for i in range(len(var.idx)):
            want = M.oracle_list(var, i)
            n = len(want["contact_dim"])
            cls = [M.contact_class(var.model, int(a), int(b)) for a, b in want["contact_geom"]]
            boxed = {(int(a), int(b)) for (a, b), c in zip(want["contact_geom"], cls) if c == "box-box"}
            print(name, "world", var.idx[i], "ncon", n, "nefc", want["nefc"], "candidate pairs", npair, "box-box pairs in contact", len(boxed), {c: cls.count(c) for c in M.CLASSES})
            assert n <= M.RERUN_MAXCON and want["nefc"] <= M.RERUN_MAXEFC, (name, var.idx[i], n, want["nefc"])
            if name == "crowd-boxes":
                assert len(boxed) >= 9 and cls.count("analytic") >= 4 and n > 32, (name, var.idx[i], len(boxed), n)
            else:
                assert all(cls.count(c) >= 1 for c in M.CLASSES), (name, var.idx[i], cls)
    compared, multi = M.counts(group)
    print(name, "compared", compared, "of", group.n)
    assert compared >= 0.9 * group.n


def test_helpers_on_hand_made_data():
    """contact_class follows the branches of grx_collision; accept() refuses an error over the bound and a list that is a contact short"""
    var = M.group("crowd-mixed").variants[0]
    ty = np.asarray(var.model.tables["geom_type"]).reshape(-1)
    g = lambda t, k=0: int(np.nonzero(ty == t)[0][k])
    mesh = {int(np.asarray(var.model.tables["geom_meshnum"]).reshape(-1)[x]): x for x in np.nonzero(ty == 7)[0]}
    assert M.contact_class(var.model, g(0), g(2)) == "analytic" and M.contact_class(var.model, g(3), g(6)) == "analytic" and M.contact_class(var.model, g(0), g(5)) == "analytic"
    assert M.contact_class(var.model, g(6), g(6, 1)) == "box-box" and M.contact_class(var.model, g(2), g(5)) == "convex" and M.contact_class(var.model, g(4), g(6)) == "convex"
    assert M.contact_class(var.model, mesh[12], g(2)) == "hull" and M.contact_class(var.model, mesh[42], mesh[12]) == "hull"
    assert M.contact_class(var.model, g(0), mesh[12]) == "plane-mesh-small" and M.contact_class(var.model, mesh[42], g(0)) == "plane-mesh-large"
    group = M.group("rest-box")
    dev = emulate(group)
    M.accept(group, dev, 0.9, tangents=False)
    var, rows = next((v, r) for v, r in zip(group.variants, dev) if any(x["ncon"] == 4 for x in r))
    row = next(x for x in rows if x["ncon"] == 4)
    keep = row["contact_pos"].copy()
    row["contact_pos"] = keep + np.float32(2e-4) * np.eye(3, dtype=np.float32)[0]
    with pytest.raises(AssertionError, match="over the bound"):
        M.accept(group, dev, 0.9, tangents=False)
    row["contact_pos"] = keep
    row["contact_geom"] = row["contact_geom"][:3]
    with pytest.raises(AssertionError):
        M.accept(group, dev, 0.9, tangents=False)
