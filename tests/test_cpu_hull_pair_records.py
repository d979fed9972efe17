"""The hull-pair records (GrxModel::reci_hpair / recf_hpair, built at model creation by csrc/grx_host_model.h::grx_build_records): the set-up of a queued hull-vs-convex pair
(csrc/grx_eng_collision.h, grx_mesh_pairs) reads ONE record per pair instead of walking ~25 model tables.  That only changes where a value is loaded from: every record field IS
the table entry it replaces, and the lane emulator -- the same engine source -- steps the folded-arm fixture to the same bits with the records and without them
(GRX_NO_HULLPAIR_RECORDS at model creation: the table walk)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
RHI, RHF = 12, 8      # GRX_RHI / GRX_RHF (csrc/grx_engine.h)


def _records(model):
    from gymnasium_robotics_amd import _native

    L = _native.lib()
    L.grx_model_hull_pair_records.restype = ctypes.c_int
    L.grx_model_hull_pair_records.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int]
    H, I, F = model.pack()
    n = L.grx_model_hull_pair_records(H.ctypes.data, I.ctypes.data, F.ctypes.data, None, None, 0)
    ri, rf = np.zeros((max(n, 1), RHI), np.int32), np.zeros((max(n, 1), RHF), np.float32)
    assert L.grx_model_hull_pair_records(H.ctypes.data, I.ctypes.data, F.ctypes.data, ri.ctypes.data, rf.ctypes.data, n) == n
    return n, ri, rf


@pytest.mark.parametrize("task", ["FetchReach", "FetchPush", "FetchSlide", "FetchPickAndPlace"])
def test_every_record_field_is_the_table_entry_it_replaces(task, monkeypatch):
    from gymnasium_robotics_amd.envs.fetch import load_fetch_model

    monkeypatch.delenv("GRX_NO_HULLPAIR_RECORDS", raising=False)
    monkeypatch.delenv("GRX_NO_HULLCELLS", raising=False)
    model = load_fetch_model(task)
    T = {k: np.asarray(v) for k, v in model.tables.items()}
    g1, g2 = T["pair_geom1"].ravel(), T["pair_geom2"].ravel()
    gtype, gsize = T["geom_type"].ravel(), T["geom_size"].reshape(-1, 3).astype(np.float32)
    hadr, hnum = T["geom_hulladr"].ravel(), T["geom_hullnum"].ravel()
    rec = T["devpair_geoms"].ravel().astype(np.int64) & 0xFFFFFFFF
    mesh = ((rec >> 28) == 7) & (((rec >> 24) & 0xF) != 0)      # hull against a primitive or another hull: what grx_collision queues for grx_mesh_pairs
    mesh_pairs = np.unique(T["devpair"].ravel()[mesh])
    n, ri, rf = _records(model)
    assert len(mesh_pairs) > 0 and n == len(g1), (len(mesh_pairs), n, len(g1))
    with_cells = 0
    for p in mesh_pairs:
        a, b = int(g1[p]), int(g2[p])
        assert (ri[p, 0], ri[p, 1]) == (a, b) and (ri[p, 2], ri[p, 3]) == (gtype[a], gtype[b])
        assert ri[p, 3] == 7 and ri[p, 2] != 0
        assert rf[p, 0] == np.float32(T["pair_margin"].ravel()[p])
        assert np.array_equal(rf[p, 1:4], gsize[a]) and np.array_equal(rf[p, 4:7], gsize[b])
        for s, g in enumerate((a, b)):
            adr, num, cb = ri[p, 4 + 2 * s], ri[p, 5 + 2 * s], ri[p, 8 + s]
            if gtype[g] == 7:
                assert (adr, num) == (hadr[g], hnum[g]) and num > 0
                # the candidate lists exist for the hulls of at least 64 vertices that take part in such a pair (grx_pack_model): the record says which
                assert (cb >= 0) == (num >= 64), (p, g, cb, num)
                with_cells += int(cb >= 0)
            else:
                assert (adr, num, cb) == (0, 0, -1)
        assert ri[p, 10] == 3      # neighbour records and candidate lists exist in a model with hull pairs
    assert with_cells > 0
    # the records of two geoms of one mesh share the lists: equal hull address and count <=> equal cell base
    hulls = {}
    for p in mesh_pairs:
        for s in range(2):
            if ri[p, 2 + s] == 7 and ri[p, 8 + s] >= 0:
                assert hulls.setdefault((ri[p, 4 + 2 * s], ri[p, 5 + 2 * s]), ri[p, 8 + s]) == ri[p, 8 + s]
    # the switch leaves the table out
    monkeypatch.setenv("GRX_NO_HULLPAIR_RECORDS", "1")
    assert _records(model)[0] == 0


def test_emulated_rollouts_are_bit_identical_with_and_without_the_records(monkeypatch):
    """The FetchHullContacts fixture (folded-arm poses: hull pairs queued, cached directions re-checked and portal searches run in most substeps) through the lane emulator: from
    every 6th snapshot the world runs 3 steps on its own state, once on a model with the records and once on one created with GRX_NO_HULLPAIR_RECORDS.  State rows, the gripper
    pose, observation, achieved goal and status word are bit-identical after every step, and queued pairs really went through the set-up (both counts below are positive)."""
    import emu_fp64_check as E
    import emu_sim

    L = ctypes.CDLL(emu_sim.build())
    L.emu_create.restype = ctypes.c_void_p
    L.emu_create.argtypes = [ctypes.c_void_p] * 3
    L.emu_mesh_stat.restype = ctypes.c_long
    keep = E.as_fp64_struct
    E.as_fp64_struct = lambda s: s
    try:
        m, t, g, kind = E._fixture("hull")
    finally:
        E.as_fp64_struct = keep
    assert kind == "fetch"
    H, I, F = m.pack()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64), dtype=np.float32).copy()
    runs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("GRX_NO_HULLPAIR_RECORDS", "1")
        else:
            monkeypatch.delenv("GRX_NO_HULLPAIR_RECORDS", raising=False)
        h = L.emu_create(H.ctypes.data, I.ctypes.data, F.ctypes.data)      # (the switch is read here: model creation)
        s0 = [L.emu_mesh_stat(k) for k in range(2)]
        rows = []
        for i in range(0, g["obs"].shape[0], 6):
            qp, qv, qa = f(m.rows_from_world("qpos", g["qpos"][i])), f(g["qvel"][i]), f(g["qacc_ws"][i])
            mocap, aux, a = f(m.rows_from_world("mocap", g["mocap"][i])), f(m.rows_from_world("aux", g["aux"][i])), f(g["action"][i])
            for k in range(3):
                obs, ach, st = np.zeros(g["obs"].shape[1], np.float32), np.zeros(3, np.float32), ctypes.c_int(0)
                L.emu_fetch_step(ctypes.c_void_p(h), ctypes.byref(t), p(qp), p(qv), p(qa), p(mocap), p(aux), p(a), p(obs), p(ach), ctypes.byref(st))
                rows.append(np.concatenate([qp, qv, qa, mocap, aux, obs, ach, [np.float32(st.value)]]).copy())
        runs.append((np.array(rows), [L.emu_mesh_stat(k) - s0[k] for k in range(2)]))
        L.emu_destroy(ctypes.c_void_p(h))
    (with_rec, s_with), (without, s_without) = runs
    assert s_with[0] > 0 and s_with[1] > 0, s_with      # queued pairs whose cached direction still separated, and queued pairs that went on to a portal search
    assert s_with == s_without
    assert np.array_equal(with_rec.view(np.uint32), without.view(np.uint32))
