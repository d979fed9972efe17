"""CPU tests of the normaliser's reference (tests/norm_refs.py) and of the host surface of the feature: the reference against an independent two-pass mean / variance, its
edge rules, the exported symbols of both libraries, the ctypes mirrors and the state-blob layout, and the argument checks that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import norm_refs as N

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NORM_HEADER = os.path.join(ROOT, "include", "grx_norm.h")
ENV_CALLS = ("create", "destroy", "dims", "update", "apply_batch", "policy_input", "stats", "state_size", "get_state", "set_state")
KERNEL_CALLS = ("geometry", "layout", "update", "refresh", "apply_batch", "apply_packed")


def _rows(rng, n, od, gd, ad, loc=0.0, scale=1.0):
    return (loc + scale * rng.standard_normal((n, N.row_width(od, gd, ad)))).astype(np.float32)


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("od,gd,ad", [(1, 1, 1), (25, 3, 4)])
def test_reference_is_the_two_pass_mean_and_variance(od, gd, ad):
    rng = np.random.default_rng(7)
    batches = [_rows(rng, n, od, gd, ad, loc=3.0, scale=2.0) for n in (1, 64, 257, 1000)]
    st = N.Stats(od + gd)
    for b in batches:
        N.update(st, b, od, gd)
    allrows = np.concatenate(batches)
    x = allrows[:, N.tracked_columns(od, gd)].astype(np.float64)
    assert st.count == len(allrows) and st.skipped == 0
    mean, var = np.mean(x, axis=0), np.var(x, axis=0)      # independent: two passes over the concatenation
    mean_ref, var_ref = st.sum / st.count, st.sumsq / st.count - (st.sum / st.count) ** 2
    np.testing.assert_allclose(mean_ref, mean, rtol=1e-9, atol=0)
    np.testing.assert_allclose(var_ref, var, rtol=1e-9, atol=0)
    m32, is32 = N.refresh(st.sum, st.sumsq, st.count, 1e-2)
    np.testing.assert_array_equal(m32, mean_ref.astype(np.float32))
    np.testing.assert_allclose(1.0 / is32.astype(np.float64), np.sqrt(var), rtol=1e-6)
    # a wrong formula is caught at this tolerance: the unbiased variance, or the mean of the squares alone
    assert not np.allclose(np.var(x, axis=0, ddof=1), var_ref, rtol=1e-9, atol=0)
    assert not np.allclose(st.sumsq / st.count, var, rtol=1e-9, atol=0)


def test_tracked_columns_are_obs_and_the_relabelled_goal():
    od, gd, ad = 4, 2, 2
    W = N.row_width(od, gd, ad)
    assert W == 18
    np.testing.assert_array_equal(N.tracked_columns(od, gd), [0, 1, 2, 3, 6, 7])
    rows = np.arange(3 * W, dtype=np.float32).reshape(3, W)
    s, q, a, kept, skipped = N.batch_sums(rows, od, gd)
    np.testing.assert_array_equal(s, rows[:, [0, 1, 2, 3, 6, 7]].sum(axis=0))
    assert kept == 3 and skipped == 0


def test_eps_floor_and_empty_identity():
    m, s = N.refresh(np.zeros(3), np.zeros(3), 0, 1e-2)
    np.testing.assert_array_equal(m, np.zeros(3, np.float32))
    np.testing.assert_array_equal(s, np.ones(3, np.float32))
    # a constant column: var = 0 -> std = eps; a column whose variance is above eps^2 is not floored
    x = np.array([[2.0, 0.0], [2.0, 1.0], [2.0, 2.0], [2.0, 3.0]])
    m, s = N.refresh(x.sum(0), (x * x).sum(0), 4, 1e-2)
    np.testing.assert_array_equal(m, np.array([2.0, 1.5], np.float32))
    assert s[0] == np.float32(100.0) and s[1] == np.float32(1.0 / np.sqrt(1.25))
    # cancellation can leave a tiny negative variance: floored, never a NaN
    m, s = N.refresh(np.array([3e8]), np.array([3e16 * (1 - 1e-16)]), 3, 1e-2)
    assert np.isfinite(s).all() and s[0] == np.float32(100.0)


def test_apply_order_clip_nan_and_inf():
    mean, inv = np.array([1.0, -2.0], np.float32), np.array([3.0, 0.5], np.float32)
    x = np.array([[1.5, 0.0], [100.0, -100.0], [np.nan, np.inf], [-np.inf, np.nan]], np.float32)
    y = N.normalize(x, mean, inv, 5.0)
    np.testing.assert_array_equal(y[0], np.array([1.5, 1.0], np.float32))
    np.testing.assert_array_equal(y[1], np.array([5.0, -5.0], np.float32))
    assert np.isnan(y[2, 0]) and y[2, 1] == 5.0 and y[3, 0] == -5.0 and np.isnan(y[3, 1])
    # subtract then multiply in fp32, not one fp64 expression rounded once
    xm, mm, sm = np.float32(1.0000001), np.float32(1e-8), np.float32(3.3333333)
    assert N.normalize(xm, mm, sm, 5.0) == np.float32(np.float32(xm - mm) * sm)
    assert N.normalize(np.float32(0.1), np.float32(0.3), np.float32(7.7), 50.0) == np.float32(np.float32(np.float32(0.1) - np.float32(0.3)) * np.float32(7.7))


def test_apply_batch_and_packed_touch_the_right_columns():
    od, gd, ad = 2, 1, 1
    W = N.row_width(od, gd, ad)      # [o o | a | g | u | r | o' o' | a' | s] = 10
    assert W == 10
    mean, inv = np.array([1, 2, 3], np.float32), np.array([2, 2, 2], np.float32)
    rows = np.full((2, W), 4.0, np.float32)
    rows[1, 4:6] = np.nan      # action and reward are copied, whatever they hold
    out = N.apply_batch(rows, mean, inv, od, gd, ad, 5.0)
    np.testing.assert_array_equal(out[0], np.array([5, 4, 2, 2, 4, 4, 5, 4, 2, 4], np.float32))      # (4-1)*2 clipped to 5, (4-2)*2, (4-3)*2
    assert np.isnan(out[1, 4]) and np.isnan(out[1, 5]) and np.isfinite(np.delete(out[1], [4, 5])).all()
    packed = np.array([[4, 4, 9, 4, 0.5, 1.0]], np.float32)      # [o o | a | d | r | s]
    np.testing.assert_array_equal(N.apply_packed(packed, mean, inv, od, gd, 5.0), np.array([[5, 4, 2]], np.float32))


def test_row_skip_rule():
    od, gd, ad = 3, 2, 1
    rng = np.random.default_rng(3)
    rows = _rows(rng, 20, od, gd, ad)
    clean = rows.copy()
    rows[2, 0] = np.nan                  # obs_t
    rows[5, od + gd + 1] = np.inf        # goal
    rows[9, od + gd] = -np.inf
    rows[4, od] = np.nan                 # achieved_t: not tracked
    rows[6, od + 2 * gd] = np.nan        # action
    rows[7, -1] = np.inf                 # success word
    rows[8, od + 2 * gd + ad + 1] = np.nan      # obs_t+1
    st = N.update(N.Stats(od + gd), rows, od, gd)
    assert st.count == 17 and st.skipped == 3
    want = N.update(N.Stats(od + gd), np.delete(clean, [2, 5, 9], axis=0), od, gd)
    np.testing.assert_array_equal(st.sum, want.sum)
    np.testing.assert_array_equal(st.sumsq, want.sumsq)
    before = (st.sum.copy(), st.count, st.skipped)
    N.update(st, rows, od, gd, valid=0)      # the zero-filled slot: nothing changes
    assert (st.count, st.skipped) == before[1:] and (st.sum == before[0]).all()
    N.update(st, rows, od, gd, valid=20)
    assert st.count == 34 and st.skipped == 6


def test_ulp_distance():
    a = np.array([1.0, -1.0, 0.0], np.float32)
    assert (N.ulp_distance(a, a) == 0).all()
    assert N.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert N.ulp_distance(np.float32(-1e-45), np.float32(1e-45)) == 2


# ------------------------------------------------------------------ the host surface
def test_build_links_both_libraries():
    import __graft_entry__ as g

    g.build()
    assert os.path.exists(g.HIP_SO) and os.path.exists(g.ENV_SO)
    for dep in ("grx_norm.h", "grx_env_norm.inc"):
        assert any(os.path.basename(d) == dep for d in g.ENV_DEPS), dep
    assert any(os.path.basename(d) == "grx_normstat.h" for d in g.HIP_DEPS)


def test_kernel_entry_points_are_declared_registered_and_exported():
    from gymnasium_robotics_amd import _native

    names = {"grx_normstat_" + c for c in KERNEL_CALLS}
    header = open(os.path.join(ROOT, "include", "grx_capi.h")).read()
    assert names == set(re.findall(r"\b(grx_normstat_[a-z_]+)\s*\(", header))
    assert names <= set(_native.EXPORTED_SYMBOLS)
    L = _native.lib()      # the symbol check of the loader: a prototype on a missing symbol raises
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert not [n for n in sorted(names) if not hasattr(raw, n)]
    assert L.grx_normstat_update.argtypes is not None and len(L.grx_normstat_update.argtypes) == 9
    assert len(L.grx_normstat_apply_batch.argtypes) == 10 and len(L.grx_normstat_apply_packed.argtypes) == 9


def test_every_declared_norm_entry_point_is_exported():
    from gymnasium_robotics_amd import env_capi as E

    L = E.lib()
    text = open(NORM_HEADER).read()
    names = set(re.findall(r"\b(grx_norm_\w+)\s*\(", text))
    assert names == {"grx_norm_" + c for c in ENV_CALLS}, names
    raw = ctypes.CDLL(E.LIB_PATH)
    assert not [n for n in sorted(names) if not hasattr(raw, n)]
    for n in names:
        assert getattr(L, n).argtypes is not None, n
    assert '#include "grx_env.h"' in text
    for header in ("grx_env.h", "grx_replay.h", "grx_episodes.h"):      # nothing was added to the existing env-level headers
        assert "grx_norm" not in open(os.path.join(ROOT, "include", header)).read()


def test_geometry_and_layout_need_no_device():
    from gymnasium_robotics_amd import _native

    L = _native.lib()
    R, G = ctypes.c_int(), ctypes.c_int()
    assert L.grx_normstat_geometry(ctypes.byref(R), ctypes.byref(G)) == 0
    assert R.value >= 1 and G.value >= 1
    assert (R.value * G.value + 1) * 65 * 4 <= 64 << 20      # the largest boundary case of the GPU tests, at Fetch's row width
    lay = (ctypes.c_int64 * 8)()
    for od, gd in ((1, 1), (25, 3), (153, 7)):
        D = od + gd
        assert L.grx_normstat_layout(od, gd, lay) == 0
        assert list(lay)[:7] == [0, 8 * D, 16 * D, 16 * D + 8, 16 * D + 16, 20 * D + 16, 24 * D + 16]
        assert lay[7] >= lay[6] + G.value * (2 * D + 1) * 8      # workspace: one partial sum pair per column and one skip count per workgroup
    assert L.grx_normstat_layout(200, 57, lay) == -1 and b"exceeds 256" in L.grx_last_error()
    assert L.grx_normstat_layout(0, 3, lay) == -1
    # argument checks come before any launch
    assert L.grx_normstat_update(None, None, 4, 65, 25, 3, None, 1e-2, None) == -1 and b"null buffer" in L.grx_last_error()
    one = ctypes.c_void_p(16)
    assert L.grx_normstat_update(one, one, 0, 65, 25, 3, None, 1e-2, None) == -1 and b"batch 0" in L.grx_last_error()
    assert L.grx_normstat_update(one, one, 4, 30, 25, 3, None, 1e-2, None) == -1 and b"row_width 30" in L.grx_last_error()
    assert L.grx_normstat_update(one, one, 4, 65, 25, 3, None, 0.0, None) == -1 and b"eps" in L.grx_last_error()
    assert L.grx_normstat_apply_batch(one, one, 4, 64, 25, 3, 4, 5.0, one, None) == -1 and b"row_width 64" in L.grx_last_error()
    assert L.grx_normstat_apply_batch(one, one, 4, 65, 25, 3, 4, -1.0, one, None) == -1 and b"clip" in L.grx_last_error()
    assert L.grx_normstat_apply_packed(one, one, 4, 30, 25, 3, 5.0, one, None) == -1 and b"packed_width 30" in L.grx_last_error()


def test_struct_mirrors_and_state_blob_round_trip():
    from gymnasium_robotics_amd import env_capi as E

    assert ctypes.sizeof(E.NormConfig) == 16 and E.NormConfig.clip.offset == 8
    H = E.NormStateHeader
    assert ctypes.sizeof(H) == 40
    assert [getattr(H, f).offset for f in ("magic", "version", "obs_dim", "goal_dim", "zero0", "eps", "clip", "zero1")] == [0, 8, 12, 16, 20, 24, 32, 36]
    od, gd = 25, 3
    rng = np.random.default_rng(0)
    total, sumsq = rng.standard_normal(od + gd), rng.random(od + gd) * 1e3
    blob = E.pack_norm_state(od, gd, 0.02, 4.5, total, sumsq, 123456789012, 7)
    assert len(blob) == E.norm_state_size(od, gd) == 40 + 16 * 28 + 16
    assert blob[:8] == b"GRXNORM\0" and blob[8:12] == (1).to_bytes(4, "little")
    st = E.parse_norm_state(blob)
    assert (st["obs_dim"], st["goal_dim"], st["eps"], st["clip"], st["count"], st["skipped"]) == (od, gd, 0.02, 4.5, 123456789012, 7)
    np.testing.assert_array_equal(st["sum"], total)
    np.testing.assert_array_equal(st["sumsq"], sumsq)
    assert E.pack_norm_state(od, gd, st["eps"], st["clip"], st["sum"], st["sumsq"], st["count"], st["skipped"]) == blob
    with pytest.raises(ValueError):
        E.parse_norm_state(blob[:-8])
    with pytest.raises(ValueError):
        E.parse_norm_state(b"GRXENVS\0" + blob[8:])


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    from gymnasium_robotics_amd import env_capi as E

    L = E.lib()
    err = lambda: L.grx_env_last_error().decode()
    p = ctypes.c_void_p()
    assert L.grx_norm_create(None, None, ctypes.byref(p)) == -1 and "NULL handle" in err() and not p.value
    assert L.grx_norm_create(None, None, None) == -1 and "out is NULL" in err()
    for cfg, want in ((E.NormConfig(0.0, 5.0), "eps"), (E.NormConfig(-1.0, 5.0), "eps"), (E.NormConfig(1e-2, 0.0), "clip"), (E.NormConfig(1e-2, -5.0), "clip"),
                      (E.NormConfig(float("nan"), 5.0), "eps")):
        assert L.grx_norm_create(None, ctypes.byref(cfg), ctypes.byref(p)) == -1 and want in err(), err()
        assert not p.value
    size = ctypes.c_size_t()
    for rc in (L.grx_norm_destroy(None), L.grx_norm_update(None, None, 4, None, None), L.grx_norm_apply_batch(None, None, 4, None, None),
               L.grx_norm_policy_input(None, None, None), L.grx_norm_dims(None, None, None, None, None),
               L.grx_norm_stats(None, None, None, None, None, None, None, None)):
        assert rc == -1 and "NULL normalizer" in err(), err()
    for rc in (L.grx_norm_state_size(None, ctypes.byref(size)), L.grx_norm_get_state(None, None, 0), L.grx_norm_set_state(None, None, 0)):
        assert rc == -1 and "NULL argument" in err(), err()


def test_python_class_checks_its_arguments_without_a_device():
    from gymnasium_robotics_amd.her import Normalizer

    class Space:
        def __init__(self, n):
            self.shape = (n,)

    class Env:
        device = "cpu"
        packed = np.zeros((4, 33), np.float32)
        single_observation_space = {"desired_goal": Space(3)}
        single_action_space = Space(4)

    with pytest.raises(ValueError, match="positive"):
        Normalizer(Env(), eps=0.0)
    with pytest.raises(ValueError, match="positive"):
        Normalizer(Env(), clip=-1.0)
