"""The plain references of the episode store (tests/episode_refs.py), checked without a GPU before a device is compared with them -- the archive against a case worked out
by hand, the vectorised draw against the one-sample restatement -- and the case tables of tests/test_gpu_episode_refs.py, shown to discriminate: a reference with one
deliberate mistake gives another answer on them, so a kernel with that mistake would fail there.  Then the CPU side of the C ABI (include/grx_episodes.h): the exported
symbols, the struct mirrors, the argument refusals that need no device, and a C99 build of the worked example."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import episode_refs as P
import her_refs as R
import test_gpu_episode_refs as G

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPISODES_HEADER = os.path.join(ROOT, "include", "grx_episodes.h")
CALLS = {"create", "destroy", "dims", "sample", "reseed", "store"}


# ------------------------------------------------------------------------------------------------------------------ the references themselves
def test_archive_worked_out_by_hand():
    """T = 3 (four ring rows), t_prev = 9: the ring holds rows 6..9 at ring rows 2, 3, 0, 1.  World 0 began at row 8, world 1 at row 2 (before the oldest row).
    Without terminal rows: world 0 -> rows 8, 9 (L = 1), world 1 -> rows 6..9 (L = 3).  With them the oldest admissible row is 7: world 1 -> rows 7, 8, 9 + the terminal
    row (L = 3), world 0 -> rows 8, 9 + terminal (L = 2)."""
    T, N, W, ad = 3, 2, 2, 1
    ring = np.zeros((4, N, W), np.float32)
    acts = np.zeros((4, N, ad), np.float32)
    for t in range(6, 10):
        ring[t % 4, :, 0], ring[t % 4, :, 1], acts[t % 4, :, 0] = t, [0, 1], 100 + t      # word 0: the absolute row, word 1: the world
    start = np.array([8, 2], np.int32)
    st = P.ref_archive(P.empty_store(3, T, W, ad, fill=-1.0, fill_meta=-1), ring, acts, start, 9, T, np.array([1, 0], np.int32), 2)
    assert st["count"] == 2 and st["meta"].tolist() == [[3, 1, 6, 0], [1, 0, 8, 0], [-1, -1, -1, -1]]
    assert st["rows"][0, :, 0].tolist() == [6, 7, 8, 9] and st["acts"][0, :, 0].tolist() == [0, 107, 108, 109]
    assert st["rows"][1, :, 0].tolist() == [8, 9, -1, -1] and st["acts"][1, :, 0].tolist() == [0, 109, -1, -1] and (st["rows"][2] == -1).all()
    final, step = np.array([[50, 0], [51, 1]], np.float32), np.array([[200], [201]], np.float32)
    st = P.ref_archive(st, ring, acts, start, 9, T, np.array([1, 0], np.int32), 2, final, False, step)      # slots 2 and 0 (wrap)
    assert st["count"] == 4 and st["meta"].tolist() == [[2, 0, 8, 0], [1, 0, 8, 0], [3, 1, 7, 0]]
    assert st["rows"][2, :, 0].tolist() == [7, 8, 9, 51] and st["acts"][2, :, 0].tolist() == [0, 108, 109, 201]
    assert st["rows"][0, :, 0].tolist() == [8, 9, 50, 9] and st["acts"][0, :, 0].tolist() == [0, 109, 200, 109]      # (row 3 of the slot: what the earlier episode left)
    st2 = P.ref_archive(P.empty_store(3, T, W, ad), ring, acts, start, 9, T, np.array([1, 0], np.int32), 2, final[::-1].copy(), True, step)      # compact: row j of position j
    assert st2["rows"][0, 3, 0] == 51 and st2["rows"][1, 2, 0] == 50


def test_archive_table_covers_the_start_kinds():
    """every kind of episode mark is in the table, and the lengths it produces include 0, 1 and T"""
    seen = set()
    for c in G.archive_cases(64):
        want = G.archive_expected(c)
        live = want["meta"][want["meta"][:, 0] != G.SENT_I]
        seen |= set(live[:, 0].tolist())
        assert ((live[:, 0] >= 0) & (live[:, 0] <= c["T"])).all()
    assert {0, 1, 3, 10} <= seen
    starts = G.archive_starts(64, 10, 23, 1)
    assert (starts < 0).any() and (starts == 23 - 10 - 2).any() and (starts == 23 - 10 + 1).any() and (starts == 23).any()


def _draw_cases():
    for name in G.DRAW_STORES + G.EMPTY_STORES:
        lens, count, _ = G.store_lens(name)
        for strategy, k, seed, call, B in G.draw_cases(name):
            yield lens, count, strategy, k, seed, call, sorted({0, B // 2, B - 1})
    for at in G.SPARSE_AT:
        lens, count, _ = G.sparse_lens(at)
        for strategy in G.STRATEGIES:
            yield lens, count, strategy, 4, 11, 3, [0, 1, 2, 3]
    s = G.THRESHOLD_STORE
    for k, by_m in G.THRESHOLD_CALLS.items():
        for call in by_m.values():
            yield s["lens"], s["count"], P.FUTURE, k, s["seed"], call, [0]


def test_vectorised_draw_is_the_one_sample_restatement():
    n = probed = 0
    for lens, count, strategy, k, seed, call, bs in _draw_cases():
        e, t, g, found = P.ref_episode_draw(lens, count, len(lens), strategy, k, seed, call, np.array(bs))
        for i, b in enumerate(bs):
            assert P.ref_episode_draw_scalar(lens, count, len(lens), strategy, k, seed, call, b) == (e[i], t[i], g[i], found[i]), (count, strategy, k, seed, call, b)
            n += 1
        F = min(count, len(lens))
        if F and (lens[:F] > 0).any():
            probed += int(P.episode_attempts(lens.astype(np.int64), F, seed, call, np.array(bs))[2].sum())
    assert n > 1200 and probed >= 8      # seven stores x 72 launches x up to three samples, the sparse stores, the threshold calls


def test_draws_stay_inside_the_episode():
    lens, count, T = G.store_lens("beyond")
    for strategy in G.STRATEGIES:
        e, t, g, found = P.ref_episode_draw(lens, count, len(lens), strategy, 7, 11, 0, np.arange(4096))
        L = lens[e]
        assert found.all() and (L > 0).all() and (t >= 0).all() and (t < L).all() and ((g == -1) | ((g >= 0) & (g <= L))).all()
        sub = g >= 0
        assert 0.8 < sub.mean() < 0.95      # 7 / 8 of the goals are substituted
        if strategy == P.FUTURE:
            assert (g[sub] > t[sub]).all()
        if strategy == P.FINAL:
            assert (g[sub] == L[sub]).all()
        if strategy == P.EPISODE:
            assert (g[sub] == 0).any() and (g[sub] <= t[sub]).any()
    assert (P.ref_episode_draw(lens, count, len(lens), P.FUTURE, 0, 11, 0, np.arange(64))[2] == -1).all()      # k_future = 0 keeps every goal


def test_threshold_calls_draw_the_boundary():
    s = G.THRESHOLD_STORE
    for k, by_m in G.THRESHOLD_CALLS.items():
        boundary = -(-(k << 24) // (k + 1))
        assert set(by_m) == {boundary - 1, boundary}
        for m, call in by_m.items():
            state = R.splitmix64(R.splitmix64(P.episode_key(s["seed"], call, [0]))[0])[0]      # past the discarded output and the one attempt
            assert int(P.episode_uniforms(state)[2][0]) == m
            g = P.ref_episode_draw(s["lens"], s["count"], 1, P.FUTURE, k, s["seed"], call, np.arange(1))[2][0]
            assert g == (-1 if m == boundary else 1)


# ------------------------------------------------------------------------------------------------------------------ wrong archives
def _archive(c, mistake=None):
    """archive_expected with one step wrong"""
    st = G.archive_store(c)
    for call in range(2 if c["twice"] else 1):
        rows, acts, start, lst, k, final, compact, step_action = G.archive_inputs(c, call)
        T, t_prev = c["T"], c["t_prev"]
        if mistake == "after_overwrite":      # taken after the append: ring row (t_prev + 1) % (T + 1) already holds this step's row
            rows, acts = rows.copy(), acts.copy()
            rows[(t_prev + 1) % (T + 1)], acts[(t_prev + 1) % (T + 1)] = 77.0, 77.0
        if mistake == "a0_without_s" and final is not None:      # the oldest admissible row without the + s: one row too many for the slot
            Rn, N, E = T + 1, rows.shape[1], len(st["meta"])
            before = st["count"]
            for j in range(min(max(k, 0), N)):
                w, slot = int(lst[j]), (before + j) % E
                if not 0 <= w < N:
                    st["meta"][slot] = (0, w, 0, 0)
                    continue
                a0 = max(int(start[w]), t_prev - T, 0)
                L = t_prev - a0 + 1
                st["meta"][slot] = (L, w, a0, 0)
                n = min(t_prev - a0 + 1, Rn)
                ring = (a0 + np.arange(n)) % Rn
                st["rows"][slot, :n] = rows[ring, w]
                st["acts"][slot, 0] = 0.0
                st["acts"][slot, 1:n] = acts[ring[1:], w]
                if L <= T:
                    st["rows"][slot, L], st["acts"][slot, L] = final[j if compact else w], step_action[w]
            st["count"] = before + min(max(k, 0), N)
            continue
        P.ref_archive(st, rows, acts, start, t_prev, T, lst, k, final, compact, step_action)
    return st


def _stores_differ(a, b):
    return a["count"] != b["count"] or not np.array_equal(a["meta"], b["meta"]) or not G._same(a["rows"], b["rows"]) or not G._same(a["acts"], b["acts"])


@pytest.mark.parametrize("mistake", ["after_overwrite", "a0_without_s"])
@pytest.mark.parametrize("N", G.ARCH_N)
def test_wrong_archives_differ_on_the_table(N, mistake):
    caught = 0
    for c in G.archive_cases(N):
        want = G.archive_expected(c)
        assert not _stores_differ(_archive(c), want)
        caught += _stores_differ(_archive(c, mistake), want)
    assert caught >= 3, (N, mistake, caught)


# ------------------------------------------------------------------------------------------------------------------ wrong draws
DRAW_MISTAKES = ["final_minus_one", "episode_over_L", "probe_modulo_E", "keep_fp32"]


def _draw(lens, count, strategy, k, seed, call, B, mistake=None):
    """ref_episode_draw put together from its steps, with one of them wrong"""
    lens = np.asarray(lens, np.int64)
    E = len(lens)
    F = min(max(count, 0), E)
    if F == 0 or not (lens[:F] > 0).any():
        return np.zeros(B, np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int32)
    s, e, pending = P.episode_attempts(lens, F, seed, call, np.arange(B))
    e[pending] = P.episode_probe(lens, e[pending], F, E if mistake == "probe_modulo_E" else None)
    u0, u1, m2 = P.episode_uniforms(s)
    L = np.maximum(lens[e], 1)      # (a wrong probe may end on an empty slot)
    t, g = P.episode_rows_of(L, u0, u1, strategy)
    if mistake == "final_minus_one" and strategy == P.FINAL:
        g = L - 1
    if mistake == "episode_over_L" and strategy == P.EPISODE:
        g = np.minimum((u1 * L.astype(np.float32)).astype(np.int64), L)
    if mistake == "keep_fp32":      # u2 >= (float)k / ((float)k + 1.0f) with a quotient that is not correctly rounded (one ulp low: her_refs.keep_thresholds)
        keep = m2.astype(np.float32) * np.float32(2.0 ** -24) >= R.keep_thresholds(k)[0]
    else:
        keep = P.episode_keep(m2, k)
    return e.astype(np.int32), t.astype(np.int32), np.where(keep, -1, g).astype(np.int32)


def _draw_tables():
    tables = {}
    for name in G.DRAW_STORES:
        lens, count, _ = G.store_lens(name)
        tables[name] = [(lens, count, *case) for case in G.draw_cases(name)]
    tables["sparse"] = [(G.sparse_lens(at)[0], G.sparse_lens(at)[1], strategy, 4, 11, 3, 4096) for at in G.SPARSE_AT for strategy in G.STRATEGIES]
    lens, count, _ = G.store_lens("beyond")
    tables["grid stride"] = [(lens, count, P.FUTURE, 4, 11, 1 << 40, 4096)]
    s = G.THRESHOLD_STORE
    tables["threshold"] = [(s["lens"], s["count"], strategy, k, s["seed"], call, 1) for k, by_m in G.THRESHOLD_CALLS.items() for call in by_m.values() for strategy in G.STRATEGIES]
    lens, count = G.row_lens()
    tables["rows"] = [(lens, count, strategy, k, 11, n, G.ROW_B) for n, (_, strategy, k) in enumerate(G.row_configs())]
    return tables


# which mistakes each table must catch.  The probe runs only after 64 attempts on empty slots, and passes F only where the count lies below the number of slots: the
# store "below" has stale lengths beyond F but most of its live slots are filled, so it is the sparse store -- and the empty one below F, see the test after this one --
# that walks the probe; r2 >> 40 sits at the boundary only in the launches searched for it.
CAUGHT = {"below": ["final_minus_one", "episode_over_L"], "equal": ["final_minus_one", "episode_over_L"], "beyond": ["final_minus_one", "episode_over_L"],
          "T1": ["final_minus_one", "episode_over_L"], "rows": ["final_minus_one", "episode_over_L"], "threshold": ["keep_fp32"]}


@pytest.fixture(scope="module")
def draw_tables():
    return _draw_tables()


@pytest.mark.parametrize("table", list(CAUGHT) + ["sparse", "grid stride"])
def test_wrong_draws_differ_on_the_tables(draw_tables, table):
    cases = draw_tables[table]
    for lens, count, strategy, k, seed, call, B in cases[:12]:      # the put-together draw is the reference where nothing is wrong
        e, t, g, _ = P.ref_episode_draw(lens, count, len(lens), strategy, k, seed, call, np.arange(B))
        assert all(np.array_equal(x, y) for x, y in zip(_draw(lens, count, strategy, k, seed, call, B), (e, t, g)))
    for mistake in CAUGHT.get(table, []):
        caught = 0
        for lens, count, strategy, k, seed, call, B in cases:
            a, b = _draw(lens, count, strategy, k, seed, call, B, mistake), _draw(lens, count, strategy, k, seed, call, B)
            caught += any(not np.array_equal(x, y) for x, y in zip(a, b))
        assert caught >= (2 if table == "threshold" else 3), (table, mistake, caught)


def test_a_probe_modulo_the_slot_count_is_caught_where_the_live_slots_are_empty():
    """"all_empty_below": count 4 of 8 slots, the four live slots empty, filled (stale) slots behind them.  The probe modulo F finds nothing -- valid = 0, a zero batch --
    and a probe modulo E walks on into the stale slots and samples them."""
    lens, count, _ = G.store_lens("all_empty_below")
    assert not P.ref_episode_draw(lens, count, len(lens), P.FUTURE, 4, 11, 0, np.arange(33))[3].any()
    wrong = P.episode_probe(lens.astype(np.int64), np.array([0, 1, 2, 3]), 4, len(lens))
    assert (lens[wrong] > 0).all() and (wrong >= 4).all()
    right = P.episode_probe(lens.astype(np.int64), np.array([0, 1, 2, 3]), 4)
    assert (lens[right] == 0).all() and (right < 4).all()
    # and in a sparse store whose one episode lies at slot 0, a probe that wraps at E instead of F passes slot F .. E - 1 first
    lens = np.zeros(128, np.int64)
    lens[0], lens[100] = 7, 5
    assert P.episode_probe(lens, np.array([50]), 64).tolist() == [0] and P.episode_probe(lens, np.array([50]), 64, 128).tolist() == [100]


# ------------------------------------------------------------------------------------------------------------------ wrong rows
def test_rows_take_the_action_and_the_goal_from_the_right_rows():
    lens, count = G.row_lens()
    for n, (c, strategy, k) in enumerate(G.row_configs()):
        data = G.store_data(c, G.ROW_E, G.ROW_T, n)
        want, (e, t, g, found) = G.expected_rows(c, data, lens, count, strategy, k, 11, n, G.ROW_B)
        od, gd, ad = c["od"], c["gd"], c["ad"]
        assert want.shape == (G.ROW_B, R.row_columns(od, gd, ad)[2]) and found.all()
        e64, t64 = e.astype(np.int64), t.astype(np.int64)
        assert G._same(want[:, od + 2 * gd:od + 2 * gd + ad], data[1][e64, t64 + 1])      # the action that led to row t + 1 ...
        assert not G._same(want[:, od + 2 * gd:od + 2 * gd + ad], data[1][e64, t64])      # ... not the one that led to row t
        sub = g >= 0
        assert sub.any() and (~sub).any()
        assert G._same(want[sub, od + gd:od + 2 * gd], data[0][e64[sub], g[sub].astype(np.int64), od:od + gd])
        assert G._same(want[~sub, od + gd:od + 2 * gd], data[0][e64[~sub], t64[~sub], od + gd:od + 2 * gd])


# ------------------------------------------------------------------------------------------------------------------ the C ABI without a device
def _E():
    from gymnasium_robotics_amd import env_capi

    return env_capi


def test_every_declared_episodes_entry_point_is_exported():
    E = _E()
    E.lib()
    names = set(re.findall(r"\b(grx_episodes_\w+)\s*\(", open(EPISODES_HEADER).read())) - {"grx_episodes_config", "grx_episodes_batch"}
    assert names == {"grx_episodes_" + c for c in CALLS}, names
    raw = ctypes.CDLL(E.LIB_PATH)
    missing = [n for n in sorted(names) if not hasattr(raw, n)]
    assert not missing, missing
    assert '#include "grx_replay.h"' in open(EPISODES_HEADER).read()
    for header in ("grx_env.h", "grx_replay.h"):      # nothing was added to the two existing headers
        assert "grx_episodes" not in open(os.path.join(ROOT, "include", header)).read()


def test_kernel_entry_points_are_exported():
    from gymnasium_robotics_amd import _native

    L = _native.lib()
    assert {"grx_her_archive", "grx_her_episode_sample"} <= set(_native.EXPORTED_SYMBOLS)
    assert hasattr(L, "grx_her_archive") and hasattr(L, "grx_her_episode_sample")


def test_struct_mirrors_match_the_header_layout():
    from gymnasium_robotics_amd import _native

    E = _E()
    assert ctypes.sizeof(E.EpisodesConfig) == 24 and E.EpisodesConfig.max_batch.offset == 8 and E.EpisodesConfig.seed.offset == 16
    assert ctypes.sizeof(E.EpisodesBatch) == 24 and E.EpisodesBatch.batch.offset == 8 and E.EpisodesBatch.valid.offset == 16
    assert E.EPISODES_STRATEGY == {"future": 0, "final": 1, "episode": 2}
    A = _native.HerArchiveArgsStruct      # five pointers, seven ints (+ 4 bytes of padding), six pointers, one 64-bit count
    assert ctypes.sizeof(A) == 5 * 8 + 7 * 4 + 4 + 6 * 8 + 8 and A.count.offset == 40 and A.final_rows.offset == 72 and A.episodes.offset == 120


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    E = _E()
    L = E.lib()
    err = lambda: L.grx_env_last_error().decode()
    p = ctypes.c_void_p()
    good = E.EpisodesConfig(episodes=1024, max_batch=256, seed=0)
    assert L.grx_episodes_create(None, ctypes.byref(good), ctypes.byref(p)) == -1 and "NULL replay" in err() and not p.value
    assert L.grx_episodes_create(None, ctypes.byref(good), None) == -1 and "out is NULL" in err()
    assert L.grx_episodes_create(None, None, ctypes.byref(p)) == -1 and "NULL config" in err()
    for field, value, want in (("max_batch", 0, "max_batch 0"), ("max_batch", -2, "max_batch -2"), ("episodes", 1 << 31, "episodes 2147483648")):
        cfg = E.EpisodesConfig(episodes=1024, max_batch=256, seed=0)
        setattr(cfg, field, value)
        assert L.grx_episodes_create(None, ctypes.byref(cfg), ctypes.byref(p)) == -1 and want in err(), (field, err())
        assert not p.value
    batch = E.EpisodesBatch()
    for rc in (L.grx_episodes_destroy(None), L.grx_episodes_sample(None, 4, 4, 0, ctypes.byref(batch), None), L.grx_episodes_reseed(None, 1),
               L.grx_episodes_dims(None, None, None, None, None), L.grx_episodes_store(None, None, None, None, None, None)):
        assert rc == -1 and "NULL store" in err(), err()


def test_python_class_refuses_too_few_slots_without_a_device():
    from gymnasium_robotics_amd.her import EpisodicHerReplay

    class Env:
        num_envs = 8

    with pytest.raises(ValueError, match="less than the number of worlds"):
        EpisodicHerReplay(Env(), horizon=5, capacity=64, episodes=7)


def example_build_line(exe):
    E = _E()
    libdir = os.path.dirname(E.LIB_PATH)
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    return [cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
            os.path.join(ROOT, "tests", "capi", "episodes_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}",
            "-o", str(exe)]


def test_episodes_example_builds_as_c99(tmp_path):
    _E().lib()
    exe = tmp_path / "episodes_rollout"
    subprocess.check_call(example_build_line(exe))
    assert exe.exists()
