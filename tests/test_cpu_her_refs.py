"""The plain HER references of tests/her_refs.py, checked without a GPU before a device is compared with them -- the stream against its published vectors, the draw against a
case worked out by hand and the vectorised draw against the one-sample restatement -- and the case tables of tests/test_gpu_her_refs.py, shown to discriminate: a reference
with one deliberate mistake (the small variants below) gives another answer on them, so a kernel with that mistake would fail there."""
import numpy as np
import pytest

import her_refs as R
import test_gpu_her_refs as G


# ------------------------------------------------------------------------------------------------------------------ the references themselves
def test_splitmix64_published_vectors():
    s, out = np.array([1234567], np.uint64), []
    for _ in range(5):
        s, z = R.splitmix64(s)
        out.append(int(z[0]))
    assert out == [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    s, z = R.splitmix64(np.array([R.M64], np.uint64))      # the state wraps
    assert int(s[0]) == 0x9E3779B97F4A7C14


def test_keep_thresholds():
    assert [float(x) * 2 ** 24 for x in R.keep_thresholds(4)] == [13421772.0, 13421773.0, 13421774.0]      # 0.8 * 2^24 = 13421772.8
    assert [float(x) * 2 ** 24 for x in R.keep_thresholds(7)] == [14680063.0, 14680064.0, 14680065.0]      # 7 / 8, exact
    assert float(R.keep_thresholds(1)[1]) == 0.5 and float(R.keep_thresholds(0)[1]) == 0.0


def test_draw_worked_out_by_hand():
    """Three worlds at t_now = 9 on a ring of T = 3 (oldest row 6).  World 0 was reset in this very step (mark 9) and its finished episode began at row 7: rows 7..8.  World 1
    began at row 4, before the oldest ring row: rows 6..8.  World 2 began at row 9: nothing to sample.  Seed 11, call 0; the outputs of the stream of key 11 * KEY_SEED + b
    after the discarded one, as (world = (z >> 32) * 3 >> 32, z >> 40, (z >> 16) & 0xFFFFFF), were computed with a stand-alone splitmix64 in Python integers:
      b = 0:  world 2 | world 2 | world 1, then r: (., 11423988, 2847139), r2: (., 13767414, .)
              lo = max(4, 6) = 6; u0 = 11423988 / 2^24 = 0.6809: t = 6 + int(0.6809 * 3) = 8; u1 = 0.1697: fut = 8 + 1 + int(0.1697 * 1) = 9;
              u2 = 13767414 / 2^24 >= 13421773 / 2^24 (k_future = 4): the episode's own goal, t_goal = -1
      b = 1:  world 0, then r: (., 12464336, 6644978), r2: (., 3793698, .)
              lo = max(7, 6) = 7 (prev_start: the mark is t_now); u0 = 0.7429: t = 7 + int(0.7429 * 2) = 8; fut = 9 + int(0.396 * 1) = 9; u2 = 0.226 < 0.8: t_goal = 9
      b = 5:  world 2 | world 0, then r: (., 6871233, 1441752), r2: (., 2050595, .)
              lo = 7; u0 = 0.4096: t = 7 + int(0.4096 * 2) = 7; u1 = 0.0859: fut = 7 + 1 + int(0.0859 * 2) = 8; u2 = 0.122 < 0.8: t_goal = 8"""
    start, prev, term = np.array([9, 4, 9], np.int32), np.array([7, 0, 0], np.int32), np.array([9, -1, -1], np.int32)
    s = R.her_key(11, 0, [0])
    assert int(s[0]) == 0xFD3D99EA8FA04B67
    s, z0 = R.splitmix64(s)
    s, z1 = R.splitmix64(s)
    assert int(z0[0]) == 1576578767780291173 and int(z1[0]) == 17584463549910380079 and (int(z1[0]) >> 32) * 3 >> 32 == 2
    t, w, tg, found = R.ref_her_draw(start, prev, term, 3, 9, 3, 4, 11, 0, np.arange(6))
    assert found.all()
    assert (t[0], w[0], tg[0]) == (8, 1, -1) and (t[1], w[1], tg[1]) == (8, 0, 9) and (t[5], w[5], tg[5]) == (7, 0, 8)
    assert R.ref_her_draw(start, prev, term, 3, 9, 3, 0, 11, 0, np.arange(6))[2].tolist() == [-1] * 6      # k_future = 0 keeps every goal
    # without the marks world 0 has nothing to sample either: b = 1 goes on to its second attempt (world 2), third (world 0), fourth (world 1)
    t, w, tg, _ = R.ref_her_draw(start, None, None, 3, 9, 3, 4, 11, 0, np.arange(6))
    assert (w == 1).all() and w.dtype == t.dtype == tg.dtype == np.int32


def test_probe_table_is_the_walk():
    lo = np.array([9, 9, 3, 9, 9, 5, 9, 9])      # t_now = 9: worlds 2 and 5 have a transition
    assert R.her_probe(lo, np.array([0, 1, 2, 3, 4, 5, 6, 7]), 9).tolist() == [2, 2, 5, 5, 5, 2, 2, 2]      # from w + 1, with wrap
    assert R.her_probe(np.full(4, 9), np.array([0, 3]), 9).tolist() == [0, 3]      # no world at all: N steps end where they began


def _sample_of_cases():
    """(marks, N, T, t_now, k, seed, call, samples) over the draw tables: every case of the small world counts, the first and last samples of its batch"""
    for N in (1, 3, 64):
        for T, t_now, k, seed, call, B, track in G.draw_cases(N):
            yield G.marks(G.boundary_state(N, T, t_now), track), N, T, t_now, k, seed, call, sorted({0, B // 2, B - 1})
    for at in G.SPARSE_AT:
        st, N, T, t_now = G.sparse_state(at)
        yield G.marks(st, True), N, T, t_now, 4, 11, 3, [0, 1, 2, 3]


def test_vectorised_draw_is_the_one_sample_restatement():
    n = probed = 0
    for mk, N, T, t_now, k, seed, call, bs in _sample_of_cases():
        t, w, tg, found = R.ref_her_draw(*mk, N, t_now, T, k, seed, call, np.array(bs))
        for i, b in enumerate(bs):
            assert R.ref_her_draw_scalar(*mk, N, t_now, T, k, seed, call, b) == (t[i], w[i], tg[i], found[i]), (N, T, t_now, k, seed, call, b)
            n += 1
        probed += int(R.her_attempts(R.her_lo(*mk, t_now, T), N, t_now, seed, call, np.array(bs))[2].sum())
    assert n > 1500 and probed >= 8


def test_threshold_calls_draw_the_candidates():
    s = G.THRESHOLD_STATE
    for k, by_m in G.THRESHOLD_CALLS.items():
        lo, q, hi = (float(x) * 2 ** 24 for x in R.keep_thresholds(k))
        assert set(by_m) <= {lo, q, hi} and q in by_m
        for m, call in by_m.items():
            u2 = R.ref_her_draw_parts(s["start"], None, None, s["N"], s["t_now"], s["T"], s["seed"], call, np.arange(1))[3]
            assert float(u2[0]) * 2 ** 24 == m


# ------------------------------------------------------------------------------------------------------------------ wrong draws
DRAW_MISTAKES = ["lo_unclamped", "prev_ignored", "probe_too_far", "probe_no_wrap", "future_from_t", "keep_gt"]


def _draw(mk, N, T, t_now, k, seed, call, B, mistake=None):
    """ref_her_draw put together from its steps, with one of them wrong"""
    start, prev, term = mk
    if mistake == "lo_unclamped":      # the episode start is not clamped to the oldest ring row
        lo_w = R.her_lo(start, prev, term, t_now, t_now)
    elif mistake == "prev_ignored":    # a world reset in this very step is not sampled from the episode that has just ended
        lo_w = R.her_lo(start, None, None, t_now, T)
    else:
        lo_w = R.her_lo(start, prev, term, t_now, T)
    s, w, pending = R.her_attempts(lo_w, N, t_now, seed, call, np.arange(B))
    if mistake == "probe_no_wrap":     # the probe stops at the last world
        have = np.nonzero(lo_w < t_now)[0]
        k_ = np.searchsorted(have, w[pending] + 1)
        w[pending] = np.where(k_ < have.size, have[np.minimum(k_, max(have.size - 1, 0))] if have.size else N - 1, N - 1)
    else:                              # probe_too_far: it starts one world too far
        w[pending] = R.her_probe(lo_w, w[pending], t_now, 2 if mistake == "probe_too_far" else 1)
    u0, u1, u2 = R.her_uniforms(s)
    t, fut = R.her_rows_of(lo_w[w], t_now, u0, u1)
    if mistake == "future_from_t":     # the future row is drawn from t, not from t + 1
        fut = np.minimum(t + (u1 * (t_now - t).astype(np.float32)).astype(np.int64), t_now)
    thr = R.keep_thresholds(k)[1]
    keep = (u2 > thr) if mistake == "keep_gt" else (u2 >= thr)
    return t.astype(np.int32), w.astype(np.int32), np.where(keep, -1, fut).astype(np.int32)


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def _draw_tables():
    """name -> list of (marks, N, T, t_now, k, seed, call, B): the draw launches of the GPU file, table by table (the 2^20-sample launches cut to their first 4096 samples)"""
    tables = {}
    for N in G.DRAW_N:
        tables[f"draws N = {N}"] = [(G.marks(G.boundary_state(N, T, t_now), track), N, T, t_now, k, seed, call, B) for T, t_now, k, seed, call, B, track in G.draw_cases(N)]
    tables["sparse"] = []
    for at in G.SPARSE_AT:
        st, N, T, t_now = G.sparse_state(at)
        tables["sparse"] += [(G.marks(st, track), N, T, t_now, 4, 11, 3, 4096) for track in (True, False)]
    st = G.boundary_state(64, 10, 23)
    tables["grid stride"] = [(G.marks(st, True), 64, 10, 23, 4, 11, 0, 4096)]
    tables["fused"] = [(G.marks(G.boundary_state(N, T, t_now), track), N, T, t_now, k, seed, call, B) for N, T, t_now, k, seed, call, B, track, _, _ in G.fused_cases()]
    s = G.THRESHOLD_STATE
    tables["threshold"] = [((s["start"], None, None), s["N"], s["T"], s["t_now"], k, s["seed"], call, 1) for k, by_m in G.THRESHOLD_CALLS.items() for call in by_m.values()]
    return tables


# which mistakes each table must catch.  A sample probes only after 64 attempts on worlds without a transition: that happens in the sparse tables alone (elsewhere at least a
# third of the worlds has one: 2^-37 per sample at the most); u2 equals the threshold only in the launches searched for it.
CAUGHT = {"draws N = 1": ["lo_unclamped"],
          "draws N = 3": ["lo_unclamped", "prev_ignored", "future_from_t"],
          "draws N = 64": ["lo_unclamped", "prev_ignored", "future_from_t"],
          "draws N = 4096": ["lo_unclamped", "prev_ignored", "future_from_t"],
          "sparse": ["probe_no_wrap", "probe_too_far"],
          "grid stride": ["lo_unclamped", "prev_ignored", "future_from_t"],
          "fused": ["lo_unclamped", "prev_ignored", "future_from_t"],
          "threshold": ["keep_gt"]}


assert {m for ms in CAUGHT.values() for m in ms} == set(DRAW_MISTAKES)      # every mistake is caught by some table


@pytest.fixture(scope="module")
def draw_tables():
    return _draw_tables()


@pytest.mark.parametrize("table", list(CAUGHT))
def test_wrong_draws_differ_on_the_tables(draw_tables, table):
    cases = draw_tables[table]
    for mk, N, T, t_now, k, seed, call, B in cases[:12]:      # the put-together draw is the reference where nothing is wrong
        t, w, tg, _ = R.ref_her_draw(*mk, N, t_now, T, k, seed, call, np.arange(B))
        assert not _differs(_draw(mk, N, T, t_now, k, seed, call, B), (t, w, tg))
    for mistake in CAUGHT[table]:
        caught = 0
        for mk, N, T, t_now, k, seed, call, B in cases:
            if _differs(_draw(mk, N, T, t_now, k, seed, call, B, mistake), _draw(mk, N, T, t_now, k, seed, call, B)):
                caught += 1
                if caught >= 3:
                    break
        assert caught >= min(3, len(cases)) or (caught and table in ("sparse", "grid stride", "threshold")), (table, mistake, caught)


def test_a_probe_that_starts_at_the_world_itself_is_the_same_draw():
    """the 64th attempt's world has no transition, so a probe that looks at it once more changes nothing: the mistake worth catching is the probe one world too FAR"""
    st, N, T, t_now = G.sparse_state(0)
    lo_w = R.her_lo(*G.marks(st, True), t_now, T)
    w = np.arange(1, N)
    assert np.array_equal(R.her_probe(lo_w, w, t_now, 0), R.her_probe(lo_w, w, t_now, 1))


# ------------------------------------------------------------------------------------------------------------------ wrong rows
ROW_MISTAKES = ["action_from_t", "ring_mod_T", "terminal_ignored", "stale_mark", "goal_from_desired"]


def _rows(c, data, t, w, tg, term, mistake=None):
    """ref_her_rows with one gather wrong"""
    rows, acts, term_rows = data
    od, gd, ad, N = c["od"], c["gd"], c["ad"], c["N"]
    t, w, tg = (np.asarray(x, np.int64) for x in (t, w, tg))
    Rn = c["T"] if mistake == "ring_mod_T" else c["T"] + 1
    tt = np.full(len(t), -1) if (term is None or mistake == "terminal_ignored") else term.astype(np.int64)[w]
    if mistake == "stale_mark":      # the mark compared as a ring row: an old mark that shares its ring row with t + 1 brings the terminal row in
        is1, isg = (tt >= 0) & ((t + 1) % Rn == tt % Rn), (tt >= 0) & (tg >= 0) & (tg % Rn == tt % Rn)
    else:
        is1, isg = t + 1 == tt, (tg == tt) & (tg >= 0)
    tr = term_rows[w] if term is not None else rows[0, w]
    r0 = rows[t % Rn, w]
    r1 = np.where(is1[:, None], tr, rows[(t + 1) % Rn, w])
    grow = np.where(isg[:, None], tr, rows[np.maximum(tg, 0) % Rn, w])
    goal = np.where((tg < 0)[:, None], r0[:, od + gd:od + 2 * gd], grow[:, od + gd:od + 2 * gd] if mistake == "goal_from_desired" else grow[:, od:od + gd])
    act = acts[(t if mistake == "action_from_t" else t + 1) % Rn, w]
    reward, success, _ = R.ref_her_outcome(r1[:, od:od + gd], goal, c["kind"], c["p0"], c["p1"], c["sparse"], c["ignore_pos"], c["ignore_rot"], c["ignore_z"])
    return np.concatenate([r0[:, :od + gd], goal, act, reward[:, None], r1[:, :od + gd], success[:, None]], axis=1).astype(np.float32)


def _bits_differ(a, b):
    return not np.array_equal(a.view(np.int32), b.view(np.int32))


def test_row_table_enumerates_every_admissible_sample():
    t, w, tg = G.row_indices(True)
    assert len(t) == 5 + 9 + 5 + 9 + 9 and set(w.tolist()) == {0, 1, 2, 3, 4}
    assert ((t == 8) & (w == 2) & (tg == 9)).any() and ((t == 6) & (w == 3)).any() and not ((t == 6) & (w == 2)).any()
    t, w, tg = G.row_indices(False)
    assert set(w.tolist()) == {0, 1, 4} and len(t) == 5 + 9 + 9


def test_wrong_rows_differ_on_every_row_case():
    n = 0
    for n, c in enumerate(G.row_configs()):
        data = G.ring_data(c, n)
        term = G.ROW_MARKS["term"] if c["track"] else None
        t, w, tg = G.row_indices(c["track"])
        want = G.ref_rows(c, data, t, w, tg, term)
        assert not _bits_differ(_rows(c, data, t, w, tg, term), want)
        assert want.shape == (len(t), R.row_columns(c["od"], c["gd"], c["ad"])[2])
        for mistake in ROW_MISTAKES:
            if c["track"] or mistake not in ("terminal_ignored", "stale_mark"):
                assert _bits_differ(_rows(c, data, t, w, tg, term, mistake), want), (mistake, c)
    assert n + 1 == 288


def test_row_cases_have_both_outcomes():
    """the goals of the ring are scaled so that the enumeration sees reached and missed goals of every kind"""
    seen = {}
    for n, c in enumerate(G.row_configs()):
        if c["track"] and c["sparse"]:
            t, w, tg = G.row_indices(True)
            success = G.ref_rows(c, G.ring_data(c, n), t, w, tg, G.ROW_MARKS["term"])[:, -1]
            key = (c["kind"], c["gd"], c["ignore_z"], c["ignore_pos"])
            seen[key] = seen.get(key, set()) | set(success.tolist())
    assert len(seen) == 8 and all(v == {0.0, 1.0} for v in seen.values()), seen


def test_wrong_rows_differ_on_the_fused_and_grid_stride_tables():
    c = G.fused_config(64, 10, G.FUSED_KINDS[0], True)
    st = G.boundary_state(64, 10, 23)
    data = G.ring_data(c, 5)
    t, w, tg, _ = R.ref_her_draw(*G.marks(st, True), 64, 23, 10, 4, 11, 0, np.arange(4096))
    want = G.ref_rows(c, data, t, w, tg, st["term"])
    for mistake in ROW_MISTAKES:
        assert _bits_differ(_rows(c, data, t, w, tg, st["term"], mistake), want), mistake


# ------------------------------------------------------------------------------------------------------------------ the fp32 distance
@pytest.fixture(scope="module")
def pairs():
    return {3: R.threshold_pairs(3), 2: R.threshold_pairs(2)}


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("thr", R.PAIR_THRESHOLDS)
def test_fp32_distance_decides_threshold_pairs_differently(pairs, thr, dim):
    a, b, d = pairs[dim][thr]
    wrong = (d > thr) != (R.distance_fp32(a, b) > np.float32(thr))
    share = wrong.mean()
    print(f"threshold {thr}, {dim}-vectors: an fp32 distance decides {wrong.sum()} of {len(d)} pairs differently ({100 * share:.2f} %); nearest pair {np.abs(d - thr).min():.3e}")
    assert len(d) == 200000 and share >= 0.01 and (d != thr).all()
    an, bn, dn = R.nearest_pairs(a, b, d, thr)      # the table the GPU file runs
    assert len(dn) == 8192 and (dn[:4096] > thr).all() and (dn[4096:] < thr).all()
    assert ((dn > thr) != (R.distance_fp32(an, bn) > np.float32(thr))).sum() >= 82      # 1 % of the table at the least
    for kind in (0, 1, 2):
        if (kind == 2) == (dim == 2):
            _, success, _ = R.ref_her_outcome(an, bn, kind, thr, 0.0, 1)
            assert success[:4096].sum() == 0 and success[4096:].sum() == 4096


def test_outcomes_of_the_euclidean_kinds():
    a, g = np.array([[0, 0, 0], [0, 0, 0]], np.float32), np.array([[0.03, 0.04, 0], [0.03, 0.04, 0.001]], np.float32)
    r, s, d = R.ref_her_outcome(a, g, 0, 0.05, 0.0, 1)
    assert d[0] < 0.05 < d[1]      # float32(0.03), float32(0.04): 0.04999999906 -- the fp64 distance of the fp32 words, not 0.05
    assert np.signbit(r[0]) and r[0] == 0 and r[1] == -1 and s.tolist() == [1, 0]      # -0.0 where the goal is reached
    r, s, _ = R.ref_her_outcome(a[:, :2], g[:, :2], 2, float(d[0]), 0.0, 1)
    assert r.tolist() == [1, 1] and s.tolist() == [1, 1]      # the maze's comparison includes the radius
    r, s, _ = R.ref_her_outcome(a[:1], g[:1], 1, float(d[0]), 0.0, 1)
    assert r[0] == 0 and s[0] == 0      # the hand's does not: d < thr fails at d == thr, and so does d > thr
    r, _, _ = R.ref_her_outcome(a, g, 0, 0.05, 0.0, 0)
    assert r.dtype == np.float32 and np.array_equal(r, (-d).astype(np.float32))
    r, _, _ = R.ref_her_outcome(a[:, :2], g[:, :2], 2, 0.45, 0.0, 0)
    assert np.allclose(r, np.exp(-0.05), rtol=1e-6)
