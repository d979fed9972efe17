"""The device bookkeeping kernels, each called directly and compared with the plain references of tests/bookkeeping_refs.py at the shapes where such kernels break:
grx_order_by_cost_slots and the sort half of grx_fetch_post_step (padding, exactly one key per thread, every register-sort width up to 32 keys per thread, clamped and tied
keys, the boundaries of the slot-aware placement, the moving average), grx_fetch_commit_rows and the commit half of grx_fetch_post_step, grx_maze_episode_end (partly filled
waves and chunks, lists that span chunks, the redraw and its guard), the maze list kernels, and grx_her_append (misaligned ring rows, tails, the list clamps, the terminal-row
scatter).  No environment is built; everything is exact except the moving average, which has a derived bound (bookkeeping_refs.EMA_ULPS)."""
import ctypes

import numpy as np
import pytest

import bookkeeping_refs as R

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel words on either side of a guarded buffer (a multiple of 4: the guarded view keeps the allocation's 16-byte alignment)
SENT_F = -12345.5   # sentinels: a float, an int and a byte no case produces
SENT_I = -77


def _torch():
    import torch

    return torch


def _lib():
    from gymnasium_robotics_amd import _native

    return _native, _native.lib()


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _dev(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return _torch().from_numpy(x).to("cuda:0")


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _guarded(n, dtype, fill):
    """(whole, view): n elements with GUARD sentinel elements before and after"""
    torch = _torch()
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, fill):
    h = whole.cpu()
    return bool((h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all())


# ================================================================================================================== order
ORDER_SIZES = [8, 64, 1048, 2040, 2048, 2056, 4104, 32768, 65536]      # per = 1, 8, 131, 255 / 256 / 257 (padding, one key per thread, the first E = 2), 513 (E = 4), 4096 (16), 8192 (32)
INT32_MAX, INT32_MIN = 2147483647, -2147483648
SPECIAL = [0, -1, INT32_MIN, 250000001, INT32_MAX, 250000000, 0, -7]      # keys 0 (negatives clamp to it) and 4e9 (the clamp; 2.5e8 + 1 rounds to 2.5e8 in float32): ties by world


def _order_launch(entry, cost, ema, alpha, n, slots, order):
    N, L = _lib()
    if entry == "slots":
        N.check(L.grx_order_by_cost_slots(_ptr(cost), _ptr(ema), alpha, n, slots, _ptr(order), _stream()))
    else:
        N.check(L.grx_fetch_post_step(_ptr(cost), _ptr(ema), alpha, n, slots, _ptr(order), None, None, _stream()))


def _cost_patterns(n):
    rng = np.random.default_rng(n)
    per = n // 8
    pats = {"ties": rng.integers(900, 1500, n), "equal": np.full(n, 1234), "ascending": 3 * np.arange(n), "descending": 3 * np.arange(n)[::-1]}
    edge = rng.integers(1, 2000, n)
    edge[(3 * per + np.arange(len(SPECIAL))) % n] = SPECIAL      # the start of slice 3 (tiny slices: spread over the following ones)
    if per >= 16:
        edge[4 * per - 1 - np.arange(len(SPECIAL))] = SPECIAL   # and its end, in the other order: among equal keys the lower world still comes first
    pats["edge"] = edge
    return {k: v.astype(np.int32) for k, v in pats.items()}


@pytest.mark.parametrize("n", ORDER_SIZES)
@pytest.mark.parametrize("entry", ["slots", "post_step"])
def test_order_is_numpy_sorted_order(entry, n):
    """plain order (slots = 0) of every world count at which the sort changes shape, for five cost patterns, against numpy's lexsort"""
    pats = _cost_patterns(n)
    runs = []
    for name, cost in pats.items():
        whole, order = _guarded(n, _torch().int32, SENT_I)
        _order_launch(entry, _dev(cost), None, 0.0, n, 0, order)
        runs.append((name, cost, whole, order))
    _torch().cuda.synchronize()
    for name, cost, whole, order in runs:
        got = _host(order)
        assert sorted(got.tolist()) == list(range(n)), name
        assert np.array_equal(got, R.ref_order(cost, None, n, 0)), name
        assert _guards_intact(whole, n, SENT_I), name


def _straggler_costs(n, K, seed):
    """every slice: cheapest cost 1000, K worlds above twice that, two worlds at exactly twice (not stragglers: the comparison is strict)"""
    rng = np.random.default_rng(seed)
    per = n // 8
    cost = rng.integers(1000, 1400, n)
    for s in range(8):
        p = rng.permutation(per) + s * per
        cost[p[:K]] = rng.integers(2900, 3400, K)
        cost[p[K]] = 1000
        if K + 3 <= per:
            cost[p[K + 1: K + 3]] = 2000
    return cost.astype(np.int32)


# (n, slots, K, the M the placement must use -- 0: the plain order).  M = per - 2 slots + K; active while 0 < slots < per <= 2 slots, M >= 0, 3 M <= per - slots, M <= slots / 4.
PLACEMENT = [
    (4096, 256, 0, 0), (4096, 256, 1, 1), (4096, 256, 64, 64), (4096, 256, 65, 0),      # per = 2 slots: M = K; M = slots / 4 and one more
    (3488, 256, 136, 60), (3488, 256, 137, 0),                                          # per = 436: 3 M = per - slots = 180 at M = 60, one more flips
    (2056, 256, 3, 0), (2056, 256, 255, 0), (2056, 256, 256, 0),                        # per = slots + 1: M < 0, M = 0, M = 1 (3 M > 1)
    (4104, 256, 5, 0),                                                                  # per = 2 slots + 1
    (1048, 100, 79, 10), (1048, 100, 80, 0),                                            # per = 131 on 100 slots (one key per thread, padded): 3 M <= 31
]


@pytest.mark.parametrize("n, slots, K, M", PLACEMENT)
@pytest.mark.parametrize("entry", ["slots", "post_step"])
def test_order_placement_boundaries(entry, n, slots, K, M):
    cost = _straggler_costs(n, K, n + K)
    per = n // 8
    keys = R.order_keys(cost)
    assert all(R.placement_m(keys[s * per:(s + 1) * per], slots) == M for s in range(8))      # the case is the one its row names
    whole, order = _guarded(n, _torch().int32, SENT_I)
    _order_launch(entry, _dev(cost), None, 0.0, n, slots, order)
    _torch().cuda.synchronize()
    want = R.ref_order(cost, None, n, slots)
    assert (M > 0) == (not np.array_equal(want, R.ref_order(cost, None, n, 0)))
    assert np.array_equal(_host(order), want) and _guards_intact(whole, n, SENT_I)


@pytest.mark.parametrize("n", [8, 2040, 2056, 4104])
@pytest.mark.parametrize("alpha", [0.1, 1.0])
@pytest.mark.parametrize("entry", ["slots", "post_step"])
def test_order_moving_average(entry, alpha, n):
    """ema within the derived bound of the fp64 average, the order that of the values written back, nothing written outside the n words of either buffer"""
    torch = _torch()
    rng = np.random.default_rng(n + int(alpha * 10))
    cost = rng.integers(900, 1500, n).astype(np.int32)
    ema0 = rng.uniform(800.0, 1600.0, n).astype(np.float32)
    ema_whole, ema = _guarded(n, torch.float32, SENT_F)
    ema.copy_(_dev(ema0))
    order_whole, order = _guarded(n, torch.int32, SENT_I)
    _order_launch(entry, _dev(cost), ema, alpha, n, 0, order)
    torch.cuda.synchronize()
    got = _host(ema)
    ulps = R.ulps_apart(got, R.ref_ema(cost, ema0, float(np.float32(alpha))))
    print(f"moving average: worst {ulps.max():.3f} float32 ulps from fp64 (bound {R.EMA_ULPS})")
    assert ulps.max() <= R.EMA_ULPS
    assert np.array_equal(_host(order), R.ref_order(cost, got, n, 0))
    assert _guards_intact(ema_whole, n, SENT_F) and _guards_intact(order_whole, n, SENT_I)


# ================================================================================================================== commit
COMMIT_DIMS = [(15, 14, 7, 25), (15, 14, 0, 25), (70, 66, 7, 70)]      # (nq, nv, mocap words, obs): FetchPickAndPlace's, no mocap body, every row wider than a wave
COMMIT_N = 64


def _commit_buffers(dims, seed):
    nq, nv, mw, od = dims
    n, rng = COMMIT_N, np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    widths = dict(qpos=nq, qvel=nv, qacc_ws=nv, mocap=mw, aux=8, goal=3, obs=od, achieved=3)
    live = {f: (r(n, w) if w else None) for f, w in widths.items()}
    live.update(packed=r(n, od + 8), final_packed=r(n, od + 8), status=rng.integers(INT32_MIN, INT32_MAX, n).astype(np.int32))      # sticky halves with every bit, the sign bit too
    staged = {f: (r(n, w) if w else None) for f, w in widths.items()}
    staged["status"] = rng.integers(0, 1 << 20, n).astype(np.int32)      # flags above the four public ones are not reported
    return live, staged


def _commit_run(dims, entry, idx, k, with_final, seed):
    torch = _torch()
    N, L = _lib()
    nq, nv, mw, od = dims
    live, staged = _commit_buffers(dims, seed)
    d_live = {f: (None if v is None else _dev(v)) for f, v in live.items()}
    d_staged = {f: (None if v is None else _dev(v)) for f, v in staged.items()}
    d_idx = _dev(np.asarray(list(idx) + [SENT_I, COMMIT_N + 9], np.int32))      # (entries past k are never read)
    args = N.FetchCommitArgsStruct(_ptr(d_idx), k, nq, nv, mw, od, *[_ptr(d_staged[f]) for f in R.COMMIT_ROWS], _ptr(d_staged["status"]),
                                   *[_ptr(d_live[f]) for f in R.COMMIT_ROWS], _ptr(d_live["packed"]), _ptr(d_live["final_packed"]) if with_final else None, _ptr(d_live["status"]))
    rows = torch.full((k + 2, od + 8), SENT_F, device="cuda:0")
    order = cost = None
    if entry == "rows":
        N.check(L.grx_fetch_commit_rows(ctypes.byref(args), _stream()))
    elif entry == "post_order":      # both halves in one launch: the commit workgroups come behind the eight sorting ones
        cost = np.random.default_rng(seed).integers(900, 1500, COMMIT_N).astype(np.int32)
        order = torch.full((COMMIT_N,), SENT_I, dtype=torch.int32, device="cuda:0")
        N.check(L.grx_fetch_post_step(_ptr(_dev(cost)), None, 0.0, COMMIT_N, 0, _ptr(order), ctypes.byref(args), _ptr(rows), _stream()))
    else:
        N.check(L.grx_fetch_post_step(None, None, 0.0, COMMIT_N, 0, None, ctypes.byref(args), _ptr(rows) if entry == "post_rows" else None, _stream()))
    torch.cuda.synchronize()
    want, want_rows = R.ref_fetch_commit(live, staged, idx, k, od, with_final)
    tag = (dims, entry, list(idx)[:6], k, with_final)
    for f, v in want.items():
        if v is not None:
            assert _same(_host(d_live[f]), v), (f, tag)      # the listed worlds' rows AND every other world's, bit for bit
    got_rows = _host(rows)
    if entry in ("post_rows", "post_order"):
        assert _same(got_rows[:k], want_rows), tag
        assert (got_rows[k:] == SENT_F).all(), tag
    else:
        assert (got_rows == SENT_F).all(), tag
    if order is not None:
        assert np.array_equal(_host(order), R.ref_order(cost, None, COMMIT_N, 0)), tag


@pytest.mark.parametrize("dims", COMMIT_DIMS)
@pytest.mark.parametrize("entry", ["rows", "post", "post_rows", "post_order"])
def test_commit_is_the_numpy_copy(entry, dims):
    n = COMMIT_N
    rng = np.random.default_rng(5)
    seed = 0
    for k in (1, 3, 4, 5, 64):      # the fused launch packs four worlds per workgroup
        lists = [[n - 1], [0]] if k == 1 else [[n - 1, 0] + [int(w) for w in rng.permutation(np.arange(1, n - 1))[:k - 2]]]
        for idx in lists:
            for with_final in (True, False):
                seed += 1
                _commit_run(dims, entry, idx, k, with_final, seed)


# ================================================================================================================== maze episode end
EPISODE_N = [1, 63, 64, 65, 1000, 1024, 1025, 2112, 3001]
ELAPSED = np.array([0, 3, 4, 5, 1 << 33], np.int64)


def _patterns(N, rng):
    w = np.arange(N)
    return {"none": w < 0, "all": w >= 0, "random": rng.random(N) < 0.5, "last": w == N - 1, "lane0": w % 64 == 0, "lane63": w % 64 == 63, "chunk0": w < 1024, "chunk1": w >= 1024}


def _episode_run(state, cfg, opt=True, final_rows=True, tag=None):
    """one launch on copies of `state` against ref_maze_episode_end; opt: the optional outputs (mask, step_success, desired, n_final, final_idx) given or NULL"""
    torch = _torch()
    Nat, L = _lib()
    N = len(state["elapsed"])
    d = {k: (None if v is None else _dev(v)) for k, v in state.items()}
    goal_xy = None if cfg.get("goal_xy") is None else _dev(np.asarray(cfg["goal_xy"], np.float64))
    pd = 0 if state["packed"] is None else state["packed"].shape[1]
    u8 = lambda: torch.full((N,), 0xAB, dtype=torch.uint8, device="cuda:0")
    i32 = lambda n: torch.full((n,), SENT_I, dtype=torch.int32, device="cuda:0")
    idx_whole, idx_view = _guarded(N, torch.int32, SENT_I)      # the two lists lie between sentinel words: a rank that is off by a wave's count lands there
    fin_whole, fin_view = _guarded(N, torch.int32, SENT_I)
    out = dict(terminated=u8(), truncated=u8(), mask=u8() if opt else None, step_success=u8() if opt else None,
               desired=torch.full((N, 2), SENT_F, device="cuda:0") if opt else None, reset_count=i32(1), reset_idx=idx_view, n_final=i32(1) if opt else None,
               final_idx=fin_view if opt else None, final_rows=torch.full((N, pd), SENT_F, device="cuda:0") if (final_rows and pd) else None)
    a = Nat.MazeEpisodeArgsStruct()
    for f in ("elapsed", "needs_reset", "success", "achieved", "goal", "status", "packed", "rng"):
        setattr(a, f, _ptr(d[f]))
    a.goal_xy = _ptr(goal_xy)
    a.n_goal = 0 if goal_xy is None else len(cfg["goal_xy"])
    a.mode, a.limit, a.continuing_task, a.reset_target, a.packed_dim = cfg["mode"], cfg["limit"], cfg["continuing_task"], cfg["reset_target"], pd
    a.noise_range, a.scaling, a.goal_radius = cfg["noise_range"], cfg["scaling"], cfg["goal_radius"]
    for f, t in out.items():
        setattr(a, f, _ptr(t))
    Nat.check(L.grx_maze_episode_end(ctypes.byref(a), N, _stream()))
    torch.cuda.synchronize()
    want = R.ref_maze_episode_end(state, cfg)
    for f in ("elapsed", "needs_reset", "goal", "status"):
        assert _same(_host(d[f]), want[f]), (f, tag)
    for f in ("success", "achieved", "packed"):      # inputs stay
        assert d[f] is None or _same(_host(d[f]), state[f]), (f, tag)
    if state["rng"] is not None:
        got = _host(d["rng"], np.uint64)
        assert R.rng_rows_equal(got, want["rng"]), tag
        same = (want["rng"] == state["rng"]).all(axis=1)      # a world that drew nothing keeps its row word for word
        assert np.array_equal(got[same], state["rng"][same]), tag
    for f in ("terminated", "truncated") + (("mask", "step_success", "desired") if opt else ()):
        assert _same(_host(out[f]), want[f]), (f, tag)
    k = want["reset_count"]
    assert int(out["reset_count"]) == k, tag
    got_idx = _host(out["reset_idx"])
    assert np.array_equal(got_idx[:k], want["reset_idx"]) and (np.diff(got_idx[:k]) > 0).all() and (got_idx[k:] == SENT_I).all(), tag
    assert _guards_intact(idx_whole, N, SENT_I) and _guards_intact(fin_whole, N, SENT_I), tag
    if opt:
        assert int(out["n_final"]) == want["n_final"], tag
        fi, kf = _host(out["final_idx"]), want["n_final"]
        assert np.array_equal(fi[:kf], want["final_idx"]) and (fi[kf:] == SENT_I).all(), tag
    if out["final_rows"] is not None:
        fr = _host(out["final_rows"])
        kf = k if cfg["mode"] == 1 else 0
        assert (kf == 0 or _same(fr[:kf], state["packed"][want["reset_idx"]])) and (fr[kf:] == SENT_F).all(), tag
    return want


def _episode_state(N, mode, cont, limit, P, rng, packed_dim):
    """inputs whose listed set is the pattern P wherever the mode and the flags allow one (mode 0: the pending worlds; mode 1: the worlds that end)"""
    success = (rng.random(N) < 0.5).astype(np.uint8)
    elapsed = ELAPSED[rng.integers(0, len(ELAPSED), N)]
    needs = np.zeros(N, np.uint8)      # (modes 1 and 2 are specified for needs_reset == 0 on entry only)
    if mode == 0:
        needs = P.astype(np.uint8)
    elif mode == 1:
        if limit > 0:      # the time limit ends exactly the worlds of the pattern: elapsed + 1 >= 5 from {4, 5, 2^33}, not from {0, 3}
            elapsed = np.where(P, ELAPSED[rng.integers(2, 5, N)], ELAPSED[rng.integers(0, 2, N)])
            if not cont:
                success = (success & P).astype(np.uint8)
        elif not cont:
            success = P.astype(np.uint8)
    return dict(elapsed=elapsed.astype(np.int64), needs_reset=needs, success=success, achieved=rng.standard_normal((N, 2)).astype(np.float32),
                goal=rng.standard_normal((N, 2)).astype(np.float32), status=rng.integers(INT32_MIN, INT32_MAX, N).astype(np.int32),
                packed=rng.standard_normal((N, packed_dim)).astype(np.float32), rng=None)


@pytest.mark.parametrize("N", EPISODE_N)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_maze_episode_end_is_the_per_world_loop(mode, N):
    rng = np.random.default_rng(100 * N + mode)
    pats = _patterns(N, rng)
    names = list(pats) if mode != 2 else ["none", "random"]
    seen = set()
    for cont in (0, 1):
        for limit in (0, 5):
            cfg = dict(mode=mode, limit=limit, continuing_task=cont, reset_target=0, goal_xy=None, noise_range=0.0, scaling=1.0, goal_radius=0.45)
            for name in names:
                variants = [(True, 7, True)] if name != "random" else [(True, 7, True), (False, 33, True), (True, 33, False)]      # (optional outputs, packed_dim, final_rows)
                for opt, pd, fr in variants:
                    st = _episode_state(N, mode, cont, limit, pats[name], rng, pd)
                    want = _episode_run(st, cfg, opt=opt, final_rows=fr, tag=(N, mode, cont, limit, name, opt, pd, fr))
                    if mode == 0 or (mode == 1 and (limit > 0 or not cont)):      # the listed set IS the pattern
                        assert np.array_equal(want["reset_idx"], np.nonzero(pats[name])[0]), (name, cont, limit)
                    seen.add(want["reset_count"])
    assert mode == 2 or {0, N} <= seen      # both the empty and the full list were produced


def _goal_cells(n_goal, scaling):
    grid = np.array([[1.5, 0.5], [-2.5, 1.5], [0.5, -1.5], [3.5, 2.5], [-0.5, -0.5], [2.5, -2.5], [-3.5, 0.5]], np.float64)
    return grid[:n_goal] * scaling


def _redraw_state(N, mode, cells, scaling, rng, seed):
    on = rng.random(N) < 1.0 / 3.0      # about a third of the worlds stand on their goal
    goal = (cells[rng.integers(0, len(cells), N)] + rng.uniform(-0.25, 0.25, (N, 2)) * scaling).astype(np.float32)
    achieved = np.where(on[:, None], goal + rng.uniform(-0.2, 0.2, (N, 2)).astype(np.float32), goal + np.float32(3.0 * scaling)).astype(np.float32)
    success = on.astype(np.uint8)
    flip = rng.random(N) < 0.1      # a success flag away from the goal (the loop ends at its first test) and a world on its goal without the flag (nothing is drawn)
    success[flip] ^= 1
    gens = [np.random.Generator(np.random.PCG64(seed + w)) for w in range(N)]
    for g in gens[1::2]:
        g.integers(0, 3)      # every other stream starts with a buffered 32-bit half
    rows = np.array([R.rng_row(g) for g in gens], dtype=np.uint64)
    needs = (rng.random(N) < 0.2).astype(np.uint8) if mode == 0 else np.zeros(N, np.uint8)      # a pending world draws nothing
    return dict(elapsed=ELAPSED[rng.integers(0, len(ELAPSED), N)].astype(np.int64), needs_reset=needs, success=success, achieved=achieved, goal=goal,
                status=rng.integers(INT32_MIN, INT32_MAX, N).astype(np.int32), packed=rng.standard_normal((N, 7)).astype(np.float32), rng=rows)


@pytest.mark.parametrize("N, scaling", [(65, 1.0), (1025, 4.0)])
@pytest.mark.parametrize("n_goal", [1, 2, 7])
@pytest.mark.parametrize("mode", [0, 1])
def test_maze_episode_end_redraw_is_numpy(mode, n_goal, N, scaling):
    """MazeEnv.update_goal on the device against a numpy Generator continued from the same row: goal, stream position, buffered half and status bit for bit, also for the worlds
    the time limit ends in the same step (limit 5 with elapsed from {0, 3, 4, 5, 2^33})"""
    rng = np.random.default_rng(7 * N + n_goal + mode)
    cells = _goal_cells(n_goal, scaling)
    st = _redraw_state(N, mode, cells, scaling, rng, 4000 + N)
    cfg = dict(mode=mode, limit=5, continuing_task=1, reset_target=1, goal_xy=cells, noise_range=0.25, scaling=scaling, goal_radius=0.45)
    want = _episode_run(st, cfg, tag=(N, mode, n_goal))
    moved = (want["goal"] != st["goal"]).any(axis=1)
    drew = (want["rng"] != st["rng"]).any(axis=1)
    if n_goal == 1:
        assert not moved.any() and not drew.any()      # one goal cell: nothing is drawn, the rows stay
    else:
        assert moved.sum() > N // 8 and np.array_equal(moved, drew)
        assert mode == 0 or (moved & (want["truncated"] != 0)).any()      # redrawn AND ended in the same step
    assert np.array_equal(want["status"], st["status"])      # nobody reached the guard


@pytest.fixture(scope="module")
def guard_case():
    """65 worlds; worlds 3 and 64 stand within the radius of BOTH goal cells and there is no noise: all 65 536 draws are rejected.  The reference is computed once."""
    N = 65
    rng = np.random.default_rng(65)
    cells = np.array([[0.0, 0.0], [0.1, 0.0]])
    st = _redraw_state(N, 1, cells, 1.0, rng, 9000)
    st["success"][:] = 0
    for w in (3, 64):
        st["success"][w], st["achieved"][w], st["goal"][w] = 1, (0.05, 0.0), (0.02, 0.01)
    st["elapsed"][3], st["elapsed"][64] = 0, 4      # world 64 is also ended by the time limit in this step
    cfg = dict(mode=1, limit=5, continuing_task=1, reset_target=1, goal_xy=cells, noise_range=0.0, scaling=1.0, goal_radius=0.45)
    return st, cfg, R.ref_maze_episode_end(st, cfg)


def test_maze_episode_end_guard_flags_the_world(guard_case, monkeypatch):
    st, cfg, want = guard_case
    monkeypatch.setattr(R, "ref_maze_episode_end", lambda s, c: want)      # (the shared reference: 2 x 65 536 rejected draws are walked once)
    _episode_run(st, cfg, tag="guard")
    for w in (3, 64):
        assert want["status"][w] & 0x10001 == 0x10001 and np.array_equal(want["goal"][w], st["goal"][w]) and not np.array_equal(want["rng"][w], st["rng"][w])
    others = np.setdiff1d(np.arange(65), [3, 64])
    assert np.array_equal(want["status"][others], st["status"][others]) and 64 in want["reset_idx"] and 3 not in want["reset_idx"]


# ================================================================================================================== maze list kernels
def _rng_rows(n, seed):
    gens = [np.random.Generator(np.random.PCG64(seed + w)) for w in range(n)]
    for g in gens[::2]:
        g.integers(0, 3)
    return np.array([R.rng_row(g) for g in gens], dtype=np.uint64)


@pytest.mark.parametrize("N, max_n", [(40, 9), (1100, 1100)])      # 1100: more list entries than the 1024 workgroups of grx_maze_reset_rows_list, which then stride
def test_maze_list_kernels_stop_at_the_device_count(N, max_n):
    """grx_maze_sample_resets_list / grx_maze_reset_rows_list with the list's length in device memory, against grx_maze_sample_resets_device / grx_maze_reset_rows (checked against
    numpy in tests/test_gpu_maze.py) on the first `count` entries; everything at or beyond the count keeps its sentinel"""
    torch = _torch()
    Nat, L = _lib()
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    rng = np.random.default_rng(N)
    rows0 = _rng_rows(N, 70)
    lst = _dev(rng.permutation(N)[:max_n].astype(np.int32))
    goal_xy, reset_xy = _dev(_goal_cells(7, 1.0)), _dev(_goal_cells(5, 1.0)[::-1].copy())
    for count in (0, 1, max_n):
        cnt = _dev(np.array([count], np.int32))
        sa, sb = _dev(rows0), _dev(rows0)
        stage_a, stage_b = torch.full((max_n, 4), SENT_F, device="cuda:0"), torch.full((max_n, 4), SENT_F, device="cuda:0")
        Nat.check(L.grx_maze_sample_resets_list(vp(_ptr(sa)), vp(_ptr(lst)), vp(_ptr(cnt)), ci(max_n), vp(_ptr(goal_xy)), ci(7), vp(_ptr(reset_xy)), ci(5), cd(0.25), cd(1.0),
                                                vp(_ptr(stage_a)), _stream()))
        Nat.check(L.grx_maze_sample_resets_device(_ptr(sb), _ptr(lst), count, _ptr(goal_xy), 7, _ptr(reset_xy), 5, 0.25, 1.0, None, None, _ptr(stage_b), _stream()))
        for nq, nv, skip in ((2, 2, 0), (15, 14, 2)):      # the point mass and the ant
            od = nq + nv - skip
            qpos0 = _dev(rng.standard_normal(nq).astype(np.float32))
            init = dict(qpos=(N, nq), qvel=(N, nv), qacc_ws=(N, nv), goal=(N, 2), obs=(N, od), achieved=(N, 2), reward=(N,), packed=(N, od + 6))
            bufs = [{f: torch.full(s, SENT_F, device="cuda:0") for f, s in init.items()} for _ in range(2)]
            for b in bufs:
                b["success"] = torch.full((N,), 0xAB, dtype=torch.uint8, device="cuda:0")
            desired = torch.full((N, 2), SENT_F, device="cuda:0")
            mk = lambda b, stage: Nat.MazeResetArgsStruct(_ptr(lst), _ptr(stage), _ptr(qpos0), nq, nv, od, skip, 0.45, 0, *[_ptr(b[f]) for f in (
                "qpos", "qvel", "qacc_ws", "goal", "obs", "achieved", "reward", "success", "packed")])
            Nat.check(L.grx_maze_reset_rows_list(ctypes.byref(mk(bufs[0], stage_a)), vp(_ptr(cnt)), ci(max_n), vp(_ptr(desired)), _stream()))
            Nat.check(L.grx_maze_reset_rows(ctypes.byref(mk(bufs[1], stage_b)), count, _stream()))
            torch.cuda.synchronize()
            listed = _host(lst)[:count]
            for f in bufs[0]:
                got = _host(bufs[0][f])
                assert _same(got, _host(bufs[1][f])), (count, nq, f)
                rest = np.setdiff1d(np.arange(N), listed)
                assert (got[rest] == (0xAB if f == "success" else SENT_F)).all(), (count, nq, f)
            des, goal = _host(desired), _host(bufs[0]["goal"])
            assert _same(des[listed], goal[listed]) and (count == 0 or (goal[listed] != SENT_F).all()), (count, nq)
            assert (des[np.setdiff1d(np.arange(N), listed)] == SENT_F).all()
        a, b = _host(stage_a), _host(stage_b)
        assert _same(a, b) and (a[count:] == SENT_F).all() and (count == 0 or (a[:count] != SENT_F).all()), count
        assert np.array_equal(_host(sa, np.uint64), _host(sb, np.uint64)), count
        unlisted = np.setdiff1d(np.arange(N), _host(lst)[:count])
        assert np.array_equal(_host(sa, np.uint64)[unlisted], rows0[unlisted]), count


# ================================================================================================================== HER append
HER_SHAPES = [(8, 33, 4), (3, 7, 2), (5, 33, 3), (1000, 9, 2)]      # (3, 7, 2): rows of 21 and 6 words -- ring rows at every misalignment, aligned ones with a tail of 1 and 2 words
RING = 4


@pytest.mark.parametrize("N, W, A", HER_SHAPES)
@pytest.mark.parametrize("track", [True, False])
def test_her_append_is_the_numpy_copy(track, N, W, A):
    """nine appends into a ring of four rows (it wraps twice) that lies between sentinel words, each with another way of naming the reset worlds"""
    torch = _torch()
    Nat, L = _lib()
    rng = np.random.default_rng(N * W + A)
    ring_whole, ring = _guarded(RING * N * W, torch.float32, SENT_F)
    acts_whole, acts = _guarded(RING * N * A, torch.float32, SENT_F)
    ring.copy_(_dev(rng.standard_normal(RING * N * W).astype(np.float32))); acts.copy_(_dev(rng.standard_normal(RING * N * A).astype(np.float32)))
    h_ring, h_acts = _host(ring).reshape(RING, N, W).copy(), _host(acts).reshape(RING, N, A).copy()
    h = dict(start=np.zeros(N, np.int32), prev=np.full(N, -3, np.int32) if track else None, term=np.full(N, -1, np.int32) if track else None,
             term_rows=rng.standard_normal((N, W)).astype(np.float32))
    d = {k: (None if v is None else _dev(v)) for k, v in h.items()}
    perm = lambda: [int(w) for w in rng.permutation(N)]
    some = perm()[:max(1, N // 2)]
    other = [w for w in range(N) if w not in some] or [0]
    bad = [some[0], -1] + some[1:] + [N + 5]
    plans = [      # (list, host count, device count or None, mask, scatter the terminal rows)
        ([], 0, None, None, False),
        ([N - 1], 1, None, None, True),
        (perm(), N, None, None, True),
        (bad, len(bad), None, None, True),                                  # entries -1 and N + 5 among valid ones: skipped, their row slot writes nowhere
        (perm(), N, -3, None, True),                                        # the device count wins and clamps to 0
        ((some + [-1] * N)[:N] + [other[0]] * 10, 1, N + 10, None, True),   # clamps to N: the ten entries beyond name a world that must stay unmarked
        (None, 0, None, (rng.random(N) < 0.5).astype(np.uint8), False),     # mask source
        ([0, N - 1], 2, 1, None, True),                                     # a device count below the host's
        (None, 0, None, None, False),                                       # neither: no world was reset
    ]
    assert len(plans) == 9
    for step, (lst, count, count_dev, mask, scatter) in enumerate(plans):
        t, r = step + 1, (step + 1) % RING
        src_off = 1 if t in (2, 8) else 0      # t = 8 appends to the aligned ring row 0 from a misaligned source
        packed_whole, act_whole = _dev(rng.standard_normal(N * W + 1).astype(np.float32)), _dev(rng.standard_normal(N * A + 1).astype(np.float32))
        packed, act = packed_whole[src_off:src_off + N * W], act_whole[src_off:src_off + N * A]
        final = rng.standard_normal((len(lst) if lst else 1, W)).astype(np.float32)
        if lst is not None and len(lst) > N:
            final[N:] = final[N]      # (only a launch that ignores the clamp reads these)
        d_final, d_list = _dev(final), _dev(np.asarray(lst if lst else [0], np.int32))
        d_cnt = None if count_dev is None else _dev(np.array([count_dev], np.int32))
        d_mask = None if mask is None else _dev(mask)
        a = Nat.HerAppendArgsStruct()
        a.packed, a.action = _ptr(packed), _ptr(act)
        a.row_dst, a.act_dst = ring.data_ptr() + 4 * r * N * W, acts.data_ptr() + 4 * r * N * A
        a.n_row, a.n_act, a.n_worlds, a.t, a.W = N * W, N * A, N, t, W
        a.start, a.prev_start, a.term_t = _ptr(d["start"]), _ptr(d["prev"]), _ptr(d["term"])
        if lst is not None:
            a.list, a.count, a.count_dev = _ptr(d_list), count, _ptr(d_cnt)
        a.mask = _ptr(d_mask)
        if scatter:
            a.final_rows, a.term_rows = _ptr(d_final), _ptr(d["term_rows"])
        Nat.check(L.grx_her_append(ctypes.byref(a), _stream()))
        torch.cuda.synchronize()
        want = R.ref_her_append(h_ring[r], h_acts[r], _host(packed), _host(act), h["start"], h["prev"], h["term"], t, N, lst=lst,
                                count=count if count_dev is None else count_dev, mask=mask, final_rows=final if scatter else None, term_rows=h["term_rows"] if scatter else None)
        h_ring[r], h_acts[r], h["start"], h["prev"], h["term"] = want["row_dst"], want["act_dst"], want["start"], want["prev_start"], want["term_t"]
        if scatter:
            h["term_rows"] = want["term_rows"]
        assert _same(_host(ring).reshape(RING, N, W), h_ring), step      # the appended row AND the three others
        assert _same(_host(acts).reshape(RING, N, A), h_acts), step
        assert _guards_intact(ring_whole, RING * N * W, SENT_F) and _guards_intact(acts_whole, RING * N * A, SENT_F), step
        for f in ("start", "prev", "term", "term_rows"):
            assert h[f] is None or _same(_host(d[f]), h[f]), (step, f)
    assert h["start"].max() == 8 and (not track or h["term"].max() == 8)
