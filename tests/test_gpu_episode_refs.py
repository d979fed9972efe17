"""The episode store's two entry points (include/grx_capi.h: grx_her_archive, grx_her_episode_sample), called directly and compared with the plain references of
tests/episode_refs.py.  No environment is built.  The archive is compared word for word (bit patterns) over the WHOLE store, which is pre-filled with sentinels: a slot or a
row the call must not touch keeps them.  Sampled rows are the reference rows of the reference draws: copied words, sparse rewards and success flags bit for bit, dense
rewards and the pose goals of kind 3 within the bounds of tests/her_refs.py.  Every device buffer lies between sentinel words.

The case tables at the top are plain numpy (torch is imported inside the tests only): tests/test_cpu_episode_refs.py imports them and shows that references with one
deliberate mistake each give other answers on them."""
import ctypes

import numpy as np
import pytest

import episode_refs as P
import her_refs as R
import test_gpu_her_refs as G

pytestmark = pytest.mark.gpu

GUARD, SENT_I, SENT_F = G.GUARD, G.SENT_I, G.SENT_F

# ================================================================================================================== archive case tables (numpy only)
ARCH_N = [1, 3, 64]
ARCH_T = [(1, 0), (1, 1), (3, 2), (3, 3), (3, 9), (10, 23)]      # (T, t_prev): ring not full, just full, wrapped, an episode that spans the wrap point
ARCH_PAD = [0, 2, 5]                                            # W = od + 2 gd + pad with od = gd = 3: 9, 11, 14 words
ARCH_AD = [1, 4, 5]
ARCH_FINAL = [None, "compact", "world"]
ARCH_OD = ARCH_GD = 3


def archive_starts(N, T, t_prev, s):
    """episode marks that mix among the worlds: 0 negative, 1 below t_prev - T (clipped), 2 exactly t_prev - T + s, 3 inside the ring, 4 equal to t_prev (L = 0 without
    terminal rows, L = 1 with them)"""
    rng = np.random.default_rng(1000 * N + 10 * T + t_prev)
    kinds = {1: [(T + t_prev) % 5], 3: [2, 4, (T + t_prev) % 2]}.get(N)
    kinds = np.array(kinds) if kinds else rng.permutation(np.arange(N) % 5)
    lo = max(t_prev - T + s, 0)
    start = rng.integers(lo, t_prev + 1, N)
    start = np.where(kinds == 0, -3, start)
    start = np.where(kinds == 1, t_prev - T - 2, start)
    start = np.where(kinds == 2, t_prev - T + s, start)
    start = np.where(kinds == 4, t_prev, start)
    return start.astype(np.int32)


def archive_cases(N):
    """one dict per launch: every (T, t_prev) x terminal rows (none, compact, world-indexed) x k in {0, 1, N} x the count on the host or on the device, the row and action
    widths taken in turn; then the special lists"""
    i = 0
    for T, t_prev in ARCH_T:
        for final in ARCH_FINAL:
            for k in sorted({0, 1, N}):
                for count_dev in (False, True):
                    yield dict(N=N, T=T, t_prev=t_prev, final=final, k=k, count_dev=count_dev, pad=ARCH_PAD[i % 3], ad=ARCH_AD[(i // 3) % 3], E=N + 5, before=(i % 4) * 3,
                               bad=None, over=False, twice=False)
                    i += 1
        for final in ARCH_FINAL:
            base = dict(N=N, T=T, t_prev=t_prev, final=final, k=N, count_dev=True, pad=ARCH_PAD[i % 3], ad=ARCH_AD[i % 3], E=N + 5, before=2, bad=None, over=False, twice=False)
            yield dict(base, over=True)                                # *count_dev = N + 9: clamped to N
            yield dict(base, bad=(-1, N), count_dev=bool(i % 2))       # entries that are no world: slot taken, len 0, nothing copied
            yield dict(base, E=N, before=N - 1, count_dev=False)       # slot assignment wraps
            yield dict(base, twice=True, E=N + 1, before=N - 1)        # two consecutive calls: the second sees the advanced count (and wraps)
            i += 1


def archive_inputs(c, call=0):
    """(ring rows, ring acts, start, list, k, final rows or None, compact, step actions or None) of the launch, float32 / int32"""
    N, T, t_prev, ad = c["N"], c["T"], c["t_prev"], c["ad"]
    W = ARCH_OD + 2 * ARCH_GD + c["pad"]
    s = 0 if c["final"] is None else 1
    rng = np.random.default_rng(7 * N + 100 * T + t_prev + 31 * call + (0 if c["final"] is None else len(c["final"])))
    rows, acts = rng.standard_normal((T + 1, N, W)).astype(np.float32), rng.standard_normal((T + 1, N, ad)).astype(np.float32)
    start = archive_starts(N, T, t_prev, s)
    lst = rng.permutation(N).astype(np.int32)      # list order is not world order
    if c["bad"] is not None:
        lst[0] = c["bad"][0]
        lst[-1] = c["bad"][1]      # (N = 1: the one entry is N)
    k = c["k"]
    final = step_action = None
    if s:
        final = rng.standard_normal((N, W)).astype(np.float32)      # compact: row j belongs to list position j; world: row w to world w
        step_action = rng.standard_normal((N, ad)).astype(np.float32)
    return rows, acts, start, lst, k, final, c["final"] == "compact", step_action


def archive_store(c):
    W = ARCH_OD + 2 * ARCH_GD + c["pad"]
    st = P.empty_store(c["E"], c["T"], W, c["ad"], fill=SENT_F, fill_meta=SENT_I)
    st["count"] = c["before"]
    return st


def archive_expected(c):
    """the store after the launch(es) of case c, by ref_archive"""
    st = archive_store(c)
    for call in range(2 if c["twice"] else 1):
        rows, acts, start, lst, k, final, compact, step_action = archive_inputs(c, call)
        P.ref_archive(st, rows, acts, start, c["t_prev"], c["T"], lst, k, final, compact, step_action)
    return st


# ================================================================================================================== sampling case tables (numpy only)
SAMPLE_K = [0, 1, 4, 7]
SAMPLE_SEEDS = [0, 11, (1 << 64) - 1]
SAMPLE_CALLS = [0, 1 << 40]
SAMPLE_B = [1, 31, 32, 33]
SAMPLE_BIG_B = 4096 * 32 + 33      # more than 4096 chunks of 32 samples: the grid-stride pass
STRATEGIES = [P.FUTURE, P.FINAL, P.EPISODE]
SMALL = dict(od=1, gd=2, ad=1, W=5, kind=2, p0=0.45, p1=0.0, sparse=1, ignore_pos=0, ignore_rot=0, ignore_z=0)      # OW = 11 words


def store_lens(name):
    """(lens [E], count, T): slots beyond min(count, E) hold stale positive lengths, which no draw may reach"""
    rng = np.random.default_rng(len(name))
    if name in ("below", "equal", "beyond"):
        E, T = 64, 10
        lens = rng.integers(0, T + 1, E)
        lens[[3, 9]], lens[[4, 11]], lens[[0, 20]] = 1, T, 0      # L = 1, L = T and empty slots among them
        return lens.astype(np.int32), {"below": 40, "equal": 64, "beyond": 64 + 17}[name], T
    if name == "T1":
        return np.array([1, 0, 1, 1, 0, 1, 1], np.int32), 6, 1
    if name == "none_archived":      # F = 0
        return np.full(8, 3, np.int32), 0, 3
    if name == "all_empty":
        return np.zeros(8, np.int32), 8, 3
    if name == "all_empty_below":    # the filled slots lie beyond F
        return np.array([0, 0, 0, 0, 2, 3, 1, 2], np.int32), 4, 3
    raise KeyError(name)


DRAW_STORES = ["below", "equal", "beyond", "T1"]
EMPTY_STORES = ["none_archived", "all_empty", "all_empty_below"]
SPARSE_AT = [0, 4095, "every 64th"]


def sparse_lens(at):
    """4096 slots of which exactly one holds an episode (64 uniform attempts miss it with probability 0.984: nearly every sample ends in the probe), or every 64th"""
    lens = np.zeros(4096, np.int32)
    lens[slice(5, None, 64) if at == "every 64th" else at] = 7
    return lens, 4096, 10


def draw_cases(name):
    """(strategy, k_future, seed, call, B) over one store: every combination, the batch sizes taken in turn"""
    i = 0
    for strategy in STRATEGIES:
        for k in SAMPLE_K:
            for seed in SAMPLE_SEEDS:
                for call in SAMPLE_CALLS:
                    yield strategy, k, seed, call, SAMPLE_B[i % 4]
                    i += 1


def store_data(c, E, T, seed):
    """(ep_rows [E, T+1, W], ep_acts [E, T+1, ad]) float32: the ring recipe of the HER row tests, one world per slot (goals on both sides of the threshold)"""
    rows, acts, _ = G.ring_data(dict(c, T=T, N=E), seed)
    return np.ascontiguousarray(rows.transpose(1, 0, 2)), np.ascontiguousarray(acts.transpose(1, 0, 2))


# calls whose sample 0 (one slot, seed 11) draws r2 >> 40 EXACTLY at the keep boundary ceil(k 2^24 / (k + 1)) and one step below it: {k_future: {r2 >> 40: call}}, found by
# a search over calls on the CPU.  At the boundary the episode's own goal is kept, one below it is not.  (An fp32 quotient that rounds 4 / 5 down puts its boundary at
# 13421772; one that gives 7 / 8 one ulp low puts it at 14680063.)
THRESHOLD_CALLS = {1: {8388607: 10743561, 8388608: 26792449},
                   4: {13421772: 31434115, 13421773: 818480},
                   7: {14680063: 16066714, 14680064: 16548307}}
THRESHOLD_STORE = dict(lens=np.array([1], np.int32), count=1, T=1, seed=11)

ROW_KINDS, ROW_DIMS, ROW_PAD = G.ROW_KINDS, G.ROW_DIMS, G.ROW_PAD
ROW_E, ROW_T, ROW_B = 16, 3, 257


def row_configs():
    """every reward kind and goal width x (obs_dim, act_dim) x sparse / dense; the padding, the strategy and k_future taken in turn"""
    i = 0
    for kc in ROW_KINDS:
        for od, ad in ROW_DIMS:
            for sparse in (1, 0):
                c = dict(p1=0.0, ignore_pos=0, ignore_rot=0, ignore_z=0)
                c.update(kc, od=od, ad=ad, W=od + 2 * kc["gd"] + ROW_PAD[i % 3], sparse=sparse)
                yield c, STRATEGIES[i % 3], SAMPLE_K[1 + i % 3]
                i += 1


def row_lens():
    lens = np.array([3, 1, 0, 2, 3, 3, 1, 2, 0, 3, 2, 1, 3, 3, 2, 1], np.int32)
    return lens, 21      # count beyond E: every slot is live


def expected_rows(c, data, lens, count, strategy, k, seed, call, B):
    """(rows [B, OW], (e, t, g, found)) of one launch by the references"""
    e, t, g, found = P.ref_episode_draw(lens, count, len(lens), strategy, k, seed, call, np.arange(B))
    return P.ref_episode_rows(data[0], data[1], c["od"], c["gd"], c["ad"], e, t, g, c["kind"], c["p0"], c["p1"], c["sparse"], c["ignore_pos"], c["ignore_rot"], c["ignore_z"],
                              found), (e, t, g, found)


# ================================================================================================================== device helpers
_torch, _lib, _stream, _dev, _ptr, _same = G._torch, G._lib, G._stream, G._dev, G._ptr, G._same
Worst = G.Worst


def _guarded_upload(arrays, fill):
    """(whole, views): the host arrays (one dtype) in one device allocation, GUARD sentinel elements before, between and after them"""
    torch = _torch()
    arrays = [np.ascontiguousarray(a).ravel() for a in arrays]
    host = np.full(sum(a.size for a in arrays) + GUARD * (len(arrays) + 1), fill, arrays[0].dtype)
    o, spans = GUARD, []
    for a in arrays:
        host[o:o + a.size] = a
        spans.append((o, a.size))
        o += a.size + GUARD
    whole = torch.from_numpy(host).to("cuda:0")
    return whole, [whole[o:o + n] for o, n in spans]


def _guarded_read(whole, sizes, fill):
    return G._split_guarded(whole, sizes, fill)


def _archive_launch(c):
    """the launch(es) of one archive case; everything needed to check it after the synchronisation"""
    torch = _torch()
    Nat, L = _lib()
    st = archive_store(c)
    W = st["rows"].shape[2]
    fw, (ep_rows, ep_acts) = _guarded_upload([st["rows"], st["acts"]], SENT_F)
    mw, (ep_meta,) = _guarded_upload([st["meta"]], SENT_I)
    cw, (ep_count,) = _guarded_upload([np.array([st["count"]], np.int64)], np.int64(SENT_I))
    keep = []
    for call in range(2 if c["twice"] else 1):
        rows, acts, start, lst, k, final, compact, step_action = archive_inputs(c, call)
        floats = [rows, acts] + ([final, step_action] if final is not None else [])
        iw, fv = _guarded_upload(floats, SENT_F)
        kd = np.array([c["N"] + 9 if c["over"] else k], np.int32)
        jw, (d_start, d_list, d_count) = _guarded_upload([start, lst, kd], SENT_I)
        a = Nat.HerArchiveArgsStruct()
        a.rows, a.acts, a.start, a.list = _ptr(fv[0]), _ptr(fv[1]), _ptr(d_start), _ptr(d_list)
        if c["count_dev"]:
            a.count_dev, a.count = _ptr(d_count), -5      # (the host count is ignored)
        else:
            a.count = k
        a.n_worlds, a.T, a.W, a.act_dim, a.t_prev = c["N"], c["T"], W, c["ad"], c["t_prev"]
        if final is not None:
            a.final_rows, a.step_action, a.final_compact = _ptr(fv[2]), _ptr(fv[3]), int(compact)
        a.ep_rows, a.ep_acts, a.ep_meta, a.ep_count, a.episodes = _ptr(ep_rows), _ptr(ep_acts), _ptr(ep_meta), _ptr(ep_count), c["E"]
        Nat.check(L.grx_her_archive(ctypes.byref(a), _stream()))
        keep.append((iw, jw, floats, [start, lst, kd]))
    return dict(c=c, fw=fw, mw=mw, cw=cw, keep=keep, shapes=(st["rows"].shape, st["acts"].shape))


def _archive_check(run):
    c = run["c"]
    want = archive_expected(c)
    rs, as_ = run["shapes"]
    rows, acts = _guarded_read(run["fw"], [int(np.prod(rs)), int(np.prod(as_))], SENT_F)
    (meta,) = _guarded_read(run["mw"], [c["E"] * 4], SENT_I)
    (count,) = _guarded_read(run["cw"], [1], SENT_I)
    tag = {k: v for k, v in c.items()}
    assert int(count[0]) == want["count"], tag
    assert np.array_equal(meta.reshape(-1, 4), want["meta"]), (tag, meta.reshape(-1, 4), want["meta"])
    assert _same(rows.reshape(rs), want["rows"]), tag
    assert _same(acts.reshape(as_), want["acts"]), tag
    for iw, jw, floats, ints in run["keep"]:      # the inputs and their guards are as they were
        got = _guarded_read(iw, [f.size for f in floats], SENT_F)
        assert all(_same(g, f.ravel()) for g, f in zip(got, floats)), tag
        got = _guarded_read(jw, [x.size for x in ints], SENT_I)
        assert all(np.array_equal(g, x.ravel()) for g, x in zip(got, ints)), tag


def _her_args(c, T):
    Nat, _ = _lib()
    a = Nat.HerArgsStruct()
    a.T, a.N, a.W, a.obs_dim, a.goal_dim, a.act_dim = T, 1, c["W"], c["od"], c["gd"], c["ad"]
    a.kind, a.p0, a.p1, a.sparse = c["kind"], c["p0"], c["p1"], c["sparse"]
    a.ignore_pos, a.ignore_rot, a.ignore_z = c["ignore_pos"], c["ignore_rot"], c["ignore_z"]
    return a


class DeviceStore:
    """a store on the device, between sentinels, shared by the launches that sample from it and checked to be unchanged afterwards"""

    def __init__(self, data, lens, count):
        self.E = len(lens)
        self.meta_host = np.stack([lens, np.arange(self.E), np.zeros(self.E), np.zeros(self.E)], axis=1).astype(np.int32)
        self.data = data
        self.fw, (self.rows, self.acts) = _guarded_upload([data[0], data[1]], SENT_F)
        self.mw, (self.meta,) = _guarded_upload([self.meta_host], SENT_I)
        self.cw, (self.count,) = _guarded_upload([np.array([count], np.int64)], np.int64(SENT_I))
        self.count_host = count

    def unchanged(self):
        rows, acts = _guarded_read(self.fw, [self.data[0].size, self.data[1].size], SENT_F)
        (meta,) = _guarded_read(self.mw, [self.E * 4], SENT_I)
        (count,) = _guarded_read(self.cw, [1], SENT_I)
        return _same(rows, self.data[0].ravel()) and _same(acts, self.data[1].ravel()) and np.array_equal(meta, self.meta_host.ravel()) and int(count[0]) == self.count_host


def _sample_launch(c, T, store, strategy, k, seed, call, B):
    torch = _torch()
    Nat, L = _lib()
    OW = R.row_columns(c["od"], c["gd"], c["ad"])[2]
    whole, (out,) = G._guarded_parts([B * OW], torch.float32, SENT_F)
    valid = torch.full((1 + 2 * GUARD,), SENT_I, dtype=torch.int32, device="cuda:0")
    Nat.check(L.grx_her_episode_sample(ctypes.byref(_her_args(c, T)), _ptr(store.rows), _ptr(store.acts), _ptr(store.meta), _ptr(store.count), store.E, strategy, k, seed, call,
                                       B, _ptr(out), _ptr(valid[GUARD:GUARD + 1]), _stream()))
    return whole, valid


def _check_sample(whole, valid, c, data, lens, count, strategy, k, seed, call, B, worst, tag):
    """one guarded launch: the guards, valid[0] = B or 0, and the rows (_compare_rows)"""
    OW = R.row_columns(c["od"], c["gd"], c["ad"])[2]
    (got,) = _guarded_read(whole, [B * OW], SENT_F)
    found = _compare_rows(got, c, data, lens, count, strategy, k, seed, call, B, worst, tag)
    v = valid.cpu().numpy()
    assert (np.delete(v, GUARD) == SENT_I).all() and v[GUARD] == (B if found.any() else 0), tag
    return found


def _compare_rows(got, c, data, lens, count, strategy, k, seed, call, B, worst, tag):
    """rows [B, OW] = ref_episode_rows(ref_episode_draw): copied words bit for bit, reward and success by the rules of the kind (tests/test_gpu_her_refs.py); a store with
    nothing to sample gives an all-zero batch.  Returns found [B]"""
    od, gd, ad = c["od"], c["gd"], c["ad"]
    rc, sc, OW = R.row_columns(od, gd, ad)
    got = np.asarray(got, np.float32).reshape(B, OW)
    want, (e, t, g, found) = expected_rows(c, data, lens, count, strategy, k, seed, call, B)
    if not found.any():
        assert _same(got, np.zeros((B, OW), np.float32)), tag
        return found
    assert found.all(), tag
    copied = np.ones(OW, bool)
    copied[[rc, sc]] = False
    assert _same(got[:, copied], want[:, copied]), tag
    _, r1, goal, _ = P.episode_gather(data[0], data[1], od, gd, e, t, g)
    _, _, dist = R.ref_her_outcome(r1[:, od:od + gd], goal, c["kind"], c["p0"], c["p1"], c["sparse"], c["ignore_pos"], c["ignore_rot"], c["ignore_z"])
    if c["kind"] == 3:
        dp, dr = dist
        clear = (np.abs(dp - c["p0"]) > R.MANIP_CLEAR_POS) & (np.abs(dr - c["p1"]) > R.MANIP_CLEAR_ROT)
        assert _same(got[clear, sc], want[clear, sc]) and np.isin(got[:, sc], (0.0, 1.0)).all(), tag
        if c["sparse"]:
            assert _same(got[clear, rc], want[clear, rc]) and np.isin(got[:, rc], (0.0, -1.0)).all(), tag
        else:
            err = np.abs(got[:, rc].astype(np.float64) + (10.0 * dp + dr))
            worst.add("kind 3 dense reward", err, np.full(len(err), R.MANIP_DENSE_ATOL))
            assert (err <= R.MANIP_DENSE_ATOL).all(), (tag, err.max())
        return found
    assert _same(got[:, sc], want[:, sc]), tag
    if c["sparse"]:
        assert _same(got[:, rc], want[:, rc]), tag      # bits: -0.0 where the goal is reached
    elif c["kind"] == 2:
        err, bound = np.abs(got[:, rc].astype(np.float64) - np.exp(-dist)), R.maze_dense_bound(dist)
        worst.add("kind 2 dense reward exp(-d)", err, bound)
        assert (err <= bound).all(), (tag, (err / bound).max())
    else:
        err, bound = np.abs(got[:, rc].astype(np.float64) + dist), R.dense_bound(dist)
        worst.add(f"kind {c['kind']} dense reward -d", err, bound)
        assert (err <= bound).all(), (tag, (err / bound).max())
    return found


# ================================================================================================================== archive
@pytest.mark.parametrize("N", ARCH_N)
def test_archive_is_the_reference_archive(N):
    """every case of the table: the whole store -- touched and untouched slots, the rows behind an episode's end, meta, count -- and the guards around every buffer"""
    runs = [_archive_launch(c) for c in archive_cases(N)]
    _torch().cuda.synchronize()
    assert len(runs) == 6 * (3 * len({0, 1, N}) * 2 + 3 * 4)
    for run in runs:
        _archive_check(run)


def test_archive_refuses_bad_arguments():
    Nat, L = _lib()
    c = next(iter(archive_cases(3)))
    err = lambda: L.grx_last_error().decode()
    assert L.grx_her_archive(None, None) != 0 and "null argument" in err()
    a = Nat.HerArchiveArgsStruct()
    assert L.grx_her_archive(ctypes.byref(a), None) != 0 and "null buffer" in err()
    dummy = _torch().zeros(64, device="cuda:0")
    for n in ("rows", "acts", "start", "ep_rows", "ep_acts", "ep_meta", "ep_count", "list"):
        setattr(a, n, dummy.data_ptr())
    a.n_worlds, a.T, a.W, a.act_dim, a.t_prev, a.count, a.episodes = 3, c["T"], 4, 1, 0, 1, 2
    assert L.grx_her_archive(ctypes.byref(a), None) != 0 and "episodes" in err()      # fewer slots than worlds
    a.episodes = 3
    a.final_rows = dummy.data_ptr()
    assert L.grx_her_archive(ctypes.byref(a), None) != 0 and "go together" in err()


# ================================================================================================================== sampling
@pytest.mark.parametrize("name", DRAW_STORES)
def test_samples_are_the_reference_rows_of_the_reference_draws(name):
    """every strategy x k_future x seed x call over a store whose count lies below, at and beyond the number of slots; empty, L = 1 and L = T slots among the live ones"""
    lens, count, T = store_lens(name)
    data = store_data(SMALL, len(lens), T, 3)
    store = DeviceStore(data, lens, count)
    runs = [(_sample_launch(SMALL, T, store, *case), case) for case in draw_cases(name)]
    _torch().cuda.synchronize()
    worst = G.Worst()
    for (whole, valid), (strategy, k, seed, call, B) in runs:
        found = _check_sample(whole, valid, SMALL, data, lens, count, strategy, k, seed, call, B, worst, (name, strategy, k, seed, call, B))
        assert found.all()
    assert store.unchanged()
    worst.report()


@pytest.mark.parametrize("name", EMPTY_STORES)
def test_an_empty_store_reports_nothing_to_sample(name):
    """nothing archived (F = 0), every slot empty, and filled slots only beyond F: valid[0] = 0 and an all-zero batch, and nothing behind it"""
    lens, count, T = store_lens(name)
    data = store_data(SMALL, len(lens), T, 4)
    store = DeviceStore(data, lens, count)
    runs = [(_sample_launch(SMALL, T, store, strategy, 4, 11, 0, B), strategy, B) for strategy in STRATEGIES for B in SAMPLE_B]
    _torch().cuda.synchronize()
    for (whole, valid), strategy, B in runs:
        found = _check_sample(whole, valid, SMALL, data, lens, count, strategy, 4, 11, 0, B, G.Worst(), (name, strategy, B))
        assert not found.any()
    assert store.unchanged()


@pytest.mark.parametrize("at", SPARSE_AT)
def test_samples_reach_the_linear_probe(at):
    lens, count, T = sparse_lens(at)
    B = 4096
    _, _, pending = P.episode_attempts(lens.astype(np.int64), 4096, 11, 3, np.arange(B))
    assert pending.mean() > (0.3 if at == "every 64th" else 0.95)      # (1 - 1 / 64)^64 = 0.365, (1 - 1 / 4096)^64 = 0.984
    data = store_data(SMALL, 4096, T, 6)
    store = DeviceStore(data, lens, count)
    runs = [(_sample_launch(SMALL, T, store, strategy, 4, 11, 3, B), strategy) for strategy in STRATEGIES]
    _torch().cuda.synchronize()
    for (whole, valid), strategy in runs:
        assert _check_sample(whole, valid, SMALL, data, lens, count, strategy, 4, 11, 3, B, G.Worst(), (at, strategy)).all()
    assert store.unchanged()


def test_samples_grid_stride_pass():
    """4096 x 32 + 33 samples: the 4096 workgroups take a second chunk each, the last one a chunk of one row"""
    lens, count, T = store_lens("beyond")
    data = store_data(SMALL, len(lens), T, 8)
    store = DeviceStore(data, lens, count)
    whole, valid = _sample_launch(SMALL, T, store, P.FUTURE, 4, 11, 1 << 40, SAMPLE_BIG_B)
    _torch().cuda.synchronize()
    assert _check_sample(whole, valid, SMALL, data, lens, count, P.FUTURE, 4, 11, 1 << 40, SAMPLE_BIG_B, G.Worst(), "grid stride").all()
    assert store.unchanged()


def test_rows_of_every_reward_kind_and_width():
    """kinds 0, 1 (goal widths 1, 15, 16), 2 and 3 at (obs_dim, act_dim) in {(1, 1), (11, 5), (70, 20)}, sparse and dense, odd and even row widths"""
    lens, count = row_lens()
    worst, runs = G.Worst(), []
    for n, (c, strategy, k) in enumerate(row_configs()):
        data = store_data(c, ROW_E, ROW_T, n)
        store = DeviceStore(data, lens, count)
        runs.append((_sample_launch(c, ROW_T, store, strategy, k, 11, n, ROW_B), c, data, strategy, k, n, store))
    _torch().cuda.synchronize()
    assert len(runs) == 8 * 3 * 2
    for (whole, valid), c, data, strategy, k, n, store in runs:
        assert _check_sample(whole, valid, c, data, lens, count, strategy, k, 11, n, ROW_B, worst, (c, strategy, k)).all()
        assert store.unchanged()
    worst.report()


def test_keep_threshold_is_the_integer_compare():
    """sample 0 of the committed calls draws r2 >> 40 exactly at ceil(k 2^24 / (k + 1)) and one below it: the episode's own goal is kept at the boundary and not below it"""
    s = THRESHOLD_STORE
    data = store_data(SMALL, 1, s["T"], 2)
    store = DeviceStore(data, s["lens"], s["count"])
    runs = [(k, m, call, strategy, _sample_launch(SMALL, s["T"], store, strategy, k, s["seed"], call, 1))
            for k, by_m in THRESHOLD_CALLS.items() for m, call in by_m.items() for strategy in STRATEGIES]
    _torch().cuda.synchronize()
    od, gd = SMALL["od"], SMALL["gd"]
    own = data[0][0, 0, od + gd:od + 2 * gd]
    for k, m, call, strategy, (whole, valid) in runs:
        boundary = -(-(k << 24) // (k + 1))
        assert m in (boundary, boundary - 1)
        _, _, m2 = P.episode_uniforms(R.splitmix64(R.splitmix64(P.episode_key(s["seed"], call, [0]))[0])[0])
        assert int(m2[0]) == m      # the case is the one its row names
        _check_sample(whole, valid, SMALL, data, s["lens"], s["count"], strategy, k, s["seed"], call, 1, G.Worst(), (k, m, call, strategy))
        (got,) = _guarded_read(whole, [11], SENT_F)
        g = P.ref_episode_draw(s["lens"], s["count"], 1, strategy, k, s["seed"], call, np.arange(1))[2][0]
        assert (g == -1) == (m == boundary) and (g == -1 or (strategy == P.EPISODE and g == 0) or g == 1)      # (L = 1: the episode strategy may take row 0)
        substituted = data[0][0, max(g, 0), od:od + gd]
        assert not np.array_equal(own, substituted)
        assert _same(got[od + gd:od + 2 * gd], own if m == boundary else substituted), (k, m, strategy)
    assert store.unchanged()
