"""The HER draw and relabel kernels, each entry point called directly and compared with the plain references of tests/her_refs.py: which (row, world, goal row) a given
(seed, call, sample) draws (grx_her_sample, grx_her_sample_final), which packed row a given draw produces (grx_her_relabel), and both at once (grx_her_draw_relabel,
grx_her_sample_relabel).  No environment is built.  Draws and copied words are bit-exact; sparse rewards and success flags of the Euclidean kinds are exact on every pair,
also on pairs placed at the threshold distance; dense rewards and the pose goals of kind 3 have the bounds written down in her_refs.  Every output lies between sentinel words.

The case tables at the top of this file are plain numpy (torch is imported inside the tests only): tests/test_cpu_her_refs.py imports them and shows that references with
one deliberate mistake each give other answers on them."""
import ctypes

import numpy as np
import pytest

import her_refs as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENT_I = -77
SENT_F = -12345.5

# ================================================================================================================== case tables (numpy only)
DRAW_N = [1, 3, 64, 4096]
DRAW_T = [(1, 1), (1, 7), (10, 9), (10, 10), (10, 11), (10, 23), (1000, 5000)]      # (T, t_now): ring not yet full, just full, wrapped
DRAW_K = [0, 1, 4, 7]
DRAW_SEEDS = [0, 11, (1 << 64) - 1]
DRAW_CALLS = [0, 1 << 40]
DRAW_B = [1, 255, 256, 257]
BIG_B = 4096 * 256 + 257          # the sample kernel's grid-stride pass
RELABEL_BIG_B = 95400             # x 11 words: just over 4096 x 256, the relabel kernel's
FUSED_B = [1, 31, 32, 33]
FUSED_BIG_B = 4096 * 32 + 33      # the fused kernel's: more than 4096 chunks of 32 samples


def boundary_state(N, T, t_now):
    """episode marks (start, prev_start, term_t) that mix among the worlds: 0 a start below 0, 1 a start below t_now - T, 2 a start inside the ring, 3 / 4 a world reset in
    this very step whose finished episode began below / above t_now - T, 5 a stale mark equal to the current start, 6 nothing to sample, 7 the start exactly at t_now - T"""
    rng = np.random.default_rng(1000 * N + 10 * T + t_now)
    lo_min = max(t_now - T, 0)
    kinds = {1: [1], 3: [4, 6, 1]}.get(N)
    kinds = np.array(kinds) if kinds else rng.permutation(np.arange(N) % 8)
    inside = lambda: rng.integers(lo_min, t_now, N)      # [lo_min, t_now - 1]
    start, prev, term = inside(), np.full(N, -5), np.full(N, -1)
    start = np.where(kinds == 0, -3, start)
    start = np.where(kinds == 1, t_now - T - 2, start)
    just = (kinds == 3) | (kinds == 4)
    prev = np.where(kinds == 3, t_now - T - 1, np.where(kinds == 4, inside(), prev))
    start, term = np.where(just, t_now, start), np.where(just, t_now, term)
    start = np.where((kinds == 5) & (rng.random(N) < 0.5) & (t_now - T - 1 >= 0), t_now - T - 1, start)      # (a mark one turn of the ring behind row t_now: it shares its ring row)
    term, prev = np.where(kinds == 5, start, term), np.where(kinds == 5, start - 5, prev)
    start = np.where(kinds == 6, t_now, start)
    start = np.where(kinds == 7, t_now - T, start)
    return dict(start=start.astype(np.int32), prev=prev.astype(np.int32), term=term.astype(np.int32))


def draw_cases(N):
    """(T, t_now, k_future, seed, call, B, track) of one world count: every combination, with and without terminal tracking, the batch sizes taken in turn"""
    i = 0
    for T, t_now in DRAW_T:
        for k in DRAW_K:
            for seed in DRAW_SEEDS:
                for call in DRAW_CALLS:
                    for track in (True, False):
                        yield T, t_now, k, seed, call, DRAW_B[i % 4], track
                        i += 1


def marks(st, track):
    return (st["start"], st["prev"], st["term"]) if track else (st["start"], None, None)


SPARSE_AT = [0, 4095, "every 64th"]


def sparse_state(at):
    """4096 worlds of which exactly one -- world `at` -- has a transition: 64 uniform attempts miss it with probability 0.984, nearly every sample ends in the linear probe.
    "every 64th": worlds 5, 69, ... have one; 36 % of the samples probe, and some of them from the world just before such a world (a probe that starts too far passes it)"""
    N, T, t_now = 4096, 10, 23
    start = np.full(N, t_now, np.int32)
    start[slice(5, None, 64) if at == "every 64th" else at] = 17
    return dict(start=start, prev=np.full(N, -5, np.int32), term=np.full(N, -1, np.int32)), N, T, t_now


# calls whose sample 0 (one world, seed 11) draws a u2 of EXACTLY m * 2^-24: {k_future: {m: call}}.  4 / 5 rounds to 13421773 * 2^-24 and a division that is not correctly
# rounded may give either neighbour; 1 / 2 and 7 / 8 are exact quotients (below 1 / 2 the neighbour is no multiple of 2^-24: no u2 can equal it).
THRESHOLD_CALLS = {1: {8388608: 29136401, 8388609: 991957},
                   4: {13421772: 44272039, 13421773: 15185899, 13421774: 34874111},
                   7: {14680063: 25443295, 14680064: 2128024, 14680065: 33239650}}
THRESHOLD_STATE = dict(start=np.zeros(1, np.int32), N=1, T=1, t_now=1, seed=11)

# ---- rows: a ring of T = 3 (four rows) at t_now = 9, five worlds
ROW_T, ROW_NOW, ROW_N = 3, 9, 5
ROW_MARKS = dict(start=np.array([7, 2, 9, 9, 5], np.int32),       # plain | began before the oldest ring row | just ended | just ended, began before the oldest row | stale mark
                 prev=np.array([0, 0, 7, 1, 3], np.int32),
                 term=np.array([-1, -1, 9, 9, 5], np.int32))       # (world 4: mark 5 = ring row 1 = ring row of 9: only the absolute comparison keeps its terminal row out)
ROW_KINDS = [dict(kind=0, gd=3, p0=0.05), dict(kind=1, gd=1, p0=0.01), dict(kind=1, gd=15, p0=0.01), dict(kind=1, gd=16, p0=0.01), dict(kind=2, gd=2, p0=0.45),
             dict(kind=3, gd=7, p0=0.01, p1=0.1), dict(kind=3, gd=7, p0=0.01, p1=0.1, ignore_z=1), dict(kind=3, gd=7, p0=0.01, p1=0.1, ignore_pos=1)]
ROW_DIMS = [(1, 1), (11, 5), (70, 20)]      # (obs_dim, act_dim)
ROW_PAD = [0, 2, 5]                         # W - (obs_dim + 2 goal_dim)


def row_indices(track):
    """every admissible (t, w, t_goal) of the five worlds: t in [lo, t_now - 1], t_goal = -1 or in [t + 1, t_now]"""
    lo = R.her_lo(*marks(ROW_MARKS, track), ROW_NOW, ROW_T)
    out = [(t, w, tg) for w in range(ROW_N) for t in range(int(lo[w]), ROW_NOW) for tg in [-1] + list(range(t + 1, ROW_NOW + 1))]
    t, w, tg = (np.array(x, np.int32) for x in zip(*out))
    return t, w, tg


def row_configs():
    for kc in ROW_KINDS:
        for od, ad in ROW_DIMS:
            for pad in ROW_PAD:
                for sparse in (1, 0):
                    for track in (True, False):
                        c = dict(p1=0.0, ignore_pos=0, ignore_rot=0, ignore_z=0)
                        c.update(kc, od=od, ad=ad, W=od + 2 * kc["gd"] + pad, sparse=sparse, track=track, T=ROW_T, N=ROW_N)
                        yield c


def _unit_quats(rng, base, spread):
    q = base + spread * rng.standard_normal(base.shape)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def ring_data(c, seed):
    """rows [T + 1, N, W], acts [T + 1, N, ad], term_rows [N, W] float32: random observations and padding words, goals scaled so that the distances lie on both sides of the
    threshold (kind 3: positions within about the position threshold, unit quaternions within about the rotation threshold of a common one per world)"""
    rng = np.random.default_rng(seed)
    Rn, N, W, od, gd, ad = c["T"] + 1, c["N"], c["W"], c["od"], c["gd"], c["ad"]
    rows = rng.standard_normal((Rn + 1, N, W))      # (the last slab: the terminal rows)
    if c["kind"] == 3:
        base = _unit_quats(rng, rng.standard_normal((1, N, 4)), 0.0)
        for o in (od, od + gd):
            rows[:, :, o:o + 3] *= 0.004
            rows[:, :, o + 3:o + 7] = _unit_quats(rng, np.broadcast_to(base, (Rn + 1, N, 4)), 0.03)
    else:
        rows[:, :, od:od + 2 * gd] *= c["p0"] / np.sqrt(2.0 * gd)
    rows = rows.astype(np.float32)
    return rows[:Rn].copy(), rng.standard_normal((Rn, N, ad)).astype(np.float32), rows[Rn].copy()


def ref_rows(c, data, t, w, tg, term=None):
    rows, acts, term_rows = data
    return R.ref_her_rows(rows, acts, c["T"], c["N"], c["W"], c["od"], c["gd"], c["ad"], t, w, tg, c["kind"], c["p0"], c["p1"], c["sparse"], c["ignore_pos"], c["ignore_rot"],
                          c["ignore_z"], term_rows if term is not None else None, term)


# ---- pairs at the threshold distance: kinds 0 and 1 take the 3-vectors of R.threshold_pairs(); kind 2 accepts only goal_dim = 2 and takes the same recipe in the plane
PAIR_KINDS = [(0, 3), (1, 3), (2, 2)]      # (kind, goal_dim)


def pair_ring(a, b):
    """one world per pair, a ring of two rows (T = 1), obs_dim = act_dim = 1: b is the desired goal of row 0, a the goal achieved at row 1; sample w = (row 0, world w, -1)"""
    n, gd = a.shape
    rows = np.random.default_rng(n).standard_normal((2, n, 1 + 2 * gd)).astype(np.float32)
    rows[0, :, 1 + gd:], rows[1, :, 1:1 + gd] = b, a
    acts = np.zeros((2, n, 1), np.float32)
    return rows, acts, np.zeros(n, np.int32), np.arange(n, dtype=np.int32), np.full(n, -1, np.int32)


# ---- fused: OW = 11 words
FUSED_DIMS = dict(od=1, gd=2, ad=1, W=5)
FUSED_KINDS = [dict(kind=2, p0=0.45, sparse=1), dict(kind=1, p0=0.01, sparse=0), dict(kind=2, p0=0.45, sparse=0), dict(kind=1, p0=0.01, sparse=1)]


def fused_cases():
    """(N, T, t_now, k_future, seed, call, B, track, kind config, flavour): the ring states of the draw tests (the 4096-world ring of 1001 rows is left out: 80 MB)"""
    i = 0
    for N in DRAW_N:
        for T, t_now in DRAW_T:
            if N == 4096 and T > 10:
                continue
            for track in (True, False):
                for flavour in ("draw", "draw_valid", "sample"):
                    yield N, T, t_now, DRAW_K[i % 4], DRAW_SEEDS[i % 3], DRAW_CALLS[(i // 4) % 2], FUSED_B[(i // 2) % 4], track, FUSED_KINDS[(i // 3) % 4], flavour
                    i += 1


def fused_config(N, T, kc, track):
    c = dict(p1=0.0, ignore_pos=0, ignore_rot=0, ignore_z=0, T=T, N=N, track=track)
    c.update(FUSED_DIMS, **kc)
    return c


# ================================================================================================================== device helpers
def _torch():
    import torch

    return torch


def _lib():
    from gymnasium_robotics_amd import _native

    return _native, _native.lib()


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _dev(x):
    return None if x is None else _torch().from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _guarded_parts(sizes, dtype, fill):
    """(whole, views): len(sizes) arrays in one allocation, GUARD sentinel elements before, between and after them"""
    torch = _torch()
    whole = torch.full((sum(sizes) + GUARD * (len(sizes) + 1),), fill, dtype=dtype, device="cuda:0")
    views, o = [], GUARD
    for n in sizes:
        views.append(whole[o:o + n])
        o += n + GUARD
    return whole, views


def _split_guarded(whole, sizes, fill):
    """host side of _guarded_parts: the arrays, after checking that every guard word kept its sentinel"""
    h = whole.cpu().numpy()
    out, o = [], GUARD
    assert (h[:GUARD] == fill).all()
    for n in sizes:
        out.append(h[o:o + n])
        assert (h[o + n:o + n + GUARD] == fill).all(), "a word behind the output was written"
        o += n + GUARD
    return out


def _sample(st, N, T, t_now, k, seed, call, B, track):
    """one launch of grx_her_sample_final (track) or grx_her_sample: (whole, [B, B, B]) to be read after the synchronisation"""
    Nat, L = _lib()
    start, prev, term = (_dev(x) for x in marks(st, track))
    whole, (t, w, tg) = _guarded_parts([B, B, B], _torch().int32, SENT_I)
    if track:
        Nat.check(L.grx_her_sample_final(_ptr(start), _ptr(prev), _ptr(term), N, t_now, T, k, seed, call, B, _ptr(t), _ptr(w), _ptr(tg), _stream()))
    else:
        Nat.check(L.grx_her_sample(_ptr(start), N, t_now, T, k, seed, call, B, _ptr(t), _ptr(w), _ptr(tg), _stream()))
    return whole, (start, prev, term)


def _check_draw(whole, st, N, T, t_now, k, seed, call, B, track):
    """t and w bit for bit; every keep decision of the launch explained by ONE threshold candidate: returns the candidates that do"""
    t, w, tg = _split_guarded(whole, [B, B, B], SENT_I)
    rt, rw, fut, u2, found = R.ref_her_draw_parts(*marks(st, track), N, t_now, T, seed, call, np.arange(B))
    tag = (N, T, t_now, k, seed, call, B, track)
    assert np.array_equal(t, rt) and np.array_equal(w, rw), tag
    names = R.matching_thresholds(k, fut, u2, tg)
    assert names, tag
    if k == 0:
        assert (tg == -1).all(), tag
    return names, found


def _her_args(c, dev, out, idx=None):
    Nat, _ = _lib()
    a = Nat.HerArgsStruct()
    a.rows, a.acts, a.out = _ptr(dev["rows"]), _ptr(dev["acts"]), _ptr(out)
    a.T, a.N, a.W, a.obs_dim, a.goal_dim, a.act_dim = c["T"], c["N"], c["W"], c["od"], c["gd"], c["ad"]
    a.kind, a.p0, a.p1, a.sparse = c["kind"], c["p0"], c["p1"], c["sparse"]
    a.ignore_pos, a.ignore_rot, a.ignore_z = c["ignore_pos"], c["ignore_rot"], c["ignore_z"]
    if c["track"]:
        a.term_rows, a.term_t = _ptr(dev["term_rows"]), _ptr(dev["term"])
    if idx is not None:
        a.t_idx, a.w_idx, a.t_goal = (_ptr(x) for x in idx)
    return a


def _upload(data, term):
    rows, acts, term_rows = data
    return dict(rows=_dev(rows), acts=_dev(acts), term_rows=_dev(term_rows), term=_dev(term))


class Worst:
    """the largest observed error of every bounded quantity, as a fraction of its bound and in absolute terms"""

    def __init__(self):
        self.seen = {}

    def add(self, name, err, bound):
        if len(err):
            i = int(np.argmax(err / bound))
            old = self.seen.get(name)
            if old is None or err[i] / bound[i] > old[0]:
                self.seen[name] = (float(err[i] / bound[i]), float(err[i]), float(bound[i]))

    def report(self):
        for name, (frac, err, bound) in sorted(self.seen.items()):
            print(f"{name}: worst observed error {err:.3e} at a bound of {bound:.3e} ({frac:.3f} of the bound)")


def _check_rows(got, c, data, t, w, tg, term, worst, tag):
    """one launch's rows against ref_her_rows: every copied word bit for bit, reward and success by the rules of the kind"""
    od, gd, ad = c["od"], c["gd"], c["ad"]
    rc, sc, OW = R.row_columns(od, gd, ad)
    got = np.asarray(got, np.float32).reshape(len(t), OW)
    want = ref_rows(c, data, t, w, tg, term)
    copied = np.ones(OW, bool)
    copied[[rc, sc]] = False
    assert _same(got[:, copied], want[:, copied]), tag
    rows, acts, term_rows = data
    _, r1, goal, _ = R.her_gather(rows, acts, c["T"], c["N"], c["W"], od, gd, ad, t, w, tg, term_rows if term is not None else None, term)
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
        return
    assert _same(got[:, sc], want[:, sc]), tag      # nothing masked
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


# ================================================================================================================== draws
@pytest.mark.parametrize("N", DRAW_N)
def test_draws_are_the_reference_draws(N):
    """every (T, t_now) x k_future x seed x call, with and without terminal tracking, on marks that mix every kind of episode boundary among the worlds"""
    runs = []
    for T, t_now, k, seed, call, B, track in draw_cases(N):
        st = boundary_state(N, T, t_now)
        whole, keep = _sample(st, N, T, t_now, k, seed, call, B, track)
        runs.append((whole, keep, st, (N, T, t_now, k, seed, call, B, track)))
    _torch().cuda.synchronize()
    per_k = {k: {"below", "rounded", "above"} for k in DRAW_K}
    for whole, _, st, case in runs:
        names, _ = _check_draw(whole, st, *case)
        per_k[case[3]] &= set(names)
    for k, names in per_k.items():
        print(f"N = {N}, k_future = {k}: keep threshold candidates that explain every launch: {sorted(names)}")
        assert names


@pytest.mark.parametrize("at", SPARSE_AT)
def test_draws_reach_the_linear_probe(at):
    st, N, T, t_now = sparse_state(at)
    B = 4096
    lo_w = R.her_lo(*marks(st, True), t_now, T)
    assert (lo_w < t_now).sum() == (64 if at == "every 64th" else 1)
    _, _, pending = R.her_attempts(lo_w, N, t_now, 11, 3, np.arange(B))
    assert pending.mean() > (0.3 if at == "every 64th" else 0.95)      # (1 - 1 / 64)^64 = 0.365, (1 - 1 / 4096)^64 = 0.984
    runs = [(_sample(st, N, T, t_now, 4, 11, 3, B, track), track) for track in (True, False)]
    _torch().cuda.synchronize()
    for (whole, _), track in runs:
        _, found = _check_draw(whole, st, N, T, t_now, 4, 11, 3, B, track)
        assert found.all()
        assert at == "every 64th" or (_split_guarded(whole, [B, B, B], SENT_I)[1] == at).all()


def test_draws_grid_stride_pass():
    N, T, t_now, k, seed, call = 64, 10, 23, 4, 11, 0
    st = boundary_state(N, T, t_now)
    whole, _keep = _sample(st, N, T, t_now, k, seed, call, BIG_B, True)
    _torch().cuda.synchronize()
    names, found = _check_draw(whole, st, N, T, t_now, k, seed, call, BIG_B, True)
    print(f"B = {BIG_B}, k_future = 4: keep threshold candidates that explain the launch: {names}")
    assert found.all()


def test_keep_threshold_is_one_candidate():
    """samples whose u2 EQUALS a candidate threshold are the only ones that tell the candidates apart: one launch each, and one candidate must explain all of a k_future's"""
    s = THRESHOLD_STATE
    st = dict(start=s["start"], prev=None, term=None)
    runs = [(k, m, call, _sample(st, s["N"], s["T"], s["t_now"], k, s["seed"], call, 1, False)) for k, by_m in THRESHOLD_CALLS.items() for m, call in by_m.items()]
    _torch().cuda.synchronize()
    per_k = {k: {"below", "rounded", "above"} for k in THRESHOLD_CALLS}
    for k, m, call, (whole, _) in runs:
        _, _, _, u2, _ = R.ref_her_draw_parts(s["start"], None, None, s["N"], s["t_now"], s["T"], s["seed"], call, np.arange(1))
        assert u2[0] == np.float32(m) / np.float32(16777216.0)      # the case is the one its row names
        names, _ = _check_draw(whole, st, s["N"], s["T"], s["t_now"], k, s["seed"], call, 1, False)
        per_k[k] &= set(names)
    for k, names in per_k.items():
        print(f"k_future = {k}: the device's keep threshold is the candidate {sorted(names)}")
        assert len(names) == 1 or (k == 1 and names)      # below 1 / 2 the neighbour is no multiple of 2^-24: two candidates decide every possible u2 alike


# ================================================================================================================== rows
def test_rows_are_the_reference_rows():
    """every admissible (t, t_goal) of the five worlds, for every reward kind, goal width, row width, padding, dense and sparse, with and without terminal rows"""
    torch = _torch()
    Nat, L = _lib()
    worst, runs = Worst(), []
    for n, c in enumerate(row_configs()):
        data = ring_data(c, n)
        term = ROW_MARKS["term"] if c["track"] else None
        t, w, tg = row_indices(c["track"])
        dev = _upload(data, term)
        idx = [_dev(x) for x in (t, w, tg)]
        OW = R.row_columns(c["od"], c["gd"], c["ad"])[2]
        whole, (out,) = _guarded_parts([len(t) * OW], torch.float32, SENT_F)
        Nat.check(L.grx_her_relabel(ctypes.byref(_her_args(c, dev, out, idx)), len(t), _stream()))
        runs.append((c, data, term, (t, w, tg), whole, OW, (dev, idx)))
    torch.cuda.synchronize()
    assert len(runs) == 8 * 3 * 3 * 2 * 2
    for c, data, term, (t, w, tg), whole, OW, _ in runs:
        (got,) = _split_guarded(whole, [len(t) * OW], SENT_F)
        _check_rows(got, c, data, t, w, tg, term, worst, {k: v for k, v in c.items() if k not in ("T", "N")})
    worst.report()


@pytest.fixture(scope="module")
def pairs():
    return {3: R.threshold_pairs(3), 2: R.threshold_pairs(2)}


@pytest.mark.parametrize("thr", R.PAIR_THRESHOLDS)
def test_outcomes_at_the_threshold_distance(pairs, thr):
    """the 4096 pairs nearest the threshold on either side: sparse reward and success exact on every one of them, for kinds 0, 1 and 2"""
    torch = _torch()
    Nat, L = _lib()
    worst, runs = Worst(), []
    for kind, gd in PAIR_KINDS:
        a, b, d = R.nearest_pairs(*pairs[gd][thr], thr)
        assert len(d) == 2 * R.PAIRS_KEPT and (d != thr).all()
        print(f"kind {kind}, threshold {thr}: the pairs lie within {np.abs(d - thr).max():.3e} of it, the nearest {np.abs(d - thr).min():.3e}")
        rows, acts, t, w, tg = pair_ring(a, b)
        for sparse in (1, 0):
            c = dict(kind=kind, gd=gd, od=1, ad=1, W=1 + 2 * gd, T=1, N=len(d), p0=thr, p1=0.0, sparse=sparse, ignore_pos=0, ignore_rot=0, ignore_z=0, track=False)
            data = (rows, acts, None)
            dev, idx = _upload((rows, acts, None), None), [_dev(x) for x in (t, w, tg)]
            OW = R.row_columns(1, gd, 1)[2]
            whole, (out,) = _guarded_parts([len(d) * OW], torch.float32, SENT_F)
            Nat.check(L.grx_her_relabel(ctypes.byref(_her_args(c, dev, out, idx)), len(d), _stream()))
            runs.append((c, data, (t, w, tg), whole, OW, d, (dev, idx)))
    torch.cuda.synchronize()
    for c, data, (t, w, tg), whole, OW, d, _ in runs:
        (got,) = _split_guarded(whole, [len(t) * OW], SENT_F)
        _check_rows(got, c, data, t, w, tg, None, worst, (c["kind"], thr, c["sparse"]))
        sc = R.row_columns(1, c["gd"], 1)[1]
        success = got.reshape(len(t), OW)[:, sc]
        assert success[:R.PAIRS_KEPT].sum() == 0 and success[R.PAIRS_KEPT:].sum() == R.PAIRS_KEPT      # beyond the threshold first, then within it
    worst.report()


def test_rows_grid_stride_pass():
    """95 400 rows of 11 words: the relabel kernel's 4096 x 256 threads take a second pass"""
    torch = _torch()
    Nat, L = _lib()
    N, T, t_now = 64, 10, 23
    c = fused_config(N, T, FUSED_KINDS[0], True)
    st = boundary_state(N, T, t_now)
    data = ring_data(c, 5)
    t, w, tg, found = R.ref_her_draw(*marks(st, True), N, t_now, T, 4, 11, 0, np.arange(RELABEL_BIG_B))
    assert found.all() and RELABEL_BIG_B * 11 > 4096 * 256 >= (RELABEL_BIG_B - 100) * 11
    dev, idx = _upload(data, st["term"]), [_dev(x) for x in (t, w, tg)]
    whole, (out,) = _guarded_parts([RELABEL_BIG_B * 11], torch.float32, SENT_F)
    Nat.check(L.grx_her_relabel(ctypes.byref(_her_args(c, dev, out, idx)), RELABEL_BIG_B, _stream()))
    torch.cuda.synchronize()
    (got,) = _split_guarded(whole, [RELABEL_BIG_B * 11], SENT_F)
    _check_rows(got, c, data, t, w, tg, st["term"], Worst(), "grid stride")


# ================================================================================================================== fused
def _fused_launch(c, dev, st, t_now, k, seed, call, B, flavour):
    torch = _torch()
    Nat, L = _lib()
    start, prev, _ = (_dev(x) for x in marks(st, c["track"]))
    whole, (out,) = _guarded_parts([B * 11], torch.float32, SENT_F)
    valid = scratch = None
    a = _her_args(c, dev, out)
    if flavour == "draw":
        Nat.check(L.grx_her_draw_relabel(ctypes.byref(a), _ptr(start), _ptr(prev), t_now, k, seed, call, B, None, _stream()))
    else:
        valid = torch.full((1 + 2 * GUARD,), SENT_I, dtype=torch.int32, device="cuda:0")
        v = valid[GUARD:GUARD + 1]
        if flavour == "draw_valid":
            Nat.check(L.grx_her_draw_relabel(ctypes.byref(a), _ptr(start), _ptr(prev), t_now, k, seed, call, B, _ptr(v), _stream()))
        else:
            scratch = torch.full((3 * B,), SENT_I, dtype=torch.int32, device="cuda:0")
            Nat.check(L.grx_her_sample_relabel(ctypes.byref(a), _ptr(start), _ptr(prev), t_now, k, seed, call, B, _ptr(scratch), _ptr(v), _stream()))
    return whole, valid, (start, prev, scratch)


def _check_fused(whole, valid, c, data, st, t_now, k, seed, call, B, worst, tag):
    """the launch's rows = ref_her_rows(ref_her_draw) for ONE threshold candidate; valid[0] = B; returns the candidates that explain it"""
    (got,) = _split_guarded(whole, [B * 11], SENT_F)
    term = st["term"] if c["track"] else None
    t, w, fut, u2, found = R.ref_her_draw_parts(*marks(st, c["track"]), c["N"], t_now, c["T"], seed, call, np.arange(B))
    assert found.all(), tag
    if valid is not None:
        v = valid.cpu().numpy()
        assert v[GUARD] == B and (np.delete(v, GUARD) == SENT_I).all(), tag
    names, tried, failure = [], [], None
    for name, thr in zip(("below", "rounded", "above"), R.keep_thresholds(k)):
        tg = np.where(u2 >= thr, np.int32(-1), fut).astype(np.int32)
        same = [n for n, g in tried if np.array_equal(g, tg)]
        if same:      # the same draws as an earlier candidate: the same verdict
            if same[0] in names:
                names.append(name)
            continue
        tried.append((name, tg))
        try:
            _check_rows(got, c, data, t, w, tg, term, worst, tag)
            names.append(name)
        except AssertionError as e:
            failure = e
    if not names:
        raise failure
    return names


def test_fused_rows_are_the_reference_rows_of_the_reference_draws():
    torch = _torch()
    worst, runs, rings = Worst(), [], {}
    for N, T, t_now, k, seed, call, B, track, kc, flavour in fused_cases():
        c = fused_config(N, T, kc, track)
        st = boundary_state(N, T, t_now)
        key = (N, T, t_now, c["kind"])
        if key not in rings:      # one ring per state and goal scale, shared by its launches and left unchanged
            data = ring_data(c, 7 * N + T)
            rings[key] = (data, _upload(data, st["term"]))
        data, dev = rings[key]
        whole, valid, keep = _fused_launch(c, dev, st, t_now, k, seed, call, B, flavour)
        runs.append((whole, valid, c, data, st, t_now, k, seed, call, B, keep, (N, T, t_now, k, seed, call, B, track, kc, flavour)))
    torch.cuda.synchronize()
    per_k = {k: {"below", "rounded", "above"} for k in DRAW_K}
    for whole, valid, c, data, st, t_now, k, seed, call, B, _, tag in runs:
        per_k[k] &= set(_check_fused(whole, valid, c, data, st, t_now, k, seed, call, B, worst, tag))
    assert all(per_k.values())
    worst.report()


@pytest.mark.parametrize("flavour", ["draw", "draw_valid", "sample"])
def test_fused_grid_stride_pass(flavour):
    """4096 x 32 + 33 samples: the 4096 workgroups take a second chunk each, the last one a chunk of one row"""
    N, T, t_now, k, seed, call = 64, 10, 23, 4, 11, 1 << 40
    c = fused_config(N, T, FUSED_KINDS[0], True)
    st = boundary_state(N, T, t_now)
    data = ring_data(c, 9)
    dev = _upload(data, st["term"])
    whole, valid, _keep = _fused_launch(c, dev, st, t_now, k, seed, call, FUSED_BIG_B, flavour)
    _torch().cuda.synchronize()
    names = _check_fused(whole, valid, c, data, st, t_now, k, seed, call, FUSED_BIG_B, Worst(), flavour)
    print(f"B = {FUSED_BIG_B}, k_future = 4: keep threshold candidates that explain the launch: {names}")


@pytest.mark.parametrize("track", [True, False])
def test_fused_empty_replay_reports_nothing_to_sample(track):
    """no world has a transition: grx_her_sample_relabel writes valid[0] = 0 and an all-zero slot, and nothing behind it"""
    torch = _torch()
    N, T, t_now, B = 64, 10, 23, 33
    c = fused_config(N, T, FUSED_KINDS[0], track)
    st = dict(start=np.full(N, t_now, np.int32), prev=np.full(N, t_now, np.int32), term=np.where(np.arange(N) % 2, t_now, -1).astype(np.int32))
    assert not (R.her_lo(*marks(st, track), t_now, T) < t_now).any()
    dev = _upload(ring_data(c, 3), st["term"])
    whole, valid, _keep = _fused_launch(c, dev, st, t_now, 4, 11, 0, B, "sample")
    torch.cuda.synchronize()
    (got,) = _split_guarded(whole, [B * 11], SENT_F)
    v = valid.cpu().numpy()
    assert v[GUARD] == 0 and (np.delete(v, GUARD) == SENT_I).all()
    assert _same(got, np.zeros(B * 11, np.float32))
