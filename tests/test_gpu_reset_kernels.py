"""The reset path's small kernels, each called directly and compared with the plain references of tests/reset_refs.py at the shapes where such kernels break:
grx_kitchen_bookkeeping (world counts around a 256-thread block, every mode and flag, pending worlds on carried state, stepped / final_info NULL), grx_hand_commit_rows and
grx_adroit_commit_rows (rows wider than a wave, the two status merges over all bit patterns, NULL pairs), grx_maze_reset_rows / _list (obs_skip, keep_outcome, packed NULL,
success at the goal radius), the samplers grx_fetch_sample_resets_device, grx_adroit_sample_resets_device, grx_maze_sample_resets_device / _list and
grx_uniform_rows_device (list lengths around a wave and a block, sparse permuted lists, streams that were advanced or hold a buffered half, the bounded rejection loops),
and the stand-alone reward kernels (batch 1 and a batch whose last three elements take the second grid-stride pass).  No environment is built.  Every buffer a kernel
writes lies between sentinel words and starts out filled with sentinels; every comparison is bit for bit over the WHOLE buffer -- the rows of unlisted worlds included --
except the dense rewards, which have the derived bounds of tests/her_refs.py."""
import ctypes

import numpy as np
import pytest

import her_refs as H
import reset_refs as R
from test_gpu_bookkeeping import _dev, _guarded, _guards_intact, _host, _lib, _ptr, _same, _stream, _torch

pytestmark = pytest.mark.gpu

FILL = {np.dtype(np.float32): R.SENT_F, np.dtype(np.float64): R.SENT_F, np.dtype(np.int32): R.SENT_I, np.dtype(np.int64): R.SENT_I, np.dtype(np.uint8): R.SENT_B}


class _Buf:
    """a host array's content in device memory between sentinel words"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.dtype, self.shape = arr.dtype, arr.shape
        raw = arr.view(np.int64) if arr.dtype == np.uint64 else arr
        self.fill = FILL[raw.dtype]
        t = _torch().from_numpy(raw.reshape(-1))
        self.whole, self.view = _guarded(raw.size, t.dtype, self.fill)
        self.view.copy_(t)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        return _host(self.view).view(self.dtype).reshape(self.shape)

    def intact(self):
        return _guards_intact(self.whole, self.view.numel(), self.fill)


def _put(arr):
    return None if arr is None else _Buf(arr)


def _p(buf):
    return None if buf is None else buf.ptr


def _beyond(idx, N):
    """two entries to put behind a list: worlds the list does not name (a kernel that reads past the list's end then changes a world that must stay, where an invalid
    index would send its write anywhere), or with every world listed the first one again"""
    rest = [w for w in range(N) if w not in set(int(x) for x in idx)]
    return (rest + [int(idx[0])] * 2)[:2]


def _sync():
    _torch().cuda.synchronize()


def _check(bufs, want, tag):
    """every buffer equals the reference's, bit for bit, and no sentinel around it was touched"""
    for f, b in bufs.items():
        if b is not None:
            assert _same(b.get(), np.asarray(want[f], dtype=b.dtype).reshape(b.shape)), (f, tag)
            assert b.intact(), (f, tag)


# ================================================================================================================== kitchen
@pytest.mark.parametrize("N", R.KITCHEN_N)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_kitchen_bookkeeping_is_the_per_world_loop(mode, N):
    """the chains of R.kitchen_chains on device buffers that are carried from call to call, every buffer compared after every call"""
    Nat, L = _lib()
    pending = 0
    for chain in R.kitchen_chains(N, mode):
        cfg, kind, init_qpos, state, calls = chain
        d = {f: _put(state[f]) for f in R.KITCHEN_FIELDS}
        d_init = _dev(init_qpos)
        book = Nat.KitchenBookStruct()
        for f in R.KITCHEN_FIELDS:
            setattr(book, f, _p(d[f]))
        book.init_qpos = d_init.data_ptr()
        for f in ("nq", "nv", "all_mask", "max_steps", "remove_when_completed", "terminate_when_completed", "mode"):
            setattr(book, f, cfg[f])
        for step, ((completed, stepped), want) in enumerate(zip(calls, R.kitchen_walk(chain))):
            d_completed, d_stepped = _dev(completed), None if stepped is None else _dev(stepped)
            book.completed, book.stepped = d_completed.data_ptr(), _ptr(d_stepped)
            pending += int(mode == 1 and d["needs_reset"].get().any())
            Nat.check(L.grx_kitchen_bookkeeping(ctypes.byref(book), N, _stream()))
            _sync()
            _check(d, want, (cfg, kind, step))
            for f in ("qpos", "qvel", "qacc_ws"):      # the step between two calls moves the worlds (as R.kitchen_chains assumes)
                d[f].view.add_(1.0)
    assert mode != 1 or pending >= 3      # pending worlds did occur


def test_kitchen_bookkeeping_rejects_bad_arguments():
    Nat, L = _lib()
    assert L.grx_kitchen_bookkeeping(None, 4, _stream()) == -1
    book = Nat.KitchenBookStruct()      # every buffer NULL
    book.nq, book.nv, book.mode = 3, 2, 1
    assert L.grx_kitchen_bookkeeping(ctypes.byref(book), 4, _stream()) == -1


# ================================================================================================================== commits
HAND_STAGED = R.HAND_ROWS + ("packed", "status")      # grx_hand_commit_args: s_qpos .. s_goal, s_packed, s_status, then the live ones in the same order
ADROIT_STAGED = R.ADROIT_ROWS + ("status",)


def _hand_run(dims, live, staged, idx, tag):
    Nat, L = _lib()
    nq, nv, od, gd = dims
    k = len(idx)
    d_live, d_staged = {f: _put(v) for f, v in live.items()}, {f: _put(v) for f, v in staged.items()}
    d_idx = _dev(np.asarray(list(idx) + _beyond(idx, R.COMMIT_N), np.int64))      # (entries past k are never read)
    args = Nat.HandCommitArgsStruct(d_idx.data_ptr(), k, nq, nv, od, gd, *[_p(d_staged[f]) for f in HAND_STAGED], *[_p(d_live[f]) for f in HAND_STAGED])
    Nat.check(L.grx_hand_commit_rows(ctypes.byref(args), _stream()))
    _sync()
    _check(d_live, R.hand_commit(live, staged, idx, k, od, gd), tag)      # the listed worlds' rows AND every other world's
    _check(d_staged, staged, tag)                                          # the staged block stays


@pytest.mark.parametrize("dims", R.HAND_DIMS)
def test_hand_commit_is_the_numpy_copy(dims):
    for call, idx in enumerate(R.commit_lists()):
        live, staged = R.hand_case(dims, call)
        _hand_run(dims, live, staged, idx, (dims, call))


def _adroit_run(dims, live, staged, idx, tag):
    Nat, L = _lib()
    nq, nv, od = dims
    k = len(idx)
    d_live, d_staged = {f: _put(v) for f, v in live.items()}, {f: _put(v) for f, v in staged.items()}
    d_idx = _dev(np.asarray(list(idx) + _beyond(idx, R.COMMIT_N), np.int64))
    args = Nat.AdroitCommitArgsStruct(d_idx.data_ptr(), k, nq, nv, od, *[_p(d_staged[f]) for f in ADROIT_STAGED], *[_p(d_live[f]) for f in ADROIT_STAGED])
    rc = L.grx_adroit_commit_rows(ctypes.byref(args), _stream())
    _sync()
    return rc, d_live, d_staged


@pytest.mark.parametrize("dims", R.ADROIT_DIMS)
@pytest.mark.parametrize("pairs", [True, False])
def test_adroit_commit_is_the_numpy_copy(pairs, dims):
    for call, idx in enumerate(R.commit_lists()):
        live, staged = R.adroit_case(dims, call, pairs)
        rc, d_live, d_staged = _adroit_run(dims, live, staged, idx, (dims, call))
        assert rc == 0
        _check(d_live, R.adroit_commit(live, staged, idx, len(idx)), (dims, pairs, call))
        _check(d_staged, staged, (dims, pairs, call))


@pytest.mark.parametrize("half", ["shift", "target", "s_shift", "s_target"])
def test_adroit_commit_mismatched_pair_launches_nothing(half):
    dims = R.ADROIT_DIMS[0]
    live, staged = R.adroit_case(dims, 0, True)
    (staged if half.startswith("s_") else live)[half[2:] if half.startswith("s_") else half] = None
    rc, d_live, d_staged = _adroit_run(dims, live, staged, list(range(R.COMMIT_N)), half)
    assert rc == -1
    _check(d_live, live, half)
    _check(d_staged, staged, half)


@pytest.mark.parametrize("family", ["hand", "adroit"])
def test_commit_status_words_over_all_bit_patterns(family):
    """four calls over all 64 worlds: the low four bits of the old and the staged word run through all 256 pairs, the other bits -- the sticky half with bit 16 and the
    sign bit, the bits of value 16 and 32 of the low half -- are random.  The two kernels merge differently ON PURPOSE: each is held to its own reference, and the two
    references are shown to disagree on these very words."""
    idx = list(range(R.COMMIT_N))[::-1]
    for call in range(4):
        if family == "hand":
            dims = R.HAND_DIMS[2]
            live, staged = R.hand_case(dims, call)
            _hand_run(dims, live, staged, idx, call)
            other = R.hand_commit(live, staged, idx, len(idx), dims[2], dims[3], mistake="status_adroit_way")["status"]
            assert not np.array_equal(other, R.hand_commit(live, staged, idx, len(idx), dims[2], dims[3])["status"])
        else:
            dims = R.ADROIT_DIMS[0]
            live, staged = R.adroit_case(dims, call, call % 2 == 0)
            rc, d_live, _ = _adroit_run(dims, live, staged, idx, call)
            want = R.adroit_commit(live, staged, idx, len(idx))
            assert rc == 0
            _check(d_live, want, call)
            assert not np.array_equal(want["status"], R.adroit_commit(live, staged, idx, len(idx), mistake="status_hand_way")["status"])
            assert not np.array_equal(want["status"], R.adroit_commit(live, staged, idx, len(idx), mistake="bit16_leak")["status"])


# ================================================================================================================== maze rows
MAZE_OUT = ("qpos", "qvel", "qacc_ws", "goal", "obs", "achieved", "reward", "success", "packed")      # grx_maze_reset_args' output pointers, in order


@pytest.mark.parametrize("dims", R.MAZE_ROW_DIMS)
@pytest.mark.parametrize("entry", ["rows", "list"])
def test_maze_reset_rows_are_the_numpy_rows(entry, dims):
    """17 scattered worlds of 48; the list entry point reads the count from device memory (17, below max_n = 20) and writes the goal to `desired` as well"""
    Nat, L = _lib()
    nq, nv, skip = dims
    seed = 0
    for keep in (0, 1):
        for packed in (1, 0):
            seed += 1
            live, idx, k, stage, qpos0, radius = R.maze_row_case(dims, keep, packed, seed)
            if entry == "rows":
                live["desired"] = None
            d = {f: _put(live[f]) for f in R.MAZE_ROW_FIELDS}
            max_n = k + 3
            d_stage = _put(np.concatenate([stage, np.full((max_n - k, 4), 0.25, np.float32)]))      # rows at or beyond the count: valid numbers that must not be used
            d_idx, d_q0 = _dev(idx), _dev(qpos0)
            args = Nat.MazeResetArgsStruct(d_idx.data_ptr(), d_stage.ptr, d_q0.data_ptr(), nq, nv, nq + nv - skip, skip, radius, keep, *[_p(d[f]) for f in MAZE_OUT])
            if entry == "rows":
                Nat.check(L.grx_maze_reset_rows(ctypes.byref(args), k, _stream()))
            else:
                d_cnt = _dev(np.array([k], np.int32))
                Nat.check(L.grx_maze_reset_rows_list(ctypes.c_void_p(ctypes.addressof(args)), ctypes.c_void_p(d_cnt.data_ptr()), ctypes.c_int(max_n),
                                                     ctypes.c_void_p(d["desired"].ptr), _stream()))
            _sync()
            want = R.maze_reset_rows(live, idx, k, stage, qpos0, nq, nv, skip, radius, keep)
            tag = (dims, entry, keep, packed)
            _check(d, want, tag)
            assert d_stage.intact() and _same(d_stage.get()[:k], stage), tag
            succ = want["success"][idx[:k]]
            assert succ[:3].tolist() == [1, 1, 0] and 0 < succ.sum() < k, tag      # at the radius, one ulp inside, one ulp outside


# ================================================================================================================== samplers
def _idx32(idx, extra=()):
    return _dev(np.asarray(list(idx) + list(extra), np.int32))


def _fetch_launch(d_rows, d_idx, n, c, d_samples):
    Nat, L = _lib()
    toff, g0 = np.array(R.FETCH_OFFSET, np.float64), np.array(R.FETCH_GRIPPER, np.float64)      # host pointers
    Nat.check(L.grx_fetch_sample_resets_device(d_rows.ptr, d_idx.data_ptr(), n, c["has_object"], c["in_air"], c["obj_range"], c["target_range"], toff.ctypes.data,
                                               g0.ctypes.data, R.FETCH_HEIGHT, d_samples.ptr, _stream()))


@pytest.mark.parametrize("n", R.SAMPLER_N)
def test_fetch_sampler_is_numpy(n):
    """n worlds of 300, a sparse permuted list; two consecutive resets; samples, every stream row (the unlisted worlds' too) and the sentinels around both"""
    for c in R.fetch_cfgs():
        rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 500 + n), R.sparse_list(n, n)
        d_rows, d_idx = _put(rows), _idx32(idx, _beyond(idx, R.SAMPLER_WORLDS))
        want_rows = rows
        for call in range(2):
            d_samples = _put(np.full((n, 5), R.SENT_F, np.float32))
            _fetch_launch(d_rows, d_idx, n, c, d_samples)
            _sync()
            want_rows, want = R.fetch_reference(want_rows, idx, c)
            _check(dict(samples=d_samples, rows=d_rows), dict(samples=want.astype(np.float32), rows=want_rows), (c, call))
            if not c["has_object"]:      # nothing is drawn for the object: the gripper's x and y
                assert (d_samples.get()[:, :2] == np.array(R.FETCH_GRIPPER[:2], np.float32)).all()
        rest = np.setdiff1d(np.arange(R.SAMPLER_WORLDS), idx)
        got = d_rows.get()
        assert np.array_equal(got[rest], rows[rest]) and not (got[idx] == rows[idx]).all(axis=1).any()


def test_fetch_sampler_gives_up_after_65536_rejections():
    """obj_range = 0.05 can never clear the 0.1 m ring around the gripper: one thread walks 65 536 rejected pairs, then poisons the object words with NaN and goes on to
    the goal, which therefore equals numpy's drawn after bit_generator.advance(131072); the stream ends right behind the goal draws"""
    n, c = 3, dict(has_object=1, in_air=0, obj_range=0.05, target_range=0.15)
    rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 900), R.sparse_list(n, 33)
    d_rows, d_idx, d_samples = _put(rows), _idx32(idx, _beyond(idx, R.SAMPLER_WORLDS)), _put(np.full((n, 5), R.SENT_F, np.float32))
    _fetch_launch(d_rows, d_idx, n, c, d_samples)
    _sync()
    want_rows, want = R.fetch_reference(rows, idx, c)
    _check(dict(samples=d_samples, rows=d_rows), dict(samples=want.astype(np.float32), rows=want_rows), "guard")
    got, got_rows = d_samples.get(), d_rows.get()
    for k, w in enumerate(idx):
        g = R.rng_from_row(list(rows[w]) + [0])
        g.bit_generator.advance(2 * R.GUARD_DRAWS)
        goal = [R.FETCH_GRIPPER[e] + g.uniform(-0.15, 0.15) + R.FETCH_OFFSET[e] for e in range(2)]
        g.uniform(-0.15, 0.15)      # (z is drawn, then replaced by the height offset)
        assert np.isnan(got[k, :2]).all() and got[k, 2:].tolist() == [np.float32(goal[0]), np.float32(goal[1]), np.float32(R.FETCH_HEIGHT)], k
        assert R.rng_row(g)[:4] == [int(x) for x in got_rows[w]], k


ADROIT_BUFS = ("edit", "target64", "shift", "target")


def _adroit_bufs(seed):
    """edit rows preset to distinct values (the kept components must survive), the outputs sentinel-filled"""
    N = R.SAMPLER_WORLDS
    return dict(edit=np.random.default_rng(seed).uniform(-1.0, 1.0, (N, 3)), target64=np.full((N, 3), R.SENT_F, np.float64), shift=np.full((N, 7), R.SENT_F, np.float32),
                target=np.full((N, 3), R.SENT_F, np.float32))


def _adroit_launch(d_rows, d_idx, n, kind, d, with_target=True):
    Nat, L = _lib()
    pos0 = np.array(R.ADROIT_POS0, np.float64)      # host pointer
    return L.grx_adroit_sample_resets_device(d_rows.ptr, d_idx.data_ptr(), n, kind, pos0.ctypes.data, d["edit"].ptr, d["target64"].ptr if with_target else None, d["shift"].ptr,
                                             d["target"].ptr if with_target else None, _stream())


@pytest.mark.parametrize("n", R.SAMPLER_N)
@pytest.mark.parametrize("kind", [0, 1, 3])
def test_adroit_sampler_is_numpy(kind, n):
    rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 600 + n), R.sparse_list(n, n + kind)
    bufs = _adroit_bufs(n)
    d_rows, d_idx, d = _put(rows), _dev(np.concatenate([idx, _beyond(idx, R.SAMPLER_WORLDS)]).astype(np.int64)), {f: _put(bufs[f]) for f in ADROIT_BUFS}
    want_rows, want = rows, bufs
    for call in range(2):
        assert _adroit_launch(d_rows, d_idx, n, kind, d, with_target=(kind == 3 or call == 1)) == 0      # hammer / door: the target rows NULL, or given and left alone
        _sync()
        want_rows, want = R.adroit_reference(want_rows, idx, kind, want)
        _check(dict(d, rows=d_rows), dict(want, rows=want_rows), (kind, call))
    got, kept = d["edit"].get()[idx], {0: [0, 1], 1: [], 3: [2]}[kind]
    drawn = [c for c in range(3) if c not in kept]
    assert np.array_equal(got[:, kept], bufs["edit"][idx][:, kept]) and (got[:, drawn] != bufs["edit"][idx][:, drawn]).all()      # the kept components of edit survive
    target = d["target"].get()
    assert (target[idx] != R.SENT_F).all() if kind == 3 else (target == R.SENT_F).all()


@pytest.mark.parametrize("kind, with_target", [(2, True), (3, False), (-1, True), (4, True)])
def test_adroit_sampler_rejects_the_pen_and_a_relocate_without_target_rows(kind, with_target):
    rows, idx, bufs = R.stream_rows(R.SAMPLER_WORLDS, 600), R.sparse_list(65, 1), _adroit_bufs(0)
    d_rows, d_idx, d = _put(rows), _dev(idx), {f: _put(bufs[f]) for f in ADROIT_BUFS}
    assert _adroit_launch(d_rows, d_idx, 65, kind, d, with_target) == -1
    _sync()
    _check(dict(d, rows=d_rows), dict(bufs, rows=rows), kind)      # nothing was launched


def _maze_launch(entry, d_rows, d_idx, n, goal_xy, reset_xy, noise, scaling, fixed_goal, fixed_reset, d_stage, max_n=None):
    Nat, L = _lib()
    d_g, d_r = _dev(goal_xy), _dev(reset_xy)
    if entry == "device":
        fg, fr = (None if v is None else np.array(v, np.float64) for v in (fixed_goal, fixed_reset))      # host pointers
        Nat.check(L.grx_maze_sample_resets_device(d_rows.ptr, d_idx.data_ptr(), n, d_g.data_ptr(), len(goal_xy), d_r.data_ptr(), len(reset_xy), noise, scaling,
                                                  None if fg is None else fg.ctypes.data, None if fr is None else fr.ctypes.data, d_stage.ptr, _stream()))
    else:
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        d_cnt = _dev(np.array([n], np.int32))
        Nat.check(L.grx_maze_sample_resets_list(vp(d_rows.ptr), vp(d_idx.data_ptr()), vp(d_cnt.data_ptr()), ci(max_n), vp(d_g.data_ptr()), ci(len(goal_xy)), vp(d_r.data_ptr()),
                                                ci(len(reset_xy)), cd(noise), cd(scaling), vp(d_stage.ptr), _stream()))
    _sync()


def _maze_configs():
    """(n_goal, n_reset, fixed goal, fixed reset, scaling): the five cell-count pairs without options, and the four combinations of the two options"""
    out = [(ng, nr, None, None, (1.0, 4.0)[i % 2]) for i, (ng, nr) in enumerate(R.MAZE_CELL_COUNTS)]
    return out + [(7, 3, (0.5, 2.5), None, 1.0), (3, 7, None, (-1.5, -0.5), 4.0), (2, 2, (0.5, 2.5), (-1.5, -0.5), 1.0)]


@pytest.mark.parametrize("n", R.SAMPLER_N)
@pytest.mark.parametrize("entry", ["device", "list"])
def test_maze_sampler_is_numpy(entry, n):
    """rows [300, 5] of which every third enters with a buffered 32-bit half; the list entry point takes the count (n) from device memory with max_n = n + 7, and the
    seven entries beyond the count name worlds that must not draw"""
    idx_all = R.sparse_list(min(n + 7, R.SAMPLER_WORLDS), n)
    idx = idx_all[:n]
    buffered_in = 0
    for ng, nr, fg, fr, scaling in _maze_configs():
        if entry == "list" and (fg is not None or fr is not None):
            continue      # (the list entry point has no options)
        goal_xy, reset_xy = R.maze_cells(ng, scaling), R.maze_reset_cells(nr, scaling)
        rows = R.stream_rows(R.SAMPLER_WORLDS, 800 + n, wide=True, buffered=True)
        buffered_in += int(((rows[idx, 4] >> np.uint64(32)) != 0).sum())
        d_rows, d_idx = _put(rows), _idx32(idx_all)
        want_rows = rows
        for call in range(2):
            d_stage = _put(np.full((len(idx_all), 4), R.SENT_F, np.float32))
            _maze_launch(entry, d_rows, d_idx, n, goal_xy, reset_xy, 0.25, scaling, fg, fr, d_stage, max_n=len(idx_all))
            want_rows, want = R.maze_reference(want_rows, idx, goal_xy, reset_xy, 0.25, scaling, fg, fr)
            tag = (ng, nr, fg, fr, call)
            got, got_rows = d_stage.get(), d_rows.get()
            assert _same(got[:n], want.astype(np.float32)) and (got[n:] == R.SENT_F).all() and d_stage.intact(), tag
            assert R.rows_equal(got_rows, want_rows) and d_rows.intact(), tag
            same = (want_rows == rows).all(axis=1)      # a world that drew nothing keeps its row word for word
            assert np.array_equal(got_rows[same], rows[same]) and same.sum() >= R.SAMPLER_WORLDS - n, tag
    assert n < 3 or buffered_in > 0


def test_maze_sampler_one_goal_cell_draws_no_integer():
    """n_goal = 1: integers(0, 1) consumes nothing -- with the reset cell fixed as well, a world's stream advances by exactly the four noise draws"""
    n = 65
    rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 70, wide=True, buffered=True), R.sparse_list(n, 3)
    d_rows, d_stage = _put(rows), _put(np.full((n, 4), R.SENT_F, np.float32))
    _maze_launch("device", d_rows, _idx32(idx, _beyond(idx, R.SAMPLER_WORLDS)), n, R.maze_cells(1), R.maze_reset_cells(3), 0.25, 1.0, None, (2.5, 0.5), d_stage)
    got_rows = d_rows.get()
    for k, w in enumerate(idx):
        g = R.rng_from_row(rows[w])
        noise = [g.uniform(-0.25, 0.25) for _ in range(4)]
        assert R.rows_equal(got_rows[w], np.array(R.rng_row(g), dtype=np.uint64)), k
        assert got_rows[w][4] == rows[w][4]      # the buffered half is neither used nor dropped
        assert d_stage.get()[k].tolist() == [np.float32(2.5 + noise[2]), np.float32(0.5 + noise[3]), np.float32(1.5 + noise[0]), np.float32(0.5 + noise[1])], k


@pytest.mark.parametrize("entry", ["device", "list"])
def test_maze_sampler_gives_up_on_a_single_cell(entry):
    """one cell that is the goal cell and the only reset cell: integers(0, 1) draws nothing, so all 65 536 candidates are the goal cell.  The start is NaN and the stream
    has advanced by the four noise draws only."""
    n, cells = 3, R.maze_cells(1)
    rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 90, wide=True, buffered=True), R.sparse_list(n, 5)
    d_rows, d_stage = _put(rows), _put(np.full((n, 4), R.SENT_F, np.float32))
    _maze_launch(entry, d_rows, _idx32(idx, _beyond(idx, R.SAMPLER_WORLDS)), n, cells, cells, 0.25, 1.0, None, None, d_stage, max_n=n)
    want_rows, want = R.maze_reference(rows, idx, cells, cells, 0.25, 1.0)
    got, got_rows = d_stage.get(), d_rows.get()
    assert _same(got, want.astype(np.float32)) and np.isnan(got[:, :2]).all() and not np.isnan(got[:, 2:]).any()
    assert R.rows_equal(got_rows, want_rows) and d_rows.intact() and d_stage.intact()
    for w in idx:
        g = R.rng_from_row(rows[w])
        g.uniform(size=4)
        assert R.rows_equal(got_rows[w], np.array(R.rng_row(g), dtype=np.uint64))


@pytest.mark.parametrize("n", R.UNIFORM_N)
@pytest.mark.parametrize("count", [1, 59, 64])
def test_uniform_rows_are_numpy(count, n):
    """the first n of 300 streams, all of them or those of a mask; two consecutive calls; the rows of unmasked worlds and the streams at and beyond n stay"""
    Nat, L = _lib()
    for masked in (False, True):
        rows = R.stream_rows(R.SAMPLER_WORLDS, 700 + n)
        mask = (np.random.default_rng(n + count).random(n) < 0.5).astype(np.uint8) * 5 if masked else None
        if masked and n > 1:
            mask[0], mask[n - 1] = 0, 5
        worlds = np.arange(n) if mask is None else np.nonzero(mask)[0]
        d_rows, d_out, d_mask = _put(rows), _put(np.full((n, count), R.SENT_F, np.float32)), None if mask is None else _dev(mask)
        want_rows, want_out = rows, np.full((n, count), R.SENT_F, np.float32)
        for call in range(2):
            Nat.check(L.grx_uniform_rows_device(d_rows.ptr, _ptr(d_mask), n, count, d_out.ptr, _stream()))
            _sync()
            want_rows, drawn = R.uniform_reference(want_rows, worlds, count)
            for w, row in drawn.items():
                want_out[w] = row
            _check(dict(out=d_out, rows=d_rows), dict(out=want_out, rows=want_rows), (masked, call))
        assert np.array_equal(d_rows.get()[n:], rows[n:])


# ================================================================================================================== reward kernels
TAIL = 2048 * 256 + 3      # the grid is capped at 2048 workgroups of 256: the last three elements are a second pass of the grid-stride loop
# (What a value test can tell here: a loop that makes no second pass, or strides past the tail.  A stride that is too SHORT -- blockDim.x alone -- still writes every
# element, many times over with the same value: slower, not different.)
BATCHES = (1, 255, TAIL)


@pytest.fixture(scope="module")
def pairs():
    """the pairs of her_refs nearest each threshold, from both sides (computed once): {dim: {thr: (a, b, d)}}"""
    tables = {dim: H.threshold_pairs(dim) for dim in (2, 3)}
    return {dim: {thr: H.nearest_pairs(*tables[dim][thr], thr) for thr in H.PAIR_THRESHOLDS} for dim in (2, 3)}


def _tiled(a, b, batch):
    """`batch` pairs: the table repeated, rotated so that the LAST elements of the batch are pairs from both sides of the threshold"""
    sel = (np.arange(batch) * 4097 + 11) % len(a)      # 4097: consecutive elements alternate between the two halves of the table (beyond / within the threshold)
    return np.ascontiguousarray(a[sel]), np.ascontiguousarray(b[sel])


def _reward_check(got, ag, g, kind, p0, p1, sparse, tag, worst, sel=None, **ignore):
    """sel: (ag, g) is a table and element i of the batch is its pair sel[i] -- the reference is computed once per table row, not once per element"""
    want, _, dist = H.ref_her_outcome(ag, g, kind, p0, p1, sparse, **ignore)
    if sel is not None:
        want, dist = want[sel], (tuple(d[sel] for d in dist) if kind == 3 else dist[sel])
    if sparse and kind != 3:
        assert _same(got, want), tag
        return
    if kind == 3:
        dp, dr = dist
        if sparse:
            clear = (np.abs(dp - p0) > H.MANIP_CLEAR_POS) & (np.abs(dr - p1) > H.MANIP_CLEAR_ROT)
            assert clear.mean() > 0.5 and _same(got[clear], want[clear]) and np.isin(got, [0.0, -1.0]).all(), tag
            return
        err, bound = np.abs(got.astype(np.float64) + (10.0 * dp + dr)), np.full(len(got), H.MANIP_DENSE_ATOL)
    elif kind == 2:
        err, bound = np.abs(got.astype(np.float64) - np.exp(-dist)), H.maze_dense_bound(dist)
    else:
        err, bound = np.abs(got.astype(np.float64) + dist), H.dense_bound(dist)
    ratio = float((err / bound).max())
    worst.append((tag, ratio))
    print(f"dense reward {tag}: worst error / bound = {ratio:.3f}")
    assert (err <= bound).all(), (tag, ratio)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("entry", ["fetch", "goal3", "goal15", "maze"])
def test_reward_kernels_at_the_threshold_distance(entry, batch, pairs):
    """sparse: bit-exact on pairs whose fp64 distance lies within a few float32 ulps of the threshold, on either side; dense: within the bounds of her_refs"""
    Nat, L = _lib()
    worst = []
    for thr in H.PAIR_THRESHOLDS:
        a, b, _ = pairs[2 if entry == "maze" else 3][thr]
        a, b = _tiled(a, b, batch)
        if entry == "goal15":      # five 3-vectors of which four agree: the same distances on 15-vectors
            pad = np.random.default_rng(batch).uniform(-1, 1, (len(a), 12)).astype(np.float32)
            a, b = np.ascontiguousarray(np.concatenate([pad[:, :6], a, pad[:, 6:]], axis=1)), np.ascontiguousarray(np.concatenate([pad[:, :6], b, pad[:, 6:]], axis=1))
        d_a, d_b = _dev(a), _dev(b)
        for sparse in (1, 0):
            out = _put(np.full(batch, R.SENT_F, np.float32))
            if entry == "fetch":
                Nat.check(L.grx_fetch_compute_reward(d_a.data_ptr(), d_b.data_ptr(), batch, thr, sparse, out.ptr, _stream()))
            elif entry == "maze":
                Nat.check(L.grx_maze_compute_reward(d_a.data_ptr(), d_b.data_ptr(), batch, thr, sparse, out.ptr, _stream()))
            else:
                Nat.check(L.grx_goal_compute_reward(d_a.data_ptr(), d_b.data_ptr(), batch, a.shape[1], thr, sparse, out.ptr, _stream()))
            _sync()
            got = out.get()
            assert out.intact() and not (got == np.float32(R.SENT_F)).any(), (entry, thr, sparse)      # every element was written, the tail's three too
            _reward_check(got, a, b, {"fetch": 0, "goal3": 1, "goal15": 1, "maze": 2}[entry], thr, 0.0, sparse, (entry, batch, thr), worst)
            if sparse and batch > 1:
                assert len(np.unique(got)) == 2 and len(np.unique(got[-3:])) == 2      # both outcomes, in the second pass too


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("ignore", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)])
def test_manip_reward_kernel(ignore, batch):
    """7-vector pose goals with each ignore_* flag; sparse rewards are exact for the pairs that are clear of both thresholds (her_refs.MANIP_CLEAR_*)"""
    Nat, L = _lib()
    rng = np.random.default_rng(batch + 7 * sum(ignore))
    worst = []

    def poses(n):
        q = rng.standard_normal((n, 4))
        return np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)) + [1.0, 0.87, 0.2], q / np.linalg.norm(q, axis=1, keepdims=True)], axis=1).astype(np.float32)

    base = poses(4096)
    near = base.copy()      # half of the pairs: a small offset and a small rotation away, on both sides of the thresholds 0.01 m / 0.1 rad
    near[:, :3] += rng.uniform(-0.012, 0.012, (4096, 3)).astype(np.float32)
    dq = np.concatenate([np.ones((4096, 1)), rng.uniform(-0.06, 0.06, (4096, 3))], axis=1)
    w0, v0, w1, v1 = base[:, 3:4], base[:, 4:], dq[:, :1], dq[:, 1:]
    qn = np.concatenate([w0 * w1 - (v0 * v1).sum(1, keepdims=True), w0 * v1 + w1 * v0 + np.cross(v0, v1)], axis=1)
    near[:, 3:] = (qn / np.linalg.norm(qn, axis=1, keepdims=True)).astype(np.float32)
    other = poses(4096)
    other[::2] = near[::2]
    sel = (np.arange(batch) * 4097 + 11) % 4096
    a, b = np.ascontiguousarray(base[sel]), np.ascontiguousarray(other[sel])
    d_a, d_b = _dev(a), _dev(b)
    ip, ir, iz = ignore
    for sparse in (1, 0):
        out = _put(np.full(batch, R.SENT_F, np.float32))
        Nat.check(L.grx_manip_compute_reward(d_a.data_ptr(), d_b.data_ptr(), batch, ip, ir, iz, 0.01, 0.1, sparse, out.ptr, _stream()))
        _sync()
        got = out.get()
        assert out.intact() and not (got == np.float32(R.SENT_F)).any(), (ignore, sparse)
        _reward_check(got, base, other, 3, float(np.float32(0.01)), float(np.float32(0.1)), sparse, ("manip", ignore, batch), worst, sel=sel, ignore_pos=ip, ignore_rot=ir, ignore_z=iz)
