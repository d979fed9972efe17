"""The plain references of tests/reset_refs.py, checked without a GPU before a device is compared with them: the samplers against the pinned host routines
(fetch.sample_fetch_reset, adroit_spec.sample_reset, maze_spec.sample_maze_reset) bit for bit, the kitchen reference against examples worked out by hand, the host
twins grx_fetch_sample_resets / grx_sample_uniform_rows against the references at the GPU file's case tables, the ctypes mirrors of four argument blocks against a C
compiler's view of include/grx_capi.h, and every deliberate mistake of the references shown to answer differently from the correct one on the GPU file's tables."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import reset_refs as R
from bookkeeping_refs import rng_from_row, rng_row

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else (a.view(np.int64) if a.dtype == np.float64 else a)


def _same(a, b):
    return (a is None and b is None) or (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)))


def _dicts_same(a, b):
    return all(_same(a[f], b[f]) for f in a)


# ------------------------------------------------------------------------------------------------------------------ references against the pinned host routines
def _gens(n, seed):
    gens = [np.random.Generator(np.random.PCG64(seed + i)) for i in range(n)]
    for i, g in enumerate(gens):
        g.uniform(size=i % 4)
    return gens


def test_fetch_reference_equals_sample_fetch_reset():
    from gymnasium_robotics_amd.envs.fetch import sample_fetch_reset

    for c in R.fetch_cfgs():
        cfg = dict(has_object=c["has_object"], target_in_the_air=c["in_air"], obj_range=c["obj_range"], target_range=c["target_range"], target_offset=np.array(R.FETCH_OFFSET))
        gens = _gens(300, 40)
        rows = np.array([rng_row(g)[:4] for g in gens], dtype=np.uint64)
        for episode in range(2):      # the second reset continues the streams
            rows, got = R.fetch_reference(rows, np.arange(300), c)
            for i, g in enumerate(gens):
                oxy, goal = sample_fetch_reset(cfg, g, np.array(R.FETCH_GRIPPER), R.FETCH_HEIGHT)
                assert np.array_equal(got[i, 2:], goal), (c, i)
                assert np.array_equal(got[i, :2], oxy if c["has_object"] else R.FETCH_GRIPPER[:2]), (c, i)
                assert rng_row(g)[:4] == [int(x) for x in rows[i]], (c, i)


def test_adroit_reference_equals_adroit_spec_sample_reset():
    from gymnasium_robotics_amd.envs.adroit_spec import sample_reset

    model = types.SimpleNamespace(info={"shift_pos0": list(R.ADROIT_POS0)})
    for kind, task in ((0, "hammer"), (1, "door"), (3, "relocate")):
        gens = _gens(200, 60 + kind)
        current = np.random.default_rng(kind).uniform(-0.4, 0.4, (200, 3))
        for i, g in enumerate(gens):
            h = rng_from_row(rng_row(g))
            want = sample_reset(task, g, model, current=current[i])
            e, t, s = R.adroit_sample(h, kind, current[i], R.ADROIT_POS0)
            assert np.array_equal(np.array(e), want["edit"]) and np.array_equal(s, want["shift"].astype(np.float32)), (task, i)
            assert (t is None and want["target"] is None) or np.array_equal(np.array(t), want["target"]), (task, i)
            assert rng_row(h) == rng_row(g), (task, i)
            if kind == 0:
                assert e[:2] == list(current[i, :2])      # the kept components
            if kind == 3:
                assert e[2] == current[i, 2]


TINY_MAP = [[1, 1, 1, 1, 1, 1], [1, "g", 0, "r", "c", 1], [1, "c", 1, 0, "g", 1], [1, "r", "c", 0, "r", 1], [1, 1, 1, 1, 1, 1]]


def test_maze_reference_equals_maze_spec_sample_maze_reset():
    from gymnasium_robotics_amd.envs import maze_spec

    cell = {"g": maze_spec.G, "r": maze_spec.R, "c": maze_spec.C}
    maze = maze_spec.Maze([[cell.get(v, v) for v in row] for row in TINY_MAP], 2.0, 0.5)
    goal_xy, reset_xy = np.array(maze.unique_goal_locations), np.array(maze.unique_reset_locations)
    assert len(goal_xy) == 5 and len(reset_xy) == 6
    for options in ({}, {"goal_cell": (1, 2)}, {"reset_cell": (3, 3)}, {"goal_cell": (2, 3), "reset_cell": (1, 1)}):
        fg = maze.cell_rowcol_to_xy(options["goal_cell"]) if "goal_cell" in options else None
        fr = maze.cell_rowcol_to_xy(options["reset_cell"]) if "reset_cell" in options else None
        gens = _gens(200, 80)
        for g in gens[::3]:
            g.integers(0, 3)      # a buffered half on entry
        for i, g in enumerate(gens):
            h = rng_from_row(rng_row(g))
            goal, start = maze_spec.sample_maze_reset(maze, g, 0.25, options)
            got = R.maze_sample(h, goal_xy, reset_xy, 0.25, 2.0, fg, fr)
            assert got == [start[0], start[1], goal[0], goal[1]], (options, i)
            assert rng_row(h) == rng_row(g), (options, i)


def test_uniform_reference_is_generator_uniform():
    g, h = np.random.Generator(np.random.PCG64(4)), np.random.Generator(np.random.PCG64(4))
    assert np.array_equal(R.uniform_row(g, 59), h.uniform(-1.0, 1.0, 59).astype(np.float32)) and rng_row(g) == rng_row(h)


def test_sampler_guards():
    """obj_range 0.05 never clears the 0.1 m ring: NaN object words, the goal drawn after 131 072 outputs; one maze cell that is goal and reset cell: NaN start, the
    stream advanced by the four noise draws only (integers(0, 1) draws nothing)"""
    g, h = np.random.Generator(np.random.PCG64(9)), np.random.Generator(np.random.PCG64(9))
    got = R.fetch_sample(g, 1, 0, 0.05, 0.15, R.FETCH_OFFSET, R.FETCH_GRIPPER, R.FETCH_HEIGHT)
    h.bit_generator.advance(2 * R.GUARD_DRAWS)
    want = [R.FETCH_GRIPPER[e] + h.uniform(-0.15, 0.15) + R.FETCH_OFFSET[e] for e in range(3)]
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2:4] == want[:2] and got[4] == R.FETCH_HEIGHT and rng_row(g) == rng_row(h)
    cells = R.maze_cells(1)
    g, h = np.random.Generator(np.random.PCG64(9)), np.random.Generator(np.random.PCG64(9))
    got = R.maze_sample(g, cells, cells, 0.25, 1.0)
    n = [h.uniform(-0.25, 0.25) for _ in range(4)]
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2:] == [cells[0, 0] + n[0], cells[0, 1] + n[1]] and rng_row(g) == rng_row(h)


# ------------------------------------------------------------------------------------------------------------------ kitchen, by hand
def _kitchen_state(ttc, epi, el, needs):
    n = len(ttc)
    return dict(tasks_to_complete=np.array(ttc, np.int32), episode_completions=np.array(epi, np.int32), elapsed=np.array(el, np.int32), step_completions=np.full(n, -77, np.int32),
                reward=np.full(n, -5.0, np.float32), terminated=np.full(n, 9, np.uint8), truncated=np.full(n, 9, np.uint8), needs_reset=np.array(needs, np.uint8),
                reset_now=np.full(n, 9, np.uint8), qpos=np.full((n, 3), 7.0, np.float32), qvel=np.full((n, 2), 7.0, np.float32), qacc_ws=np.full((n, 2), 7.0, np.float32),
                final_info=np.full((n, 3), -77, np.int32))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_kitchen_reference_by_hand(mode):
    """four worlds of a two-task episode (bits 1 and 3), remove and terminate on, limit 3: world 0 completes its last open task (bit 3, with a foreign bit 2 set), world 1
    completes bit 1 and stays open, world 2 reaches the limit with nothing completed, world 3 is pending (mode 1) / was not stepped (modes 0, 2)"""
    cfg = dict(nq=3, nv=2, all_mask=0b1010, max_steps=3, remove_when_completed=1, terminate_when_completed=1, mode=mode)
    st = _kitchen_state(ttc=[0b1000, 0b1010, 0b1010, 0b0010], epi=[0b0010, 0, 0, 0b1000], el=[1, 0, 2, 3], needs=[0, 0, 0, 1] if mode == 1 else [5, 5, 5, 5])
    init = np.array([1.0, 2.0, 3.0], np.float32)
    o = R.kitchen_bookkeeping(st, cfg, completed=[0b1100, 0b0110, 0b0101, 0b0010], stepped=[1, 1, 1, 0], init_qpos=init)
    assert o["reward"].tolist() == [1.0, 1.0, 0.0, 0.0] and o["terminated"].tolist() == [1, 0, 0, 0] and o["truncated"].tolist() == [0, 0, 1, 0]
    rewound = {0: [], 1: [3], 2: [0, 2]}[mode]
    assert o["reset_now"].tolist() == [int(w in rewound) for w in range(4)]
    for w in range(4):
        assert o["qpos"][w].tolist() == (init.tolist() if w in rewound else [7.0] * 3) and o["qvel"][w].tolist() == ([0.0, 0.0] if w in rewound else [7.0, 7.0])
        assert o["qacc_ws"][w].tolist() == o["qvel"][w].tolist()
    if mode == 0:
        assert o["tasks_to_complete"].tolist() == [0, 0b1000, 0b1010, 0b0010] and o["episode_completions"].tolist() == [0b1010, 0b0010, 0, 0b1000]
        assert o["elapsed"].tolist() == [2, 1, 3, 3] and o["step_completions"].tolist() == [0b1000, 0b0010, 0, 0] and o["needs_reset"].tolist() == [5, 5, 5, 5]
        assert (o["final_info"] == -77).all()
    if mode == 1:
        assert o["tasks_to_complete"].tolist() == [0, 0b1000, 0b1010, 0b1010] and o["episode_completions"].tolist() == [0b1010, 0b0010, 0, 0]
        assert o["elapsed"].tolist() == [2, 1, 3, 0] and o["step_completions"].tolist() == [0b1000, 0b0010, 0, 0] and o["needs_reset"].tolist() == [1, 0, 1, 0]
        assert (o["final_info"] == -77).all()
    if mode == 2:
        assert o["tasks_to_complete"].tolist() == [0b1010, 0b1000, 0b1010, 0b0010] and o["episode_completions"].tolist() == [0, 0b0010, 0, 0b1000]
        assert o["elapsed"].tolist() == [0, 1, 0, 3] and o["step_completions"].tolist() == [0, 0b0010, 0, 0] and o["needs_reset"].tolist() == [5, 5, 5, 5]
        assert o["final_info"].tolist() == [[0, 0b1000, 0b1010], [-77] * 3, [0b1010, 0, 0], [-77] * 3]


# ------------------------------------------------------------------------------------------------------------------ host twins at the GPU file's tables
def _native():
    from gymnasium_robotics_amd import _native

    return _native.lib()


@pytest.mark.parametrize("n", R.SAMPLER_N)
def test_host_fetch_sampler_is_the_reference(n):
    L = _native()
    for c in R.fetch_cfgs():
        rows = R.stream_rows(R.SAMPLER_WORLDS, 500 + n)
        idx = R.sparse_list(n, n)
        st = rows.copy()
        toff, g0 = np.array(R.FETCH_OFFSET, np.float64), np.array(R.FETCH_GRIPPER, np.float64)
        want_rows = rows
        for call in range(2):
            oxy, goal = np.full((n, 2), R.SENT_F), np.full((n, 3), R.SENT_F)
            assert L.grx_fetch_sample_resets(st.ctypes.data, idx.ctypes.data, n, c["has_object"], c["in_air"], c["obj_range"], c["target_range"], toff.ctypes.data,
                                             g0.ctypes.data, R.FETCH_HEIGHT, oxy.ctypes.data, goal.ctypes.data) == 0
            want_rows, want = R.fetch_reference(want_rows, idx, c, guard=False)
            assert np.array_equal(goal, want[:, 2:]) and np.array_equal(st, want_rows), (c, call)
            assert np.array_equal(oxy, want[:, :2]) if c["has_object"] else (oxy == R.SENT_F).all(), (c, call)
        rest = np.setdiff1d(np.arange(R.SAMPLER_WORLDS), idx)
        assert np.array_equal(st[rest], rows[rest]) and not (st[idx] == rows[idx]).all(axis=1).any()


@pytest.mark.parametrize("n", R.UNIFORM_N)
@pytest.mark.parametrize("count", [1, 59, 64])
def test_host_uniform_rows_are_the_reference(count, n):
    L = _native()
    rows = R.stream_rows(R.SAMPLER_WORLDS, 700 + n)
    for idx in (None, R.sparse_list(min(n, R.SAMPLER_WORLDS), n + count)):
        st, want_rows = rows.copy(), rows
        worlds = np.arange(n) if idx is None else idx
        for call in range(2):
            out = np.full((len(worlds) + 1, count), R.SENT_F, np.float32)
            assert L.grx_sample_uniform_rows(st.ctypes.data, None if idx is None else idx.ctypes.data, len(worlds), count, out.ctypes.data) == 0
            want_rows, want = R.uniform_reference(want_rows, worlds, count)
            assert _same(out[:-1], np.array([want[int(w)] for w in worlds])) and (out[-1] == R.SENT_F).all() and np.array_equal(st, want_rows), (idx is None, call)
        rest = np.setdiff1d(np.arange(R.SAMPLER_WORLDS), worlds)
        assert np.array_equal(st[rest], rows[rest])


# ------------------------------------------------------------------------------------------------------------------ the ctypes mirrors
STRUCTS = {      # header struct -> (ctypes mirror, the header's fields in order)
    "grx_kitchen_book": ("KitchenBookStruct", "completed stepped tasks_to_complete episode_completions elapsed step_completions reward terminated truncated needs_reset reset_now "
                         "qpos qvel qacc_ws init_qpos nq nv all_mask max_steps remove_when_completed terminate_when_completed mode final_info"),
    "grx_hand_commit_args": ("HandCommitArgsStruct", "idx k nq nv obs_dim goal_dim s_qpos s_qvel s_qacc_ws s_obs s_achieved s_palm s_goal s_packed s_status qpos qvel qacc_ws obs "
                             "achieved palm goal packed status"),
    "grx_adroit_commit_args": ("AdroitCommitArgsStruct", "idx k nq nv obs_dim s_qpos s_qvel s_qacc_ws s_shift s_target s_obs s_status qpos qvel qacc_ws shift target obs status"),
    "grx_maze_reset_args": ("MazeResetArgsStruct", "idx stage qpos0 nq nv obs_dim obs_skip goal_radius keep_outcome qpos qvel qacc_ws goal obs achieved reward success packed"),
}


def test_argument_structs_mirror_the_header(tmp_path):
    from gymnasium_robotics_amd import _native

    for cname, (pyname, fields) in STRUCTS.items():
        assert [n for n, _ in getattr(_native, pyname)._fields_] == fields.split(), cname
    # hand counts on an LP64 target: 15 pointers + 7 ints (+ 4 padding) + 1 pointer; pointer + 5 ints (+ 4) + 18 pointers; pointer + 4 ints + 14 pointers;
    # 3 pointers + 4 ints + double + int (+ 4) + 9 pointers
    sizes = {"KitchenBookStruct": 15 * 8 + 7 * 4 + 4 + 8, "HandCommitArgsStruct": 8 + 5 * 4 + 4 + 18 * 8, "AdroitCommitArgsStruct": 8 + 4 * 4 + 14 * 8,
             "MazeResetArgsStruct": 3 * 8 + 4 * 4 + 8 + 4 + 4 + 9 * 8}
    for pyname, size in sizes.items():
        assert ctypes.sizeof(getattr(_native, pyname)) == size, pyname
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:      # the hand counts above stand alone
        return
    lines = []
    for cname, (_, fields) in STRUCTS.items():
        lines.append(f'  printf("%zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f}));' for f in fields.split()]
        lines.append('  printf("\\n");')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "grx_capi.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for (cname, (pyname, fields)), row in zip(STRUCTS.items(), got):
        S = getattr(_native, pyname)
        assert row == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields.split()], cname


# ------------------------------------------------------------------------------------------------------------------ deliberate mistakes
@pytest.mark.parametrize("mistake", R.KITCHEN_MISTAKES)
def test_kitchen_mistakes_are_caught_by_the_table(mistake):
    """the fields in which the mistaken copy differs from the reference somewhere on the table (N = 257 and 1 suffice), and the modes in which it does"""
    where = set()
    for N in (1, 257):
        for mode in (0, 1, 2):
            for chain in R.kitchen_chains(N, mode):
                good, bad = R.kitchen_walk(chain), R.kitchen_walk(chain, mistake)
                where |= {(mode, f) for g, b in zip(good, bad) for f in R.KITCHEN_FIELDS if not _same(g[f], b[f])}
    fields = {f for _, f in where}
    expect = dict(el_gt="truncated", term_unstepped="terminated", pending_reward="reward", step_completions_kept="step_completions", needs_reset_kept="needs_reset",
                  final_info_mode1="final_info")[mistake]
    assert expect in fields, (mistake, where)


def test_kitchen_table_reaches_every_rule():
    seen = dict(pending=0, term=0, trunc=0, unstepped=0, both=0, foreign=0)
    for mode in (0, 1, 2):
        for chain in R.kitchen_chains(257, mode):
            cfg, kind, _, state, calls = chain
            prev = state
            for (completed, stepped), out in zip(calls, R.kitchen_walk(chain)):
                seen["pending"] += int(mode == 1 and prev["needs_reset"].any())
                seen["term"] += int(out["terminated"].any()); seen["trunc"] += int(out["truncated"].any()); seen["both"] += int((out["terminated"] & out["truncated"]).any())
                seen["unstepped"] += int(stepped is not None and (stepped == 0).any())
                seen["foreign"] += int((completed & ~cfg["all_mask"]).any())
                prev = out
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("mistake", R.HAND_MISTAKES)
def test_hand_commit_mistakes_are_caught_by_the_table(mistake):
    caught = 0
    for dims in R.HAND_DIMS:
        for call, idx in enumerate(R.commit_lists()):
            live, staged = R.hand_case(dims, call)
            caught += not _dicts_same(R.hand_commit(live, staged, idx, len(idx), dims[2], dims[3]), R.hand_commit(live, staged, idx, len(idx), dims[2], dims[3], mistake=mistake))
    assert caught == 3 * len(R.HAND_DIMS) if mistake != "by_world" else caught >= 2 * len(R.HAND_DIMS), caught


@pytest.mark.parametrize("mistake", R.ADROIT_MISTAKES)
def test_adroit_commit_mistakes_are_caught_by_the_table(mistake):
    for dims in R.ADROIT_DIMS:
        for call, idx in enumerate(R.commit_lists()[1:]):
            live, staged = R.adroit_case(dims, call, pairs=call % 2 == 0)
            assert not _same(R.adroit_commit(live, staged, idx, len(idx))["status"], R.adroit_commit(live, staged, idx, len(idx), mistake=mistake)["status"]), (dims, call)


def test_status_merges_by_hand():
    """the two merges on one pair of words: old = sticky 0x8002 | low 0x25, staged = sticky 0x0011 | low 0x36"""
    old, staged = R.as_int32(0x80020025), 0x00110036
    assert R.hand_status(old, staged) & 0xFFFFFFFF == 0x80130025      # the staged sticky half joins, the low half stays
    assert R.adroit_status(old, staged) & 0xFFFFFFFF == 0x80060006    # the staged low four bits replace the low half and join the sticky half; its bits 4, 5 and 16+ are dropped
    pairs = {(int(o) & 15, int(s) & 15) for call in range(4) for o, s in zip(*R.status_words(call, np.random.default_rng(call)))}
    assert len(pairs) == 256


@pytest.mark.parametrize("mistake", R.MAZE_ROW_MISTAKES)
def test_maze_row_mistakes_are_caught_by_the_table(mistake):
    caught = []
    for dims in R.MAZE_ROW_DIMS:
        for keep in (0, 1):
            for packed in (0, 1):
                live, idx, k, stage, qpos0, radius = R.maze_row_case(dims, keep, packed, 0)
                args = (live, idx, k, stage, qpos0, dims[0], dims[1], dims[2], radius, keep)
                if not _dicts_same(R.maze_reset_rows(*args), R.maze_reset_rows(*args, mistake=mistake)):
                    caught.append((dims, keep, packed))
    want = {"skip_ignored": lambda c: c[0][2] > 0, "radius_lt": lambda c: True, "reward_zeroed": lambda c: c[1] == 1}[mistake]
    assert caught == [(d, k, p) for d in R.MAZE_ROW_DIMS for k in (0, 1) for p in (0, 1) if want((d, k, p))], caught


def test_maze_stage_rows_sit_at_the_radius():
    for radius in (R.RADIUS_A, R.RADIUS_B):
        s = R.maze_stage(17, radius, np.random.default_rng(0)).astype(np.float64)
        d = np.hypot(s[:, 0] - s[:, 2], s[:, 1] - s[:, 3])
        assert (d == radius).sum() >= 2 and ((d < radius) & (d > radius * (1 - 3e-7))).sum() >= 2 and ((d > radius) & (d < radius * (1 + 3e-7))).sum() >= 2


@pytest.mark.parametrize("mistake", R.FETCH_MISTAKES)
def test_fetch_sampler_mistakes_are_caught_by_the_table(mistake):
    caught = {}
    for c in R.fetch_cfgs():
        rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 565), R.sparse_list(65, 65)
        (r0, s0), (r1, s1) = R.fetch_reference(rows, idx, c), R.fetch_reference(rows, idx, c, mistake=mistake)
        caught[(c["has_object"], c["in_air"])] = not (np.array_equal(s0.astype(np.float32), s1.astype(np.float32)) and np.array_equal(r0, r1))
    assert caught[(1, 1)] and (mistake == "air_unconditional" or caught[(1, 0)]), caught


@pytest.mark.parametrize("mistake, kind", [("door_swapped", 1), ("target_first", 3)])
def test_adroit_sampler_mistakes_are_caught_by_the_table(mistake, kind):
    rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 565), R.sparse_list(65, 65)
    bufs = dict(edit=np.random.default_rng(0).uniform(-1, 1, (R.SAMPLER_WORLDS, 3)), target64=np.zeros((R.SAMPLER_WORLDS, 3)), shift=np.zeros((R.SAMPLER_WORLDS, 7), np.float32),
                target=np.zeros((R.SAMPLER_WORLDS, 3), np.float32))
    (_, good), (_, bad) = R.adroit_reference(rows, idx, kind, bufs), R.adroit_reference(rows, idx, kind, bufs, mistake=mistake)
    assert not _same(good["shift"], bad["shift"]) and not _same(good["edit"], bad["edit"])
    assert kind != 3 or not _same(good["target"], bad["target"])


@pytest.mark.parametrize("mistake", R.MAZE_SAMPLE_MISTAKES)
def test_maze_sampler_mistakes_are_caught_by_the_table(mistake):
    caught = {}
    for n_goal, n_reset in ((1, 3), (3, 1), (7, 8), (2, 2)):
        rows, idx = R.stream_rows(R.SAMPLER_WORLDS, 565, wide=True, buffered=True), R.sparse_list(65, 65)
        args = (rows, idx, R.maze_cells(n_goal), R.maze_reset_cells(n_reset), 0.25, 1.0)
        (r0, s0), (r1, s1) = R.maze_reference(*args), R.maze_reference(*args, mistake=mistake)
        caught[(n_goal, n_reset)] = not (np.array_equal(s0.astype(np.float32), s1.astype(np.float32)) and R.rows_equal(r0, r1))
    assert (caught[(1, 3)] and caught[(3, 1)]) if mistake == "integers_1_draws" else (caught[(7, 8)] and caught[(2, 2)]), caught
