"""The plain references of tests/bookkeeping_refs.py, checked without a GPU before a device is compared with them: ref_order against every assertion the two order tests of
tests/test_gpu_api.py make of the device (same inputs), the redraw of ref_maze_episode_end against maze_spec.redraw_goal draw for draw, its 65 536-rejection guard, and the
ctypes mirror of grx_maze_episode_args against the size a C compiler gives the header's struct."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import bookkeeping_refs as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------------------------------------------------------------ order
def test_ref_order_places_three_cheap_worlds_on_the_slots_that_run_three():
    """the inputs and assertions of test_gpu_api.py::test_order_by_cost_slots_places_three_cheap_worlds_on_the_slots_that_run_three"""
    n, per, slots = 4096, 512, 256
    rng = np.random.default_rng(3)
    cost = rng.integers(1000, 1400, n).astype(np.int32)
    strag = {s: rng.choice(per, size=3 + (s % 3), replace=False) + s * per for s in range(8)}
    for s in range(8):
        cost[strag[s]] = rng.integers(2900, 3400, len(strag[s]))
    P, T_ = R.ref_order(cost, None, n, 0).reshape(per, 8), R.ref_order(cost, None, n, slots).reshape(per, 8)
    for s in range(8):
        d, t = P[:, s], T_[:, s]
        assert sorted(t.tolist()) == sorted(d.tolist()) == list(range(s * per, (s + 1) * per))
        M = len(strag[s])
        assert R.placement_m(R.order_keys(cost)[s * per:(s + 1) * per], slots) == M
        assert set(d[:M].tolist()) == set(strag[s].tolist())
        assert (t[:slots - M] == d[:slots - M]).all()
        assert (t[slots - M:slots] == d[per - M:]).all()
        assert (t[slots:slots + M] == d[per - 2 * M:per - M]).all()
        assert (t[slots + M:per - M] == d[slots - M:per - 3 * M]).all()
        assert (t[per - M:] == d[per - 3 * M:per - 2 * M]).all()
    n2 = 8192      # three rounds and more: the plain order
    c2 = rng.integers(1000, 4000, n2).astype(np.int32)
    assert np.array_equal(R.ref_order(c2, None, n2, 0), R.ref_order(c2, None, n2, slots))


def test_ref_order_is_decreasing_cost_per_slice_ties_by_world():
    """the assertions of test_gpu_api.py::test_order_by_cost_and_balance_invariance on its kind of input (2048 worlds, costs below 5000, many ties), and the moving average"""
    n = 2048
    c = np.random.default_rng(0).integers(0, 5000, n).astype(np.int32)
    o = R.ref_order(c, None, n, 0).reshape(n // 8, 8)
    assert sorted(o.ravel().tolist()) == list(range(n))
    per = n // 8
    for s in range(8):
        w = o[:, s]
        assert (w // per == s).all()
        key = np.stack([-c[w].astype(np.int64), w.astype(np.int64)], axis=1)
        assert (np.lexsort((key[:, 1], key[:, 0])) == np.arange(per)).all()
    ema = R.ref_ema(c, np.full(n, 100.0), 0.25)
    assert np.allclose(ema, 75.0 + 0.25 * c, rtol=1e-6)
    # the order on a returned average is the order of those values
    e32 = ema.astype(np.float32)
    o2 = R.ref_order(c, e32, n, 0)
    assert all((np.diff(e32[o2[s::8]]) <= 0).all() for s in range(8))


def test_ref_order_keys_clamp_and_tie():
    c = np.array([0, -5, -2147483648, 250000001, 2147483647, 1, 250000000, 249999984], np.int32)
    k = R.order_keys(c)
    assert k.tolist() == [0, 0, 0, 4000000000, 4000000000, 16, 4000000000, 3999999744]
    o = R.ref_order(np.tile(c, 8), None, 64, 0).reshape(8, 8)
    assert (o[:, 0] == [3, 4, 6, 7, 5, 0, 1, 2]).all()      # the clamped keys tie: the lower world first


def test_ulps_apart():
    x = np.float32(1000.0)
    assert R.ulps_apart(np.nextafter(x, np.float32(2000)), 1000.0) == 1.0 and R.ulps_apart(x, 1000.0) == 0.0


# ------------------------------------------------------------------------------------------------------------------ redraw
def _maze():
    from gymnasium_robotics_amd.envs.maze_spec import MAPS, Maze

    return Maze(MAPS["Large_Diverse_G"], 1.0, 0.5)


def _state(n, goal, achieved, rows, success=None):
    return dict(elapsed=np.zeros(n, np.int64), needs_reset=np.zeros(n, np.uint8), success=np.ones(n, np.uint8) if success is None else success, achieved=achieved, goal=goal,
                status=np.zeros(n, np.int32), packed=None, rng=rows)


def test_redraw_equals_maze_spec_redraw_goal_bit_for_bit():
    from gymnasium_robotics_amd.envs.maze_spec import GOAL_RADIUS, redraw_goal

    maze = _maze()
    cells = np.array(maze.unique_goal_locations)
    assert len(cells) > 2
    n = 200
    rng = np.random.default_rng(11)
    gens = [np.random.Generator(np.random.PCG64(900 + i)) for i in range(n)]
    for g in gens[::2]:
        g.integers(0, 3)      # leaves a buffered 32-bit half
    assert sum(g.bit_generator.state["has_uint32"] for g in gens) == n // 2
    rows = np.array([R.rng_row(g) for g in gens], dtype=np.uint64)
    goal = (cells[rng.integers(0, len(cells), n)] + rng.uniform(-0.25, 0.25, (n, 2))).astype(np.float32)
    achieved = (goal + rng.uniform(-0.2, 0.2, (n, 2)).astype(np.float32)).astype(np.float32)      # every world within the radius of its goal
    cfg = dict(mode=2, limit=0, continuing_task=1, reset_target=1, goal_xy=cells, noise_range=0.25, scaling=maze.maze_size_scaling, goal_radius=GOAL_RADIUS)
    out = R.ref_maze_episode_end(_state(n, goal, achieved, rows), cfg)
    moved = 0
    for w in range(n):
        want = redraw_goal(maze, gens[w], achieved[w], goal[w], 0.25)
        assert np.array_equal(out["goal"][w], want.astype(np.float32)), w
        assert R.rng_rows_equal(out["rng"][w], np.array(R.rng_row(gens[w]), dtype=np.uint64)), w      # the stream ends where redraw_goal's does
        moved += not np.array_equal(out["goal"][w], goal[w])
    assert moved == n and not out["status"].any()
    # a world that did not succeed, and one that is pending, draw nothing
    st = _state(n, goal, achieved, rows, success=np.zeros(n, np.uint8))
    out0 = R.ref_maze_episode_end(st, cfg)
    assert np.array_equal(out0["rng"], rows) and np.array_equal(out0["goal"], goal)


def test_redraw_guard_after_65536_rejections():
    """two goal cells, the agent within the radius of both, no noise: every draw is rejected.  The goal stays, the world is flagged in both halves of its status word and the
    stream has advanced by exactly 65 536 integers and 131 072 uniform draws.  (The reference walks them in about 0.4 s, the replay below in as much again.)"""
    cells = np.array([[0.0, 0.0], [0.1, 0.0]])
    gen = np.random.Generator(np.random.PCG64(5))
    rows = np.array([R.rng_row(gen)], dtype=np.uint64)
    goal, achieved = np.array([[0.02, 0.01]], np.float32), np.array([[0.05, 0.0]], np.float32)
    cfg = dict(mode=2, limit=0, continuing_task=1, reset_target=1, goal_xy=cells, noise_range=0.0, scaling=1.0, goal_radius=0.45)
    st = _state(1, goal, achieved, rows)
    st["status"][0] = 4 << 16
    out = R.ref_maze_episode_end(st, cfg)
    assert np.array_equal(out["goal"], goal) and out["status"][0] == (4 << 16 | 1 << 16 | 1)
    for _ in range(65536):
        gen.integers(0, 2); gen.uniform(-0.0, 0.0); gen.uniform(-0.0, 0.0)
    assert R.rng_rows_equal(out["rng"][0], np.array(R.rng_row(gen), dtype=np.uint64))
    assert not R.rng_rows_equal(out["rng"][0], rows[0])


def test_rng_row_round_trip_and_buffer_flag():
    g = np.random.Generator(np.random.PCG64(3))
    g.integers(0, 3)
    row = R.rng_row(g)
    assert row[4] >> 32 == 1
    h = R.rng_from_row(row)
    assert [int(g.integers(0, 1000)) for _ in range(5)] == [int(h.integers(0, 1000)) for _ in range(5)] and g.uniform() == h.uniform()
    a = np.array(row, dtype=np.uint64); b = a.copy()
    b[4] = 7      # a consumed buffer's stale value is not state ...
    a[4] = 9
    assert R.rng_rows_equal(a, b)
    b[4] = (1 << 32) | 7      # ... a live one is
    assert not R.rng_rows_equal(a, b)


def test_episode_end_rules_by_hand():
    """one world per rule of the header comment, mode by mode"""
    z = lambda n, dt: np.zeros(n, dt)
    st = dict(elapsed=np.array([3, 4, 1 << 33, 4, 0], np.int64), needs_reset=np.array([0, 0, 0, 1, 0], np.uint8), success=np.array([0, 0, 1, 1, 1], np.uint8),
              achieved=np.zeros((5, 2), np.float32), goal=np.ones((5, 2), np.float32), status=z(5, np.int32), packed=np.arange(15, dtype=np.float32).reshape(5, 3), rng=None)
    cfg = dict(mode=0, limit=5, continuing_task=0, reset_target=0, goal_xy=None, noise_range=0.0, scaling=1.0, goal_radius=0.45)
    o = R.ref_maze_episode_end(st, cfg)
    assert o["elapsed"].tolist() == [4, 5, (1 << 33) + 1, 0, 1] and o["terminated"].tolist() == [0, 0, 1, 0, 1] and o["truncated"].tolist() == [0, 1, 1, 0, 0]
    assert o["reset_idx"].tolist() == [3] and o["needs_reset"].tolist() == [0, 1, 1, 0, 1] and o["mask"].tolist() == [1, 0, 0, 1, 0] and o["n_final"] == 0
    st["needs_reset"][:] = 0
    o = R.ref_maze_episode_end(st, dict(cfg, mode=1))
    assert o["reset_idx"].tolist() == [1, 2, 3, 4] and o["elapsed"].tolist() == [4, 0, 0, 0, 0] and not o["needs_reset"].any() and o["mask"].all() and o["n_final"] == 4
    assert np.array_equal(o["final_rows"], st["packed"][1:])
    o = R.ref_maze_episode_end(st, dict(cfg, mode=2, continuing_task=1, limit=0))
    assert o["reset_count"] == 0 and not o["terminated"].any() and not o["truncated"].any() and o["elapsed"].tolist() == [4, 5, (1 << 33) + 1, 5, 1]


# ------------------------------------------------------------------------------------------------------------------ copies
def test_ref_her_append_and_commit_by_hand():
    N, W, A = 4, 3, 2
    packed, act = np.arange(N * W, dtype=np.float32).reshape(N, W), np.arange(N * A, dtype=np.float32).reshape(N, A)
    start, prev, term = np.array([1, 2, 3, 4], np.int32), np.zeros(N, np.int32), np.full(N, -1, np.int32)
    fin = 100 + np.arange(6 * W, dtype=np.float32).reshape(6, W)
    o = R.ref_her_append(np.zeros((N, W), np.float32), np.zeros((N, A), np.float32), packed, act, start, prev, term, 9, N, lst=[2, -1, N + 5, 0, 1, 3], count=N + 10,
                         final_rows=fin, term_rows=np.zeros((N, W), np.float32))
    assert np.array_equal(o["row_dst"], packed) and np.array_equal(o["act_dst"], act)
    assert o["start"].tolist() == [9, 2, 9, 4] and o["prev_start"].tolist() == [1, 0, 3, 0] and o["term_t"].tolist() == [9, -1, 9, -1]      # the count clamps to N = 4 entries
    assert np.array_equal(o["term_rows"][2], fin[0]) and np.array_equal(o["term_rows"][0], fin[3]) and not o["term_rows"][[1, 3]].any()
    o = R.ref_her_append(np.zeros((N, W), np.float32), np.zeros((N, A), np.float32), packed, act, start, None, None, 9, N, lst=[2], count=-3)
    assert o["start"].tolist() == [1, 2, 3, 4] and o["prev_start"] is None

    od = 2
    live = {f: np.full((3, d), 1.0, np.float32) for f, d in (("qpos", 2), ("qvel", 1), ("qacc_ws", 1), ("mocap", 7), ("aux", 8), ("goal", 3), ("obs", od), ("achieved", 3))}
    live.update(packed=np.arange(3 * (od + 8), dtype=np.float32).reshape(3, od + 8), final_packed=np.zeros((3, od + 8), np.float32),
                status=np.array([0, (0x8002 << 16) - (1 << 32) | 4, 5], np.int64).astype(np.int32))
    staged = {f: np.full_like(live[f], 2.0) for f in R.COMMIT_ROWS}
    staged["status"] = np.array([0, 0x31, 0], np.int32)
    new, rows = R.ref_fetch_commit(live, staged, [1], 1, od)
    assert np.array_equal(rows[0], live["packed"][1]) and np.array_equal(new["final_packed"][1], live["packed"][1])
    assert new["packed"][1].tolist() == [2.0] * (od + 6) + live["packed"][1, -2:].tolist()
    assert int(new["status"][1]) & 0xFFFFFFFF == (0x8003 << 16 | 1)      # only the four public flags of the reset launch count
    for f in live:
        assert np.array_equal(new[f][[0, 2]], live[f][[0, 2]]), f


# ------------------------------------------------------------------------------------------------------------------ the ctypes mirror
SIZE_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "grx_capi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(grx_maze_episode_args), offsetof(grx_maze_episode_args, n_goal), offsetof(grx_maze_episode_args, noise_range),
         offsetof(grx_maze_episode_args, terminated), offsetof(grx_maze_episode_args, reset_count), offsetof(grx_maze_episode_args, final_rows));
  return 0;
}
"""


def test_maze_episode_args_struct_mirrors_the_header(tmp_path):
    from gymnasium_robotics_amd import _native

    S = _native.MazeEpisodeArgsStruct
    # nine pointers, six ints, three doubles, ten pointers: no padding on an LP64 target
    assert ctypes.sizeof(S) == 9 * 8 + 6 * 4 + 3 * 8 + 10 * 8 == 200
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:      # the hand count above stands alone
        return
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text(SIZE_C)
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(S), S.n_goal.offset, S.noise_range.offset, S.terminated.offset, S.reset_count.offset, S.final_rows.offset]
    names = [n for n, _ in S._fields_]      # field for field, in the header's order
    assert names == ["elapsed", "needs_reset", "success", "achieved", "goal", "status", "packed", "rng", "goal_xy", "n_goal", "mode", "limit", "continuing_task", "reset_target",
                     "packed_dim", "noise_range", "scaling", "goal_radius", "terminated", "truncated", "mask", "step_success", "desired", "reset_count", "reset_idx", "n_final",
                     "final_idx", "final_rows"]
