"""Plain numpy / Python restatements of the contracts of the device bookkeeping entry points (include/grx_capi.h): the cost order with its slot-aware placement, the moving
average, a maze step's episode bookkeeping with MazeEnv.update_goal's redraw, the HER append and the commit of an overlapped Fetch reset.  Nothing here imports the package or
its native library, nothing is written the way a kernel is: the sort is numpy's, the redraw walks a numpy Generator, every copy is an array assignment.  The references are
checked on their own in tests/test_cpu_bookkeeping_refs.py and the device is compared with them in tests/test_gpu_bookkeeping.py."""
import math

import numpy as np

M64 = (1 << 64) - 1
STATUS_BADNUM = 1      # GRX_STATUS_BADNUM
REDRAW_GUARD = 65536   # rejected draws after which grx_maze_episode_end gives up on a world


# ------------------------------------------------------------------------------------------------------------------ order
def order_keys(cost, ema_out=None):
    """uint32 sort key of every world: 16 x the cost (as float32, or the moving average the device wrote back), clipped to [0, 4e9].  A float32 times 16 is exact."""
    c = np.asarray(cost).astype(np.float32) if ema_out is None else np.asarray(ema_out, dtype=np.float32)
    return np.clip(c * np.float32(16.0), np.float32(0.0), np.float32(4.0e9)).astype(np.uint32)


def placement_m(k_slice, slots):
    """M of one slice (0 = the plain order): the number of worlds that have to be some wave slot's THIRD world when `per` worlds share `slots` slots and the K predicted
    stragglers -- key above twice the slice's smallest -- hold theirs for the whole launch."""
    per = len(k_slice)
    if not (0 < slots < per <= 2 * slots):
        return 0
    K = int((k_slice.astype(np.uint64) > 2 * int(k_slice.min())).sum())
    M = per - 2 * slots + K
    if M < 0 or 3 * M > per - slots or 4 * M > slots:
        return 0
    return M


def ref_order(cost, ema_out, n, slots):
    """order [n] int32 of grx_order_by_cost_slots / grx_fetch_post_step: eight slices of n / 8 contiguous worlds, each by decreasing key with the lower world first among equals;
    order[pos * 8 + s] = the world that workgroup position `pos` of slice s runs.  With the placement active (placement_m > 0) the positions read the decreasing list d as
        [0, slots - M)          d[pos]                      the stragglers and the expensive worlds start the launch
        [slots - M, slots)      the M cheapest              they end the first round and free their slots first
        [slots, slots + M)      the next M cheapest         dispatched onto exactly those slots
        [slots + M, per - M)    d[pos - 2 M]                the middle, still decreasing
        [per - M, per)          the next M cheapest again   dispatched last, when that second cheap world ends
    each group of M in the list's own (decreasing) order."""
    assert n > 0 and n % 8 == 0
    per = n // 8
    k = order_keys(cost, ema_out)
    assert k.shape == (n,)
    order = np.full(n, -1, np.int32)
    for s in range(8):
        worlds = np.arange(s * per, (s + 1) * per)
        ks = k[worlds]
        d = worlds[np.lexsort((worlds, -ks.astype(np.int64)))]      # by (-key, world)
        M = placement_m(ks, slots)
        if M > 0:
            d = np.concatenate([d[:slots - M], d[per - M:], d[per - 2 * M: per - M], d[slots - M: per - 3 * M], d[per - 3 * M: per - 2 * M]])
            assert len(d) == per
        order[s::8] = d
    return order


def ref_ema(cost, ema_in, alpha):
    """the moving average in fp64; the device's float32 value lies within EMA_ULPS float32 ulps of it (ulps_apart)"""
    return (1.0 - float(alpha)) * np.asarray(ema_in, dtype=np.float64) + float(alpha) * np.asarray(cost, dtype=np.float64)


# Three float32 roundings separate the device from ref_ema -- 1 - alpha, (1 - alpha) * ema (alpha * cost fuses into the sum or rounds once more), the sum -- of at most half
# an ulp of a term that, on positive inputs, is no larger than the result; float32(alpha) itself is the value the caller passes to both.  4 ulps covers them with room.
EMA_ULPS = 4


def ulps_apart(value32, ref64):
    """|value - ref| in units of the float32 spacing at ref"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.abs(np.asarray(value32, dtype=np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ PCG64 rows
def rng_row(gen):
    """a numpy Generator's position as the device row: state_hi, state_lo, inc_hi, inc_lo, has_uint32 << 32 | uinteger (the stale half of a consumed buffer is not state)"""
    s = gen.bit_generator.state
    st, inc, has = s["state"]["state"], s["state"]["inc"], int(s["has_uint32"])
    return [st >> 64, st & M64, inc >> 64, inc & M64, (has << 32) | (int(s["uinteger"]) if has else 0)]


def rng_from_row(row):
    """the numpy Generator that continues the stream of a device row"""
    hi, lo, ihi, ilo, buf = (int(x) for x in row)
    bg = np.random.PCG64()
    bg.state = {"bit_generator": "PCG64", "state": {"state": (hi << 64) | lo, "inc": (ihi << 64) | ilo}, "has_uint32": int(buf >> 32) & 1, "uinteger": buf & 0xFFFFFFFF}
    return np.random.Generator(bg)


def redraw(gen, achieved32, goal32, goal_xy, noise_range, scaling, goal_radius):
    """MazeEnv.update_goal for one world: starting from the float32 goal and position widened to fp64, draw a goal cell and two noise terms until the goal is farther than the
    radius.  Returns (goal fp64 pair, rejected draws); REDRAW_GUARD rejections end the loop (the caller keeps the old goal and flags the world)."""
    ax, ay = float(achieved32[0]), float(achieved32[1])
    gx, gy = float(goal32[0]), float(goal32[1])
    n_goal, rejected = len(goal_xy), 0
    while rejected < REDRAW_GUARD:
        dx, dy = ax - gx, ay - gy
        if not math.sqrt(dx * dx + dy * dy) <= goal_radius:
            break
        c = int(gen.integers(0, n_goal))
        gx = float(goal_xy[c][0]) + float(gen.uniform(-noise_range, noise_range)) * scaling
        gy = float(goal_xy[c][1]) + float(gen.uniform(-noise_range, noise_range)) * scaling
        rejected += 1
    return (gx, gy), rejected


# ------------------------------------------------------------------------------------------------------------------ maze episode end
def ref_maze_episode_end(state, cfg):
    """grx_maze_episode_end, world by world.  state: elapsed int64 [N], needs_reset / success uint8 [N], achieved / goal float32 [N, 2], status int32 [N], packed float32
    [N, D] or None, rng uint64 [N, 5] or None.  cfg: mode, limit, continuing_task, reset_target, goal_xy [n_goal, 2], noise_range, scaling, goal_radius.  Returns every array
    the call writes (inputs are not modified), reset_idx as the ascending list, reset_count, n_final, final_idx and final_rows (the listed worlds' packed rows)."""
    N = len(state["elapsed"])
    mode, limit, cont = int(cfg["mode"]), int(cfg["limit"]), bool(cfg["continuing_task"])
    assert mode in (0, 1, 2)
    out = {k: (None if state.get(k) is None else np.array(state[k], copy=True)) for k in ("elapsed", "needs_reset", "goal", "status", "rng")}
    out["terminated"], out["truncated"], out["mask"] = np.zeros(N, np.uint8), np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    out["step_success"] = (np.asarray(state["success"]) != 0).astype(np.uint8)
    out["desired"] = np.array(state["goal"], dtype=np.float32, copy=True)
    goal_xy = None if cfg.get("goal_xy") is None else np.asarray(cfg["goal_xy"], dtype=np.float64)
    listed = []
    for w in range(N):
        pending = bool(state["needs_reset"][w])
        stepped, succ = not pending, bool(state["success"][w])
        el = int(state["elapsed"][w]) + int(stepped)
        term = stepped and not cont and succ
        trunc = stepped and limit > 0 and el >= limit
        done = term or trunc
        out["terminated"][w], out["truncated"][w] = term, trunc
        if cfg.get("reset_target") and cont and goal_xy is not None and len(goal_xy) > 1 and stepped and succ:
            gen = rng_from_row(state["rng"][w])
            (gx, gy), rejected = redraw(gen, state["achieved"][w], state["goal"][w], goal_xy, float(cfg["noise_range"]), float(cfg["scaling"]), float(cfg["goal_radius"]))
            out["rng"][w] = np.array(rng_row(gen), dtype=np.uint64)
            if rejected == REDRAW_GUARD:
                out["status"][w] = np.int32(int(out["status"][w]) | STATUS_BADNUM | (STATUS_BADNUM << 16))
            else:
                out["goal"][w] = (np.float32(gx), np.float32(gy))
        next_pending = False
        if mode == 0:
            if pending:
                listed.append(w); el = 0
            next_pending = stepped and done
        elif mode == 1 and done:
            listed.append(w); el = 0
        out["elapsed"][w] = el
        out["needs_reset"][w] = next_pending
        out["mask"][w] = not next_pending
    out["reset_idx"] = np.array(listed, dtype=np.int32)
    out["reset_count"] = len(listed)
    out["n_final"] = len(listed) if mode == 1 else 0
    out["final_idx"] = out["reset_idx"] if mode == 1 else np.zeros(0, np.int32)
    out["final_rows"] = None if state.get("packed") is None or mode != 1 else np.asarray(state["packed"])[out["reset_idx"]]
    return out


def rng_rows_equal(a, b):
    """two [.., 5] arrays of PCG64 rows name the same stream positions: the buffered half counts only while its flag is set"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    flag = (a[..., 4] >> np.uint64(32)) == (b[..., 4] >> np.uint64(32))
    half = np.where((a[..., 4] >> np.uint64(32)) != 0, a[..., 4] == b[..., 4], True)
    return bool(np.array_equal(a[..., :4], b[..., :4]) and flag.all() and half.all())


# ------------------------------------------------------------------------------------------------------------------ HER append
def ref_her_append(row_dst, act_dst, packed, action, start, prev_start, term_t, t, n_worlds, lst=None, count=0, mask=None, final_rows=None, term_rows=None):
    """grx_her_append on copies: the ring row takes the step's rows; every reset world w -- mask[w] != 0, or the in-range entries among the first clip(count, 0, n_worlds) of
    the list -- gets prev_start <- start, term_t <- t, start <- t; final_rows[j] goes to term_rows[lst[j]] for those entries.  prev_start / term_t / term_rows may be None."""
    cp = lambda x: None if x is None else np.array(x, copy=True)
    row_dst, act_dst, start, prev_start, term_t, term_rows = cp(row_dst), cp(act_dst), cp(start), cp(prev_start), cp(term_t), cp(term_rows)
    row_dst[...] = np.asarray(packed).reshape(row_dst.shape)
    act_dst[...] = np.asarray(action).reshape(act_dst.shape)
    worlds = []
    if mask is not None:
        worlds = [(None, w) for w in range(n_worlds) if mask[w]]
    elif lst is not None:
        k = min(max(int(count), 0), n_worlds)
        worlds = [(j, int(lst[j])) for j in range(k) if 0 <= int(lst[j]) < n_worlds]
    for j, w in worlds:
        if prev_start is not None:
            prev_start[w], term_t[w] = start[w], t
        start[w] = t
        if term_rows is not None and j is not None:
            term_rows[w] = final_rows[j]
    return dict(row_dst=row_dst, act_dst=act_dst, start=start, prev_start=prev_start, term_t=term_t, term_rows=term_rows)


# ------------------------------------------------------------------------------------------------------------------ Fetch commit
COMMIT_ROWS = ("qpos", "qvel", "qacc_ws", "mocap", "aux", "goal", "obs", "achieved")


def ref_fetch_commit(live, staged, idx, k, obs_dim, with_final=True):
    """grx_fetch_commit_rows on copies of `live` (dict of [n, ...] arrays: COMMIT_ROWS, packed, final_packed, status; mocap None for a model without mocap bodies): the staged
    rows of every listed world replace the live ones, the packed row becomes obs | achieved | goal | its old last two words, the old packed row is parked in final_packed and
    in rows[j], the status word takes the reset launch's flags in its low half and accumulates them in the sticky half.  Returns (new live dict, rows [k, obs_dim + 8])."""
    new = {f: (None if v is None else np.array(v, copy=True)) for f, v in live.items()}
    rows = np.zeros((k, obs_dim + 8), np.float32)
    for j in range(k):
        w = int(idx[j])
        old = np.array(live["packed"][w], copy=True)
        rows[j] = old
        if with_final:
            new["final_packed"][w] = old
        for f in COMMIT_ROWS:
            if new[f] is not None:
                new[f][w] = staged[f][w]
        new["packed"][w] = np.concatenate([staged["obs"][w], staged["achieved"][w], staged["goal"][w], old[-2:]])
        now, was = int(staged["status"][w]) & 15, int(live["status"][w])
        word = now | ((((was >> 16) | now) & 0xFFFF) << 16)      # (>> on a Python int is arithmetic, like the C shift of the int32 word)
        new["status"][w] = word - (1 << 32) if word >= (1 << 31) else word      # the same 32 bits as an int32
    return new, rows
