"""Plain numpy / Python-integer restatements of the reset path's small entry points (include/grx_capi.h): grx_kitchen_bookkeeping, grx_hand_commit_rows,
grx_adroit_commit_rows, grx_maze_reset_rows[_list] and the reset samplers (grx_fetch_sample_resets[_device], grx_adroit_sample_resets_device,
grx_maze_sample_resets_device / _list, grx_sample_uniform_rows / grx_uniform_rows_device).  Written from the header's contracts and the reference lines they cite:
the bookkeeping is a per-world loop over Python ints, the commits are slicing copies, every sampler continues a numpy Generator rebuilt from the world's state row
and calls nothing but Generator.uniform and Generator.integers, in the reference's order.  Nothing here imports torch or the native library.

Every reference takes `mistake=None`; a name from its MISTAKES tuple makes it wrong in one deliberate way.  The case tables at the end are shared by
tests/test_cpu_reset_refs.py (which shows that each mistake answers differently from the correct reference on them) and tests/test_gpu_reset_kernels.py (which
runs the device on them)."""
import math

import numpy as np

from bookkeeping_refs import M64, rng_from_row, rng_row

SENT_F, SENT_I, SENT_B = -12345.5, -77, 0xAB      # what the GPU file pre-fills outputs with (tests/test_gpu_bookkeeping.py); the tables below carry them as prior content
GUARD_DRAWS = 65536                              # iterations after which a device sampler's rejection loop gives up
NAN = float("nan")


def as_int32(word):
    """the 32 bits of a Python int as an int32 value"""
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >= (1 << 31) else word


# ================================================================================================================== kitchen bookkeeping
KITCHEN_MISTAKES = ("el_gt", "term_unstepped", "pending_reward", "step_completions_kept", "needs_reset_kept", "final_info_mode1")
KITCHEN_FIELDS = ("tasks_to_complete", "episode_completions", "elapsed", "step_completions", "reward", "terminated", "truncated", "needs_reset", "reset_now", "qpos", "qvel",
                  "qacc_ws", "final_info")


def kitchen_bookkeeping(state, cfg, completed, stepped, init_qpos, mistake=None):
    """grx_kitchen_bookkeeping on copies of `state` (every buffer of KITCHEN_FIELDS with its content before the call; final_info None = NULL), world by world on Python
    ints: KitchenEnv.step's bookkeeping (kitchen_env.py:386-423), the TimeLimit, and the autoreset rules of the header comment / KitchenVecEnv.step_finish.
    cfg: nq, nv, all_mask, max_steps, remove_when_completed, terminate_when_completed, mode (0 disabled, 1 next_step, 2 same_step).  stepped: [N] or None (= all)."""
    assert mistake is None or mistake in KITCHEN_MISTAKES
    out = {k: (None if state[k] is None else np.array(state[k], copy=True)) for k in KITCHEN_FIELDS}
    N, mode, all_mask, max_steps = len(state["elapsed"]), int(cfg["mode"]), int(cfg["all_mask"]), int(cfg["max_steps"])
    for w in range(N):
        st = True if stepped is None else bool(stepped[w])
        pending = mode == 1 and bool(state["needs_reset"][w])
        ttc, epi, el = int(state["tasks_to_complete"][w]), int(state["episode_completions"][w]), int(state["elapsed"][w])
        step_done = (int(completed[w]) & ttc) if st else 0
        if cfg["remove_when_completed"]:
            ttc &= ~step_done
        epi |= step_done
        term = bool(cfg["terminate_when_completed"]) and (st or mistake == "term_unstepped") and epi == all_mask
        el += int(st)
        trunc = max_steps > 0 and st and (el > max_steps if mistake == "el_gt" else el >= max_steps)
        done = term or trunc
        reset_now = pending or (mode == 2 and done)
        out["reward"][w] = 0.0 if (pending and mistake != "pending_reward") else float(bin(step_done).count("1"))
        out["terminated"][w], out["truncated"][w] = term, trunc
        out["step_completions"][w] = 0 if (mode == 2 and done and mistake != "step_completions_kept") else step_done
        if mode == 1:
            out["needs_reset"][w] = (1 if mistake == "needs_reset_kept" else 0) if pending else int(bool(state["needs_reset"][w]) or done)
        out["reset_now"][w] = reset_now
        if out["final_info"] is not None and done and (mode == 2 or (mode == 1 and mistake == "final_info_mode1")):
            out["final_info"][w] = (ttc, step_done, epi)      # of the episode that just ended, before the rewind
        if reset_now:      # FrankaRobot.reset_model: init_qpos, zero velocity, no warm start
            ttc, epi, el = all_mask, 0, 0
            out["qpos"][w], out["qvel"][w], out["qacc_ws"][w] = init_qpos, 0.0, 0.0
        out["tasks_to_complete"][w], out["episode_completions"][w], out["elapsed"][w] = ttc, epi, el
    return out


# ================================================================================================================== commits
HAND_ROWS = ("qpos", "qvel", "qacc_ws", "obs", "achieved", "palm", "goal")
HAND_MISTAKES = ("by_world", "status_adroit_way", "last_two", "goal_slot")
ADROIT_ROWS = ("qpos", "qvel", "qacc_ws", "shift", "target", "obs")
ADROIT_MISTAKES = ("status_hand_way", "bit16_leak")


def hand_status(old, staged):
    """the sticky (upper) half of the staged word is OR-ed in; the low half stays the finished episode's"""
    return as_int32(int(old) | (int(staged) & 0xFFFF0000))


def adroit_status(old, staged, leak=False):
    """the four public flags of the staged word replace the low half and join the sticky half; its internal bits 4 and above, bit 16 and above included, are dropped
    (>> on a Python int is arithmetic, like the C shift of the int32 word)"""
    now = int(staged) & 15
    sticky = (int(old) >> 16) | now | ((int(staged) >> 16) if leak else 0)
    return as_int32(now | ((sticky & 0xFFFF) << 16))


def hand_commit(live, staged, idx, k, od, gd, mistake=None):
    """grx_hand_commit_rows on copies of `live` ([N, ...] arrays HAND_ROWS, packed [N, od + 2 gd + 2], status): row j of the staged block (indexed by LIST POSITION)
    replaces world idx[j]; the packed row becomes [staged obs | staged achieved | the new goal | its own last two words]"""
    assert mistake is None or mistake in HAND_MISTAKES
    new = {f: np.array(v, copy=True) for f, v in live.items()}
    for j in range(k):
        w = int(idx[j])
        s = w if mistake == "by_world" else j
        for f in HAND_ROWS:
            new[f][w] = staged[f][s]
        row = np.array(live["packed"][w], copy=True)
        row[:od + gd] = staged["packed"][s][:od + gd]
        if mistake != "goal_slot":
            row[od + gd:od + 2 * gd] = staged["goal"][s]
        if mistake == "last_two":
            row[-2:] = staged["packed"][s][-2:]
        new["packed"][w] = row
        new["status"][w] = adroit_status(live["status"][w], staged["status"][s]) if mistake == "status_adroit_way" else hand_status(live["status"][w], staged["status"][s])
    return new


def adroit_commit(live, staged, idx, k, mistake=None):
    """grx_adroit_commit_rows on copies of `live` ([N, ...] arrays ADROIT_ROWS -- shift / target None without the pair --, status): the staged row of WORLD idx[j]
    replaces the live one"""
    assert mistake is None or mistake in ADROIT_MISTAKES
    new = {f: (None if v is None else np.array(v, copy=True)) for f, v in live.items()}
    for j in range(k):
        w = int(idx[j])
        for f in ADROIT_ROWS:
            if new[f] is not None:
                new[f][w] = staged[f][w]
        if mistake == "status_hand_way":
            new["status"][w] = hand_status(live["status"][w], staged["status"][w])
        else:
            new["status"][w] = adroit_status(live["status"][w], staged["status"][w], leak=mistake == "bit16_leak")
    return new


# ================================================================================================================== maze reset rows
MAZE_ROW_FIELDS = ("qpos", "qvel", "qacc_ws", "goal", "obs", "achieved", "reward", "success", "packed", "desired")
MAZE_ROW_MISTAKES = ("skip_ignored", "radius_lt", "reward_zeroed")


def maze_reset_rows(live, idx, n_reset, stage, qpos0, nq, nv, skip, goal_radius, keep_outcome, mistake=None):
    """grx_maze_reset_rows[_list] on copies of `live` (MAZE_ROW_FIELDS; packed [N, od + 6] or None, desired [N, 2] or None): for list position k, world idx[k] gets
    qpos = qpos0 with xy <- the staged start, zero velocity and warm start, the staged goal, obs = qpos[skip:] | qvel, achieved = the start, success = fp64 distance of
    the float32 stage values <= goal_radius, and -- unless keep_outcome -- reward 0 and the packed row's [reward, success] words."""
    assert mistake is None or mistake in MAZE_ROW_MISTAKES
    new = {f: (None if live[f] is None else np.array(live[f], copy=True)) for f in MAZE_ROW_FIELDS}
    od = nq + nv - skip
    sk = 0 if mistake == "skip_ignored" else skip
    for k in range(n_reset):
        w = int(idx[k])
        sx, sy, gx, gy = (np.float32(v) for v in stage[k])
        q = np.array(qpos0, dtype=np.float32, copy=True)
        q[0], q[1] = sx, sy
        obs = np.concatenate([q[sk:], np.zeros(nv + sk, np.float32)])[:od]
        d = math.sqrt((float(sx) - float(gx)) ** 2 + (float(sy) - float(gy)) ** 2)
        succ = d < goal_radius if mistake == "radius_lt" else d <= goal_radius
        new["qpos"][w], new["qvel"][w], new["qacc_ws"][w], new["obs"][w] = q, 0.0, 0.0, obs
        new["goal"][w], new["achieved"][w], new["success"][w] = (gx, gy), (sx, sy), succ
        zero = not keep_outcome or mistake == "reward_zeroed"
        if zero:
            new["reward"][w] = 0.0
        if new["packed"] is not None:
            new["packed"][w, :od + 4] = np.concatenate([obs, [sx, sy, gx, gy]])
            if zero:
                new["packed"][w, od + 4] = 0.0
            if not keep_outcome:
                new["packed"][w, od + 5] = 1.0 if succ else 0.0
        if new["desired"] is not None:
            new["desired"][w] = (gx, gy)
    return new


# ================================================================================================================== samplers
FETCH_MISTAKES = ("goal_first", "offset_after_height", "air_unconditional")
ADROIT_SAMPLE_MISTAKES = ("door_swapped", "target_first")
MAZE_SAMPLE_MISTAKES = ("integers_1_draws", "buffer_dropped")


def fetch_sample(gen, has_object, in_air, obj_range, target_range, target_offset, gripper, height_offset, guard=True, mistake=None):
    """_reset_sim + _sample_goal of one world (fetch_env.py:153-166, 388-391) -> (object x, y, goal x, y, z) in fp64.  Without an object the first two are the gripper's
    x and y (nothing is drawn for them).  guard: the device gives up after GUARD_DRAWS rejected object draws and poisons the object words with NaN."""
    assert mistake is None or mistake in FETCH_MISTAKES
    g0 = [float(v) for v in gripper]

    def draw_goal():
        return [g0[e] + gen.uniform(-target_range, target_range) for e in range(3)]

    goal = draw_goal() if mistake == "goal_first" else None
    ox, oy = g0[0], g0[1]
    if has_object:
        rejected = 0
        while math.sqrt((ox - g0[0]) ** 2 + (oy - g0[1]) ** 2) < 0.1:
            ox = g0[0] + gen.uniform(-obj_range, obj_range)
            oy = g0[1] + gen.uniform(-obj_range, obj_range)
            rejected += 1
            if guard and rejected == GUARD_DRAWS:      # the device tests the distance GUARD_DRAWS times, then gives up
                ox = oy = NAN
                break
    if goal is None:
        goal = draw_goal()
    if has_object:
        goal = [goal[e] + float(target_offset[e]) for e in range(3)]
        goal[2] = float(height_offset) + (float(target_offset[2]) if mistake == "offset_after_height" else 0.0)
        if mistake == "air_unconditional":
            if in_air:
                gen.uniform(0.0, 1.0)
                goal[2] += gen.uniform(0, 0.45)
        elif in_air and gen.uniform(0.0, 1.0) < 0.5:
            goal[2] += gen.uniform(0, 0.45)
    return [ox, oy] + goal


def adroit_sample(gen, kind, edit_row, pos0, mistake=None):
    """reset_model's draws of hammer (kind 0: board z), door (1: frame position) and relocate (3: ball x / y, then the target) -> (edit [3] fp64 with the components the
    task does not redraw kept, target [3] fp64 or None, shift [7] float32 = float32(edit - the XML pose) and the identity rotation)"""
    assert mistake is None or mistake in ADROIT_SAMPLE_MISTAKES
    e = [float(v) for v in edit_row]
    target = None
    if kind == 0:
        e[2] = gen.uniform(0.1, 0.25)
    elif kind == 1:
        if mistake == "door_swapped":
            e = [gen.uniform(0.25, 0.35), gen.uniform(-0.3, -0.2), gen.uniform(0.252, 0.35)]
        else:
            e = [gen.uniform(-0.3, -0.2), gen.uniform(0.25, 0.35), gen.uniform(0.252, 0.35)]
    elif kind == 3:
        if mistake == "target_first":
            target = [gen.uniform(-0.2, 0.2), gen.uniform(-0.2, 0.2), gen.uniform(0.15, 0.35)]
        e[0] = gen.uniform(-0.15, 0.15)
        e[1] = gen.uniform(-0.15, 0.3)
        if target is None:
            target = [gen.uniform(-0.2, 0.2), gen.uniform(-0.2, 0.2), gen.uniform(0.15, 0.35)]
    else:
        raise ValueError(kind)
    shift = np.array([e[0] - float(pos0[0]), e[1] - float(pos0[1]), e[2] - float(pos0[2]), 1.0, 0.0, 0.0, 0.0]).astype(np.float32)
    return e, target, shift


def maze_sample(gen, goal_xy, reset_xy, noise, scaling, fixed_goal=None, fixed_reset=None, guard=True, mistake=None):
    """MazeEnv.reset's draws of one world (maze_v4.py:299-358: generate_target_goal, add_xy_position_noise, generate_reset_pos, add_xy_position_noise) ->
    (start x, y, goal x, y) in fp64.  fixed_goal / fixed_reset: options["goal_cell"] / ["reset_cell"] as xy.  guard: GUARD_DRAWS rejected reset cells poison the start."""
    assert mistake in (None, "integers_1_draws")

    def cell(cells):
        n = len(cells)
        if n == 1 and mistake == "integers_1_draws":
            gen.integers(0, 2)
        return cells[int(gen.integers(0, n))]

    g = fixed_goal if fixed_goal is not None else cell(goal_xy)
    gx = float(g[0]) + gen.uniform(-noise, noise) * scaling
    gy = float(g[1]) + gen.uniform(-noise, noise) * scaling
    if fixed_reset is not None:
        rx, ry = float(fixed_reset[0]), float(fixed_reset[1])
    else:
        rx, ry, far, rejected = gx, gy, 0.5 * scaling, 0
        while math.sqrt((rx - gx) * (rx - gx) + (ry - gy) * (ry - gy)) <= far:
            r = cell(reset_xy)
            rx, ry = float(r[0]), float(r[1])
            rejected += 1
            if guard and rejected == GUARD_DRAWS:
                rx = ry = NAN
                break
    rx += gen.uniform(-noise, noise) * scaling
    ry += gen.uniform(-noise, noise) * scaling
    return [rx, ry, gx, gy]


def uniform_row(gen, count):
    """`count` consecutive uniform(-1, 1) draws, rounded to float32"""
    return np.array([gen.uniform(-1.0, 1.0) for _ in range(count)], dtype=np.float64).astype(np.float32)


def sample_listed(rows, idx, fn, mistake=None):
    """run fn(gen, k, w) for the list's worlds on generators continued from their rows; -> (new rows, [fn's results in list order]).  rows: [N, 4] (a PCG64 stream
    without its 32-bit buffer) or [N, 5] uint64.  The rows of unlisted worlds are returned as they came."""
    rows = np.array(rows, dtype=np.uint64, copy=True)
    wide = rows.shape[1] == 5
    res = []
    for k, w in enumerate(idx):
        w = int(w)
        row = [int(x) for x in rows[w]] + ([] if wide else [0])
        if mistake == "buffer_dropped":
            row[4] = 0
        gen = rng_from_row(row)
        res.append(fn(gen, k, w))
        new = rng_row(gen)
        assert wide or new[4] == 0      # a sampler on a 4-word row makes 64-bit draws only
        rows[w] = new if wide else new[:4]
    return rows, res


def rows_equal(a, b):
    """stream rows name the same positions: words 0 - 3, and for [.., 5] rows the buffer flag and -- while it is set -- the buffered half"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    if a.shape != b.shape or not np.array_equal(a[..., :4], b[..., :4]):
        return False
    if a.shape[-1] == 4:
        return True
    fa, fb = a[..., 4] >> np.uint64(32), b[..., 4] >> np.uint64(32)
    return bool(np.array_equal(fa, fb) and np.where(fa != 0, a[..., 4] == b[..., 4], True).all())


# ================================================================================================================== case tables
# ------------------------------------------------------------------------------------------------------------------ kitchen
KITCHEN_N = (1, 255, 256, 257, 1000)      # one world, and the edge of a 256-thread block from both sides, several blocks
KITCHEN_MASKS = (0b0000100, 0b0100010, 0b1111111)      # tasks_to_complete of a fresh episode: 1, 2 and 7 bits
KITCHEN_CALLS = 4


def kitchen_chains(N, mode):
    """The kitchen table of one (N, mode): one chain per remove_when_completed x terminate_when_completed x max_steps in {0, 3} (and, in mode 1, one more with
    stepped = NULL, see below), the other parameters cycling so that every mode meets each of them.  A chain is (cfg, stepped_kind, init_qpos, state, calls): the
    buffers before the first call (outputs hold sentinels) and KITCHEN_CALLS consecutive (completed, stepped) inputs on the carried state -- a world that ends in one
    call is pending in the next.  stepped_kind: "not_needs" (mode 1: !needs_reset as the call finds it), "null", "random" (modes 0 and 2).
    The completion words are random bytes: bits outside tasks_to_complete, and bit 7 outside every mask, are set all the time."""
    rng = np.random.default_rng(1000 * N + mode)
    combos = [(rem, term, ms) for rem in (0, 1) for term in (0, 1) for ms in (0, 3)]
    plans = [(c, "not_needs" if mode == 1 else ("null" if i % 2 == 0 else "random")) for i, c in enumerate(combos)]
    if mode == 1:
        # the header: a pending world is rewound and reports reward 0 WHATEVER stepped[w] says.  With stepped = NULL the pending worlds count as stepped: their
        # completions are scored into the flags, the reward still has to be 0 (this chain is what tells the "pending_reward" mistake from the reference).
        plans.append(((1, 1, 3), "null"))
    for i, ((rem, term, ms), kind) in enumerate(plans):
        nq, nv = ((30, 29), (3, 2))[i % 2]
        all_mask = KITCHEN_MASKS[(i + mode) % 3]
        cfg = dict(nq=nq, nv=nv, all_mask=all_mask, max_steps=ms, remove_when_completed=rem, terminate_when_completed=term, mode=mode)
        init_qpos = rng.standard_normal(nq).astype(np.float32)
        state = dict(tasks_to_complete=np.full(N, all_mask, np.int32), episode_completions=np.zeros(N, np.int32), elapsed=np.zeros(N, np.int32),
                     step_completions=np.full(N, SENT_I, np.int32), reward=np.full(N, SENT_F, np.float32), terminated=np.full(N, SENT_B, np.uint8),
                     truncated=np.full(N, SENT_B, np.uint8), needs_reset=np.zeros(N, np.uint8) if mode == 1 else np.full(N, SENT_B, np.uint8),
                     reset_now=np.full(N, SENT_B, np.uint8), qpos=rng.standard_normal((N, nq)).astype(np.float32), qvel=rng.standard_normal((N, nv)).astype(np.float32),
                     qacc_ws=rng.standard_normal((N, nv)).astype(np.float32), final_info=np.full((N, 3), SENT_I, np.int32) if (i // 2) % 2 == 0 else None)
        calls, cur = [], state
        for _ in range(KITCHEN_CALLS):
            completed = rng.integers(0, 256, N).astype(np.int32)
            completed[rng.random(N) < 0.3] |= all_mask      # enough worlds complete a 7-task episode for a termination to occur
            stepped = None if kind == "null" else ((cur["needs_reset"] == 0).astype(np.uint8) if kind == "not_needs" else (rng.random(N) < 0.6).astype(np.uint8) * 3)
            calls.append((completed, stepped))
            cur = kitchen_bookkeeping(cur, cfg, completed, stepped, init_qpos)
            cur["qpos"] = cur["qpos"] + np.float32(1.0)      # (the step kernel moves the worlds between two calls; the GPU test does the same)
            cur["qvel"] = cur["qvel"] + np.float32(1.0)
            cur["qacc_ws"] = cur["qacc_ws"] + np.float32(1.0)
        yield cfg, kind, init_qpos, state, calls


def kitchen_walk(chain, mistake=None):
    """the states after every call of a chain, each call starting from the CORRECT state before it (so a mistaken copy is compared call by call)"""
    cfg, _, init_qpos, state, calls = chain
    outs, cur = [], state
    for completed, stepped in calls:
        outs.append(kitchen_bookkeeping(cur, cfg, completed, stepped, init_qpos, mistake=mistake))
        cur = kitchen_bookkeeping(cur, cfg, completed, stepped, init_qpos) if mistake else outs[-1]
        cur = dict(cur, qpos=cur["qpos"] + np.float32(1.0), qvel=cur["qvel"] + np.float32(1.0), qacc_ws=cur["qacc_ws"] + np.float32(1.0))
    return outs


# ------------------------------------------------------------------------------------------------------------------ commits
COMMIT_N = 64
HAND_DIMS = ((38, 36, 61, 7), (70, 66, 70, 11), (3, 2, 5, 1))      # (nq, nv, obs, goal): the manipulate hand's, every row wider than a wave, tiny rows
ADROIT_DIMS = ((36, 36, 46), (70, 66, 70))                        # (nq, nv, obs)


def commit_lists():
    """k = 1, all worlds reversed, 17 scattered worlds"""
    rng = np.random.default_rng(17)
    return [[COMMIT_N - 1], list(range(COMMIT_N))[::-1], [int(w) for w in rng.permutation(COMMIT_N)[:17]]]


def status_words(call, rng):
    """(old, staged) int32 [64]: over calls 0 - 3 the low four bits of the two words run through all 256 pairs; the sticky bits, the bits of value 16 and 32 of the low
    half and the sign bit are random, each set and clear many times"""
    p = 64 * (call % 4) + np.arange(COMMIT_N)
    hi = lambda: rng.integers(0, 1 << 16, COMMIT_N).astype(np.int64) << 16      # sticky bits, bit 16 and the sign bit among them
    mid = lambda: rng.integers(0, 4, COMMIT_N).astype(np.int64) << 4
    to32 = lambda x: np.array([as_int32(int(v)) for v in x], dtype=np.int32)
    return to32(hi() | mid() | (p % 16)), to32(hi() | mid() | (p // 16))


def hand_case(dims, call):
    nq, nv, od, gd = dims
    n, rng = COMMIT_N, np.random.default_rng(100 * nq + call)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    widths = dict(qpos=nq, qvel=nv, qacc_ws=nv, obs=od, achieved=gd, palm=3, goal=gd, packed=od + 2 * gd + 2)
    live, staged = {f: r(n, w) for f, w in widths.items()}, {f: r(n, w) for f, w in widths.items()}      # (the staged block has a row per list position: at most n)
    live["status"], staged["status"] = status_words(call, rng)
    return live, staged


def adroit_case(dims, call, pairs):
    nq, nv, od = dims
    n, rng = COMMIT_N, np.random.default_rng(100 * nq + call + 7)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    widths = dict(qpos=nq, qvel=nv, qacc_ws=nv, shift=7, target=3, obs=od)
    live, staged = ({f: (r(n, w) if (pairs or f not in ("shift", "target")) else None) for f, w in widths.items()} for _ in range(2))
    live["status"], staged["status"] = status_words(call, rng)
    return live, staged


# ------------------------------------------------------------------------------------------------------------------ maze rows
MAZE_ROW_DIMS = ((2, 2, 0), (15, 14, 2), (70, 66, 1), (3, 2, 2))      # (nq, nv, obs_skip): the point mass, the ant, rows wider than a wave, an observation without any qpos entry but one
MAZE_ROW_N = 48
RADIUS_A = float(np.float32(0.45))      # exactly the fp64 distance of (0, 0) and (float32(0.45), 0)
RADIUS_B = 0.625                        # exactly the fp64 distance of (1, -2) and (1.375, -1.5): 3 : 4 : 5


def maze_stage(n, radius, rng):
    """[n, 4] float32 (start x, y, goal x, y): the first rows are start - goal pairs AT the radius, one float32 ulp inside and one outside it, the others random (half
    of them within a radius or so)"""
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    if radius == RADIUS_A:
        r = f(0.45)
        edge = [(0, 0, r, 0), (0, 0, dn(r), 0), (0, 0, up(r), 0), (0, 0, 0, -r), (0, 0, 0, -dn(r)), (0, 0, 0, -up(r)), (-r, 0, 0, 0), (dn(-r), 0, 0, 0), (up(-r), 0, 0, 0)]
    else:
        edge = [(1, -2, 1.375, -1.5), (1, -2, dn(1.375), -1.5), (1, -2, up(1.375), -1.5), (1, -2, 1.375, dn(-1.5)), (1, -2, 1.375, up(-1.5)),
                (1.5, -2.375, 1, -2), (1.5, up(-2.375), 1, -2), (1.5, dn(-2.375), 1, -2)]
    stage = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
    stage[n // 2:, 2:] = stage[n // 2:, :2] + rng.uniform(-0.4, 0.4, (n - n // 2, 2)).astype(np.float32)
    stage[:len(edge)] = np.array(edge, dtype=np.float32)
    return stage


def maze_row_case(dims, keep_outcome, packed, seed):
    """(live, idx, n_reset, stage, qpos0, radius): 17 scattered worlds of MAZE_ROW_N, a list longer than n_reset (the entries beyond are never read)"""
    nq, nv, skip = dims
    od, n = nq + nv - skip, MAZE_ROW_N
    rng = np.random.default_rng(10 * nq + 2 * keep_outcome + packed + 100 * seed)
    radius = (RADIUS_A, RADIUS_B)[(seed + keep_outcome) % 2]
    live = dict(qpos=(n, nq), qvel=(n, nv), qacc_ws=(n, nv), goal=(n, 2), obs=(n, od), achieved=(n, 2), reward=(n,), packed=(n, od + 6), desired=(n, 2))
    live = {f: np.full(s, SENT_F, np.float32) for f, s in live.items()}
    live["success"] = np.full(n, SENT_B, np.uint8)
    if not packed:
        live["packed"] = None
    if keep_outcome:      # the finished episode's outcome is what has to survive
        live["reward"] = rng.standard_normal(n).astype(np.float32)
        if packed:
            live["packed"][:, -2:] = rng.standard_normal((n, 2)).astype(np.float32)
    idx = rng.permutation(n).astype(np.int32)
    return live, idx, 17, maze_stage(17, radius, rng), rng.standard_normal(nq).astype(np.float32), radius


# ------------------------------------------------------------------------------------------------------------------ samplers
SAMPLER_WORLDS = 300
SAMPLER_N = (1, 63, 64, 65, 200)
UNIFORM_N = (1, 255, 256, 257)
FETCH_GRIPPER, FETCH_OFFSET, FETCH_HEIGHT = (1.3419, 0.7491, 0.5347), (0.011, -0.023, 0.037), 0.4249
ADROIT_POS0 = (-0.05, 0.31, 0.213)


def stream_rows(n, seed, wide=False, buffered=False):
    """[n, 4 or 5] uint64: PCG64 streams of seeds seed, seed + 1, ..; every other one already advanced by a few draws, and with `buffered` every third one left with a
    buffered 32-bit half"""
    gens = [np.random.Generator(np.random.PCG64(seed + w)) for w in range(n)]
    for w, g in enumerate(gens):
        if w % 2:
            g.uniform(size=1 + w % 5)
        if buffered and w % 3 == 0:
            g.integers(0, 3)
    rows = np.array([rng_row(g) for g in gens], dtype=np.uint64)
    assert not buffered or (rows[:, 4] >> np.uint64(32)).sum() >= n // 4
    return rows if wide else np.ascontiguousarray(rows[:, :4])


def sparse_list(n, seed):
    """n distinct worlds of SAMPLER_WORLDS in a random order"""
    return np.random.default_rng(seed).permutation(SAMPLER_WORLDS)[:n].astype(np.int64)


def fetch_cfgs():
    """has_object x target_in_the_air with the reference's ranges"""
    return [dict(has_object=h, in_air=a, obj_range=0.15, target_range=0.15) for h in (0, 1) for a in (0, 1)]


def fetch_reference(rows, idx, cfg, guard=True, mistake=None):
    """-> (new rows, samples [n, 5] fp64)"""
    fn = lambda gen, k, w: fetch_sample(gen, cfg["has_object"], cfg["in_air"], cfg["obj_range"], cfg["target_range"], FETCH_OFFSET, FETCH_GRIPPER, FETCH_HEIGHT, guard=guard,
                                        mistake=mistake)
    rows, res = sample_listed(rows, idx, fn)
    return rows, np.array(res, dtype=np.float64).reshape(len(idx), 5)


def adroit_reference(rows, idx, kind, bufs, mistake=None):
    """bufs: edit [N, 3] fp64, target64 [N, 3] fp64, shift [N, 7] float32, target [N, 3] float32 (the target pair may be None) -> (new rows, new bufs)"""
    new = {f: (None if v is None else np.array(v, copy=True)) for f, v in bufs.items()}

    def fn(gen, k, w):
        e, t, s = adroit_sample(gen, kind, bufs["edit"][w], ADROIT_POS0, mistake=mistake)
        new["edit"][w], new["shift"][w] = e, s
        if t is not None:
            new["target64"][w], new["target"][w] = t, np.array(t).astype(np.float32)

    rows, _ = sample_listed(rows, idx, fn)
    return rows, new


def maze_cells(n, scaling=1.0):
    grid = np.array([[1.5, 0.5], [-2.5, 1.5], [0.5, -1.5], [3.5, 2.5], [-0.5, -0.5], [2.5, -2.5], [-3.5, 0.5], [-1.5, 2.5]], np.float64)
    return np.ascontiguousarray(grid[:n] * scaling)


def maze_reset_cells(n, scaling=1.0):
    """n reset cells, from the far end of the grid: a single reset cell is no goal cell unless all eight cells are goals"""
    return maze_cells(8, scaling)[::-1][:n].copy()


MAZE_CELL_COUNTS = ((1, 7), (2, 8), (3, 1), (7, 3), (8, 2))      # (n_goal, n_reset): both run through 1, 2, 3, 7, 8; n = 1 draws nothing


def maze_reference(rows, idx, goal_xy, reset_xy, noise, scaling, fixed_goal=None, fixed_reset=None, mistake=None):
    """-> (new rows, stage [n, 4] fp64)"""
    fn = lambda gen, k, w: maze_sample(gen, goal_xy, reset_xy, noise, scaling, fixed_goal, fixed_reset, mistake=None if mistake == "buffer_dropped" else mistake)
    rows, res = sample_listed(rows, idx, fn, mistake="buffer_dropped" if mistake == "buffer_dropped" else None)
    return rows, np.array(res, dtype=np.float64).reshape(len(idx), 4)


def uniform_reference(rows, worlds, count):
    """-> (new rows, {world: float32 row})"""
    out = {}
    rows, _ = sample_listed(rows, worlds, lambda gen, k, w: out.__setitem__(w, uniform_row(gen, count)))
    return rows, out
