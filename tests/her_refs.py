"""Plain numpy / Python restatements of the hindsight-experience-replay entry points (include/grx_capi.h: grx_her_sample, grx_her_sample_final, grx_her_relabel,
grx_her_draw_relabel, grx_her_sample_relabel): which (row, world, goal row) a given (seed, call, sample) must draw, and which packed replay row a given draw must produce.
Nothing here imports torch or the native library.  The draw is stated twice -- ref_her_draw_scalar, one sample in Python integers, line for line what the device function
does, and ref_her_draw, the same over an array of samples (the linear probe is looked up in a table of "next world with a transition" instead of being walked) -- and the two
are compared in tests/test_cpu_her_refs.py.  Rewards and success flags are computed in fp64 on the fp32 words the kernel reads; the bounds of the dense rewards are derived
next to their definitions below.  The device is compared with all of this in tests/test_gpu_her_refs.py."""
import numpy as np

M64 = (1 << 64) - 1
KEY_SEED, KEY_CALL = 0xD1342543DE82EF95, 0x2545F4914F6CDD1D      # the sample key: seed * KEY_SEED + call * KEY_CALL + b (mod 2^64)
ATTEMPTS = 64                                                    # uniform world draws before the linear probe
_U = np.uint64
_INV24 = np.float32(1.0 / 16777216.0)


# ------------------------------------------------------------------------------------------------------------------ the stream
def splitmix64(state):
    """one step of splitmix64 on an array of np.uint64 states (arithmetic wraps): (new state, output)"""
    s = np.atleast_1d(np.asarray(state, dtype=np.uint64)) + _U(0x9E3779B97F4A7C15)
    z = (s ^ (s >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return s, z ^ (z >> _U(31))


def her_key(seed, call, b):
    """stream state of sample(s) b before the discarded output"""
    base = (int(seed) * KEY_SEED + int(call) * KEY_CALL) & M64
    return _U(base) + np.atleast_1d(np.asarray(b)).astype(np.uint64)


def keep_thresholds(k_future):
    """The "keep the episode's own goal" threshold (float)k / ((float)k + 1.0f).  The device's fp32 division is not required to round correctly, so its quotient may be either
    neighbour of the correctly rounded one: (below, correctly rounded, above).  u2 is a multiple of 2^-24 below 1, so only a u2 EQUAL to one of the three leaves any freedom."""
    q = np.float32(k_future) / (np.float32(k_future) + np.float32(1.0))
    return np.nextafter(q, np.float32(-1.0)), q, np.nextafter(q, np.float32(2.0))


# ------------------------------------------------------------------------------------------------------------------ the draw, one sample, line for line
def _sm(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def ref_her_draw_scalar(start, prev_start, term_t, N, t_now, T, k_future, seed, call, b, thr=None):
    """(t, w, t_goal, found) of ONE sample b, in Python integers and np.float32 scalars"""
    thr = keep_thresholds(k_future)[1] if thr is None else np.float32(thr)
    lo_min = max(t_now - T, 0)

    def lo_of(w):      # first row of the episode world w is sampled from: its current one, or the one that ended in this very step
        if term_t is not None and int(term_t[w]) == t_now:
            return max(int(prev_start[w]), lo_min)
        return max(int(start[w]), lo_min)

    s = (int(seed) * KEY_SEED + int(call) * KEY_CALL + int(b)) & M64
    s, _ = _sm(s)
    w, lo = 0, t_now
    attempt = 0
    while attempt < ATTEMPTS and lo >= t_now:
        s, z = _sm(s)
        w = ((z >> 32) * N) >> 32
        lo = lo_of(w)
        attempt += 1
    probe = 0
    while probe < N and lo >= t_now:
        w = w + 1 if w + 1 < N else 0
        lo = lo_of(w)
        probe += 1
    s, r = _sm(s)
    s, r2 = _sm(s)
    u0, u1, u2 = np.float32(r >> 40) * _INV24, np.float32((r >> 16) & 0xFFFFFF) * _INV24, np.float32(r2 >> 40) * _INV24
    t = lo + int(u0 * np.float32(t_now - lo))      # int(): towards zero, as the device's conversion
    t = min(t, t_now - 1)
    fut = t + 1 + int(u1 * np.float32(t_now - t))
    fut = min(fut, t_now)
    return t, w, (-1 if u2 >= thr else fut), lo < t_now


# ------------------------------------------------------------------------------------------------------------------ the draw, vectorised, in four steps
def her_lo(start, prev_start, term_t, t_now, T):
    """lo [N]: for every world the first row it can be sampled from (GRX_HER_LO); the world has a transition iff lo < t_now"""
    lo_min = max(int(t_now) - int(T), 0)
    first = np.asarray(start, dtype=np.int64)
    if term_t is not None:
        first = np.where(np.asarray(term_t, dtype=np.int64) == t_now, np.asarray(prev_start, dtype=np.int64), first)
    return np.maximum(first, lo_min)


def her_attempts(lo_w, N, t_now, seed, call, b):
    """the up to 64 uniform attempts of every sample: (stream state, world, pending) -- pending: all 64 attempts landed on worlds without a transition"""
    s = her_key(seed, call, b)
    s, _ = splitmix64(s)      # one discarded output
    w = np.zeros(len(s), np.int64)
    active = np.arange(len(s))
    for _ in range(ATTEMPTS):
        if active.size == 0:
            break
        s[active], z = splitmix64(s[active])
        wa = (((z >> _U(32)) * _U(N)) >> _U(32)).astype(np.int64)
        w[active] = wa
        active = active[lo_w[wa] >= t_now]
    pending = np.zeros(len(s), bool)
    pending[active] = True
    return s, w, pending


def her_probe(lo_w, w, t_now, first=1):
    """where the linear probe from world w + first ends: the first of the N worlds w + first, w + first + 1, ... (modulo N) that has a transition, or the last one visited"""
    N = len(lo_w)
    w0 = (np.asarray(w, dtype=np.int64) + first) % N
    have = np.nonzero(lo_w < t_now)[0]
    if have.size == 0:
        return (w0 + N - 1) % N
    k = np.searchsorted(have, w0)
    return np.where(k < have.size, have[np.minimum(k, have.size - 1)], have[0])


def her_uniforms(s):
    """the three 24-bit uniforms of the two outputs that follow state s, as the float32 values the device forms"""
    s, r = splitmix64(s)
    s, r2 = splitmix64(s)
    f = lambda x: x.astype(np.float32) * _INV24      # (x < 2^24: the conversion and the product are exact)
    return f(r >> _U(40)), f((r >> _U(16)) & _U(0xFFFFFF)), f(r2 >> _U(40))


def her_rows_of(lo, t_now, u0, u1):
    """(t, fut): the row uniform in [lo, t_now - 1] and the later row uniform in [t + 1, t_now], float32 products and the two clamps"""
    lo = np.asarray(lo, dtype=np.int64)
    t = lo + (u0 * (t_now - lo).astype(np.float32)).astype(np.int64)      # (astype of a float: towards zero)
    t = np.minimum(t, t_now - 1)
    fut = t + 1 + (u1 * (t_now - t).astype(np.float32)).astype(np.int64)
    return t, np.minimum(fut, t_now)


def ref_her_draw_parts(start, prev_start, term_t, N, t_now, T, seed, call, b):
    """(t, w, fut, u2, found): everything of the draw that does not depend on k_future"""
    lo_w = her_lo(start, prev_start, term_t, t_now, T)
    assert lo_w.shape == (N,)
    s, w, pending = her_attempts(lo_w, N, t_now, seed, call, b)
    w[pending] = her_probe(lo_w, w[pending], t_now)
    lo = lo_w[w]
    u0, u1, u2 = her_uniforms(s)
    t, fut = her_rows_of(lo, t_now, u0, u1)
    return t.astype(np.int32), w.astype(np.int32), fut.astype(np.int32), u2, lo < t_now


def ref_her_draw(start, prev_start, term_t, N, t_now, T, k_future, seed, call, b, thr=None):
    """(t, w, t_goal, found) of the samples b (an int array); thr: the keep threshold, by default the correctly rounded quotient (keep_thresholds)"""
    thr = keep_thresholds(k_future)[1] if thr is None else np.float32(thr)
    t, w, fut, u2, found = ref_her_draw_parts(start, prev_start, term_t, N, t_now, T, seed, call, b)
    return t, w, np.where(u2 >= thr, np.int32(-1), fut).astype(np.int32), found


def matching_thresholds(k_future, fut, u2, t_goal):
    """which of the three candidates explain EVERY decision of one launch (names among "below", "rounded", "above")"""
    return [name for name, thr in zip(("below", "rounded", "above"), keep_thresholds(k_future))
            if np.array_equal(np.where(u2 >= thr, np.int32(-1), fut).astype(np.int32), np.asarray(t_goal, dtype=np.int32))]


# ------------------------------------------------------------------------------------------------------------------ the rows
def her_gather(rows, acts, T, N, W, od, gd, ad, t, w, t_goal, term_rows=None, term_t=None):
    """(r0, r1, goal, action) of every sample: ring row t, the row the action led to (the terminal row where ring row t + 1 is already the first row of the next episode),
    the substituted goal (achieved columns of row t_goal -- of the terminal row when t_goal is that mark -- or the desired columns of row t when t_goal < 0), the action"""
    R = T + 1
    rows, acts = np.asarray(rows, np.float32).reshape(R, N, W), np.asarray(acts, np.float32).reshape(R, N, ad)
    t, w, tg = (np.asarray(x, dtype=np.int64) for x in (t, w, t_goal))
    tt = np.full(len(t), -1, np.int64) if term_t is None else np.asarray(term_t, dtype=np.int64)[w]
    r0 = rows[t % R, w]
    r1 = rows[(t + 1) % R, w]
    goal_row = rows[np.maximum(tg, 0) % R, w]
    if term_t is not None:
        tr = np.asarray(term_rows, np.float32).reshape(N, W)[w]
        r1 = np.where((t + 1 == tt)[:, None], tr, r1)
        goal_row = np.where((tg == tt)[:, None], tr, goal_row)
    goal = np.where((tg < 0)[:, None], r0[:, od + gd:od + 2 * gd], goal_row[:, od:od + gd])
    return r0, r1, goal, acts[(t + 1) % R, w]


def goal_distance(a, b):
    """np.linalg.norm of the fp64 difference of two float32 arrays [..., n]"""
    return np.linalg.norm(np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64), axis=-1)


def ref_her_outcome(ag, g, kind, p0, p1, sparse, ignore_pos=0, ignore_rot=0, ignore_z=0):
    """(reward, success, distances) float32 [B] of the (achieved, goal) pairs; distances: fp64 d for kinds 0 - 2, (d_pos, d_rot) for kind 3"""
    ag, g = np.asarray(ag, np.float32), np.asarray(g, np.float32)
    if kind == 3:
        from gymnasium_robotics_amd.envs.manipulate_spec import block_goal_distance

        dp, dr = block_goal_distance(ag, g, "ignore" if ignore_pos else "random", "ignore" if ignore_rot else "xyz", ignore_z=bool(ignore_z))
        ok = (dp < p0) & (dr < p1)
        reward = (ok.astype(np.float32) - np.float32(1.0)) if sparse else (-(10.0 * dp + dr)).astype(np.float32)
        return reward, ok.astype(np.float32), (dp, dr)
    d = goal_distance(ag, g)
    if kind == 2:
        reward = (d <= p0).astype(np.float32) if sparse else np.exp(-d).astype(np.float32)
        return reward, (d <= p0).astype(np.float32), d
    reward = -((d > p0).astype(np.float32)) if sparse else (-d).astype(np.float32)      # sparse: -0.0 where the goal is reached
    return reward, (d < p0).astype(np.float32), d


def ref_her_rows(rows, acts, T, N, W, od, gd, ad, t, w, t_goal, kind, p0, p1=0.0, sparse=1, ignore_pos=0, ignore_rot=0, ignore_z=0, term_rows=None, term_t=None):
    """[B, OW] float32: [obs_t | achieved_t | goal | action_t | reward | obs_t+1 | achieved_t+1 | success], OW = 2 od + 3 gd + ad + 2"""
    r0, r1, goal, act = her_gather(rows, acts, T, N, W, od, gd, ad, t, w, t_goal, term_rows, term_t)
    reward, success, _ = ref_her_outcome(r1[:, od:od + gd], goal, kind, p0, p1, sparse, ignore_pos, ignore_rot, ignore_z)
    return np.concatenate([r0[:, :od + gd], goal, act, reward[:, None], r1[:, :od + gd], success[:, None]], axis=1).astype(np.float32)


def row_columns(od, gd, ad):
    """(reward column, success column, OW)"""
    return od + 2 * gd + ad, 2 * od + 3 * gd + ad + 1, 2 * od + 3 * gd + ad + 2


# ------------------------------------------------------------------------------------------------------------------ derived bounds
# Dense reward of kinds 0 / 1: float32(-d).  The device and numpy both form d in fp64 from exact differences and exact squares (24-bit inputs), sums of at most 16 terms and one
# square root: they agree to a few fp64 ulps, 2^-29 of a float32 ulp.  The conversion to float32 rounds both to the same value unless a float32 rounding boundary lies between
# them, and then to neighbours: at most ONE float32 ulp of d.
def dense_bound(d):
    return np.spacing(np.asarray(d, dtype=np.float64).astype(np.float32)).astype(np.float64)


# Dense maze reward: expf(-(float)d).  Two steps.  (1) d is rounded to float32: half an ulp, one ulp where the two fp64 distances straddle a boundary as above; exp' = exp, so
# the value moves by at most exp(-d) * ulp32(d).  (2) expf itself: the HIP math library documents 1 ulp for expf, taken here at the result's magnitude with one more ulp for
# the binade edge (the result of step 1 and exp(-d) may lie on either side of a power of two): 2 * ulp32(exp(-d)).
def maze_dense_bound(d):
    d = np.asarray(d, dtype=np.float64)
    e = np.exp(-d)
    return e * np.spacing(d.astype(np.float32)).astype(np.float64) + 2.0 * np.spacing(e.astype(np.float32)).astype(np.float64)


# Kind 3 goes through fp32 atan2f / sqrtf and, with ignore_z, through Euler angles: the tolerances the project already uses for the manipulate reward kernel
# (tests/test_gpu_api.py::test_device_rewards_equal_the_reference_run_vectors).
MANIP_DENSE_ATOL = 1e-3
MANIP_CLEAR_POS, MANIP_CLEAR_ROT = 1e-5, 1e-4      # sparse reward and success are exact for pairs further than this from the two thresholds


# ------------------------------------------------------------------------------------------------------------------ pairs at the threshold distance
PAIR_THRESHOLDS = (0.05, 0.01, 0.45)
PAIRS_PER_THRESHOLD, PAIRS_KEPT = 200000, 4096


def threshold_pairs(dim=3):
    """{thr: (a, b, d)}: 200 000 float32 pairs per threshold whose fp64 distance lies at the threshold -- a uniform in [-1, 1)^dim, b = float32(a + u * thr) for a unit vector
    u -- from ONE generator of seed 0 walked through the thresholds in the order of PAIR_THRESHOLDS; d: the fp64 distance of the two float32 vectors"""
    rng = np.random.default_rng(0)
    out = {}
    for thr in PAIR_THRESHOLDS:
        n = PAIRS_PER_THRESHOLD
        a = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        u = rng.standard_normal((n, dim))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        b = (a.astype(np.float64) + u * thr).astype(np.float32)
        out[thr] = (a, b, goal_distance(a, b))
    return out


def nearest_pairs(a, b, d, thr, keep=PAIRS_KEPT):
    """the `keep` pairs nearest the threshold on either side of it: (a, b, d) of 2 * keep pairs, those beyond the threshold first"""
    above, below = np.nonzero(d > thr)[0], np.nonzero(d <= thr)[0]
    assert len(above) >= keep and len(below) >= keep
    sel = np.concatenate([above[np.argsort(d[above] - thr, kind="stable")[:keep]], below[np.argsort(thr - d[below], kind="stable")[:keep]]])
    return a[sel], b[sel], d[sel]


def distance_fp32(a, b):
    """the distance a float32 evaluation gives (the mistake the threshold pairs are there to catch)"""
    df = np.asarray(a, np.float32) - np.asarray(b, np.float32)
    return np.sqrt((df * df).sum(axis=-1, dtype=np.float32))
