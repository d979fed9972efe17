"""Plain numpy / Python restatements of the episode store (include/grx_capi.h: grx_her_archive, grx_her_episode_sample): which words a finished episode leaves in which
slot, which (slot, transition, goal row) a given (seed, call, sample) must draw from a store, and which packed replay row that draw must produce.  Nothing here imports
torch or the native library.  The draw is stated twice -- ref_episode_draw_scalar, one sample in Python integers, line for line what the device function does, and
ref_episode_draw, the same over an array of samples, put together from the small steps below so that tests/test_cpu_episode_refs.py can swap one step for a wrong one.
Rewards and success flags are her_refs.ref_her_outcome's, with the bounds derived there."""
import numpy as np

import her_refs as R

DOMAIN = 0x455049534F444553      # xor-ed into the sample key: the store's stream never coincides with the ring's
FUTURE, FINAL, EPISODE = 0, 1, 2
_U = np.uint64
_INV24 = np.float32(1.0 / 16777216.0)


# ------------------------------------------------------------------------------------------------------------------ the store
def empty_store(E, T, W, ad, fill=0.0, fill_meta=0):
    """the four parts of a store of E slots as host arrays; count is a Python integer"""
    return dict(rows=np.full((E, T + 1, W), fill, np.float32), acts=np.full((E, T + 1, ad), fill, np.float32), meta=np.full((E, 4), fill_meta, np.int32), count=0)


def ref_archive(store, ring_rows, ring_acts, start, t_prev, T, lst, k, final_rows=None, compact=False, step_action=None):
    """grx_her_archive in plain slicing, on the store in place.  ring_rows [T+1, N, W], ring_acts [T+1, N, ad]: the ring BEFORE row t_prev + 1 is appended; start [N]: the
    episode marks before the worlds of this step are re-marked; lst[:k]: the worlds whose episode ended; final_rows: the terminal rows, row j of list position j (compact)
    or of world lst[j], with step_action [N, ad]"""
    Rn, N = T + 1, ring_rows.shape[1]
    E = len(store["meta"])
    k = min(max(int(k), 0), N)
    s = 0 if final_rows is None else 1
    before = int(store["count"])
    for j in range(k):
        w, slot = int(lst[j]), (before + j) % E
        if not 0 <= w < N:      # not a world: the slot is taken and left empty
            store["meta"][slot] = (0, w, 0, 0)
            continue
        a0 = max(int(start[w]), t_prev - T + s, 0)
        L = max(t_prev - a0 + s, 0)
        store["meta"][slot] = (L, w, a0, 0)
        if L == 0:
            continue
        n = t_prev - a0 + 1      # rows of the episode that are in the ring
        ring = (a0 + np.arange(n)) % Rn
        store["rows"][slot, :n] = ring_rows[ring, w]
        store["acts"][slot, 0] = 0.0
        store["acts"][slot, 1:n] = ring_acts[ring[1:], w]
        if s:
            store["rows"][slot, L] = final_rows[j if compact else w]
            store["acts"][slot, L] = step_action[w]
    store["count"] = before + k
    return store


# ------------------------------------------------------------------------------------------------------------------ the draw, one sample, line for line
def _sm(s):
    s = (s + 0x9E3779B97F4A7C15) & R.M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
    return s, z ^ (z >> 31)


def ref_episode_draw_scalar(lens, count, E, strategy, k_future, seed, call, b):
    """(slot, t, goal row or -1 = the episode's own goal, found) of ONE sample b, in Python integers and np.float32 scalars; lens: ep_meta[:, 0]"""
    s = ((((int(seed) * R.KEY_SEED + int(call) * R.KEY_CALL) & R.M64) ^ DOMAIN) + int(b)) & R.M64
    s, _ = _sm(s)
    F = min(max(int(count), 0), int(E))
    if F == 0:
        return 0, 0, -1, False
    e, L, attempt = 0, 0, 0
    while attempt < R.ATTEMPTS and L <= 0:
        s, z = _sm(s)
        e = ((z >> 32) * F) >> 32
        L = int(lens[e])
        attempt += 1
    probe = 0
    while probe < F and L <= 0:
        e = e + 1 if e + 1 < F else 0
        L = int(lens[e])
        probe += 1
    if L <= 0:
        return 0, 0, -1, False
    s, r = _sm(s)
    s, r2 = _sm(s)
    u0, u1 = np.float32(r >> 40) * _INV24, np.float32((r >> 16) & 0xFFFFFF) * _INV24
    t = min(int(u0 * np.float32(L)), L - 1)      # int(): towards zero, as the device's conversion
    if strategy == FINAL:
        g = L
    elif strategy == EPISODE:
        g = min(int(u1 * np.float32(L + 1)), L)
    else:
        g = min(t + 1 + int(u1 * np.float32(L - t)), L)
    keep = (r2 >> 40) * (k_future + 1) >= (k_future << 24)      # integers: no fp32 quotient
    return e, t, (-1 if keep else g), True


# ------------------------------------------------------------------------------------------------------------------ the draw, vectorised, in steps
def episode_key(seed, call, b):
    base = ((int(seed) * R.KEY_SEED + int(call) * R.KEY_CALL) & R.M64) ^ DOMAIN
    with np.errstate(over="ignore"):
        return _U(base) + np.atleast_1d(np.asarray(b)).astype(np.uint64)


def episode_attempts(lens, F, seed, call, b):
    """the up to 64 uniform attempts of every sample: (stream state, slot, pending) -- pending: all 64 attempts landed on empty slots"""
    with np.errstate(over="ignore"):
        s = episode_key(seed, call, b)
        s, _ = R.splitmix64(s)
        e = np.zeros(len(s), np.int64)
        active = np.arange(len(s))
        for _ in range(R.ATTEMPTS):
            if active.size == 0:
                break
            s[active], z = R.splitmix64(s[active])
            ea = (((z >> _U(32)) * _U(F)) >> _U(32)).astype(np.int64)
            e[active] = ea
            active = active[lens[ea] <= 0]
    pending = np.zeros(len(s), bool)
    pending[active] = True
    return s, e, pending


def episode_probe(lens, e, F, modulo=None):
    """where the linear probe from slot e + 1 ends: the first of the slots e + 1, e + 2, ... (modulo F) that holds an episode, or the last one visited"""
    modulo = F if modulo is None else modulo
    e0 = (np.asarray(e, dtype=np.int64) + 1) % modulo
    have = np.nonzero(lens[:modulo] > 0)[0]
    if have.size == 0:
        return (e0 + modulo - 1) % modulo
    k = np.searchsorted(have, e0)
    return np.where(k < have.size, have[np.minimum(k, have.size - 1)], have[0])


def episode_uniforms(s):
    """(u0, u1) as the float32 values the device forms and m2 = r2 >> 40 as an integer, from the two outputs that follow state s"""
    with np.errstate(over="ignore"):
        s, r = R.splitmix64(s)
        s, r2 = R.splitmix64(s)
    f = lambda x: x.astype(np.float32) * _INV24
    return f(r >> _U(40)), f((r >> _U(16)) & _U(0xFFFFFF)), (r2 >> _U(40)).astype(np.int64)


def episode_rows_of(L, u0, u1, strategy):
    """(t, g): the transition uniform in [0, L - 1] and the goal row of the strategy, float32 products and the clamps"""
    L = np.asarray(L, dtype=np.int64)
    t = np.minimum((u0 * L.astype(np.float32)).astype(np.int64), L - 1)
    if strategy == FINAL:
        g = L.copy()
    elif strategy == EPISODE:
        g = np.minimum((u1 * (L + 1).astype(np.float32)).astype(np.int64), L)
    else:
        g = np.minimum(t + 1 + (u1 * (L - t).astype(np.float32)).astype(np.int64), L)
    return t, g


def episode_keep(m2, k_future):
    """keep the episode's own goal: m2 (k + 1) >= k 2^24, in integers"""
    return m2 * (int(k_future) + 1) >= (int(k_future) << 24)


def ref_episode_draw(lens, count, E, strategy, k_future, seed, call, b):
    """(slot, t, goal row or -1, found) of the samples b (an int array), int32"""
    b = np.atleast_1d(np.asarray(b))
    lens = np.asarray(lens, dtype=np.int64)
    F = min(max(int(count), 0), int(E))
    none = (np.zeros(len(b), np.int32), np.zeros(len(b), np.int32), np.full(len(b), -1, np.int32), np.zeros(len(b), bool))
    if F == 0 or not (lens[:F] > 0).any():
        return none
    s, e, pending = episode_attempts(lens, F, seed, call, b)
    e[pending] = episode_probe(lens, e[pending], F)
    u0, u1, m2 = episode_uniforms(s)
    t, g = episode_rows_of(lens[e], u0, u1, strategy)
    g = np.where(episode_keep(m2, k_future), -1, g)
    return e.astype(np.int32), t.astype(np.int32), g.astype(np.int32), np.ones(len(b), bool)


# ------------------------------------------------------------------------------------------------------------------ the rows
def episode_gather(ep_rows, ep_acts, od, gd, e, t, g):
    """(r0, r1, goal, action) of every draw"""
    e, t, g = (np.asarray(x, dtype=np.int64) for x in (e, t, g))
    r0, r1 = ep_rows[e, t], ep_rows[e, t + 1]
    goal = np.where((g < 0)[:, None], r0[:, od + gd:od + 2 * gd], ep_rows[e, np.maximum(g, 0)][:, od:od + gd])
    return r0, r1, goal, ep_acts[e, t + 1]


def ref_episode_rows(ep_rows, ep_acts, od, gd, ad, e, t, g, kind, p0, p1=0.0, sparse=1, ignore_pos=0, ignore_rot=0, ignore_z=0, found=None):
    """[B, OW] float32: [obs_t | achieved_t | goal | action_t | reward | obs_t+1 | achieved_t+1 | success]; rows of draws that found nothing are zero"""
    r0, r1, goal, act = episode_gather(ep_rows, ep_acts, od, gd, e, t, g)
    reward, success, _ = R.ref_her_outcome(r1[:, od:od + gd], goal, kind, p0, p1, sparse, ignore_pos, ignore_rot, ignore_z)
    out = np.concatenate([r0[:, :od + gd], goal, act, reward[:, None], r1[:, :od + gd], success[:, None]], axis=1).astype(np.float32)
    if found is not None:
        out[~np.asarray(found, bool)] = 0.0
    return out
