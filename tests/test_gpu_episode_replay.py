"""The episode store end to end: EpisodicHerReplay (gymnasium_robotics_amd/her.py) around a device environment against a store kept on the host by plain slicing
(tests/episode_refs.py), and the store of the env-level C ABI (include/grx_episodes.h, libgrx_env.so) against the Python class, run beside each other with the same seeds
and actions.  64 worlds, a time limit and horizon of 5, 24 steps, the worlds staggered (so the first episodes are partial: begin finds non-zero elapsed counters and the
episode marks start negative).  Comparison is exact (float32 bit patterns) except dense rewards, which take the bounds of tests/her_refs.py.

One documented difference is applied by hand: before anything has been archived EpisodicHerReplay.sample returns an empty view and advances nothing, grx_episodes_sample
writes a zero batch with valid[0] = 0 and advances its call counter.  Both sides are therefore reseeded before every sample."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import episode_refs as P
import test_cpu_episode_refs as C
import test_gpu_env_replay as H
import test_gpu_episode_refs as G

pytestmark = pytest.mark.gpu
N, T, STEPS, BATCH = 64, 5, 24, 257
SLOTS = 96      # fewer than the episodes that end in 24 steps: the slots wrap
FETCH_IDS = ["FetchReach-v4", "FetchPickAndPlaceDense-v4"]
MAZE_ID = "PointMaze_UMaze-v3"
STRATEGY_NAMES = ["future", "final", "episode"]


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    """the default launch group on both sides: no experiment switch of the Python environment is set"""
    for k in list(os.environ):
        if k.startswith("GRX_"):
            monkeypatch.delenv(k)


def _E():
    from gymnasium_robotics_amd import env_capi

    return env_capi


class Store:
    """a grx_episodes store attached to a test_gpu_env_replay.Replay; device pointers as torch views"""

    def __init__(self, rp, episodes, max_batch=BATCH, seed=9):
        E = _E()
        self.rp, self.L, self.c = rp, rp.L, rp.c
        cfg = E.EpisodesConfig(episodes=episodes, max_batch=max_batch, seed=seed)
        self.p = ctypes.c_void_p()
        E.check(self.L.grx_episodes_create(rp.r, ctypes.byref(cfg), ctypes.byref(self.p)))
        d = [ctypes.c_int() for _ in range(4)]
        E.check(self.L.grx_episodes_dims(self.p, *[ctypes.byref(x) for x in d]))
        self.dims = tuple(x.value for x in d)      # row_width, horizon, packed_width, act_dim

    def sample(self, batch, k, strategy):
        E = _E()
        b = E.EpisodesBatch()
        E.check(self.L.grx_episodes_sample(self.p, batch, k, strategy, ctypes.byref(b), self.c.stream()))
        assert b.batch == batch
        return E.device_view(b.rows, (batch, self.dims[0])), E.device_view(b.valid, (1,), np.int32)

    def reseed(self, seed):
        return self.L.grx_episodes_reseed(self.p, seed)

    def views(self):
        E = _E()
        rows, acts, meta, count, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        E.check(self.L.grx_episodes_store(self.p, ctypes.byref(rows), ctypes.byref(acts), ctypes.byref(meta), ctypes.byref(count), ctypes.byref(n)))
        ow, hz, w, ad = self.dims
        return (E.device_view(rows.value, (n.value, hz + 1, w)), E.device_view(acts.value, (n.value, hz + 1, ad)), E.device_view(meta.value, (n.value, 4), np.int32),
                E.device_view(count.value, (1,), np.int64))

    def close(self):
        if self.p:
            _E().check(self.L.grx_episodes_destroy(self.p))
            self.p = None


def _host_store(views):
    rows, acts, meta, count = (v.detach().cpu().numpy() for v in views)
    return dict(rows=rows, acts=acts, meta=meta, count=int(count[0]))


def _stores_equal(a, b):
    return a["count"] == b["count"] and np.array_equal(a["meta"], b["meta"]) and G._same(a["rows"], b["rows"]) and G._same(a["acts"], b["acts"])


def _stagger(env, c):
    phase = (np.arange(N) * 3) % T      # world i is at step 3 i mod 5 of its episode
    env._elapsed[:] = phase
    if c is not None:
        c.set_elapsed(phase)
    return phase


# ================================================================================================================== the Python class against plain slicing
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("env_id", FETCH_IDS)
def test_python_store_is_the_sliced_store_and_samples_are_the_reference_rows(env_id, mode):
    """after every step the packed rows, the actions, the mask and the terminal rows are copied to the host, the expected store is kept there by ref_archive (plain slicing
    of a host ring), and the whole device store is compared with it; then 257 rows of every strategy against ref_episode_rows of ref_episode_draw"""
    import torch
    from gymnasium_robotics_amd.her import EpisodicHerReplay

    env = H._fetch_env(env_id, N, mode, T)
    try:
        env.reset(seed=7)
        phase = _stagger(env, None)
        buf = EpisodicHerReplay(env, horizon=T, capacity=1024, episodes=SLOTS, seed=5, continuous=True)
        buf.begin_episode(env.packed)
        buf.set_episode_start(-env._elapsed)
        W, ad = buf.W, buf.act_dim
        c = dict(od=buf.obs_dim, gd=buf.goal_dim, ad=ad, W=W, ignore_pos=0, ignore_rot=0, ignore_z=0)
        c.update(buf.spec)
        want = P.empty_store(SLOTS, T, W, ad)
        ring_rows, ring_acts = np.zeros((T + 1, N, W), np.float32), np.zeros((T + 1, N, ad), np.float32)
        ring_rows[0], start, t = env.packed.cpu().numpy(), -phase.astype(np.int64), 0
        assert (start < 0).any()      # partial episodes: under way at row 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)
        worst, sampled, seen = G.Worst(), 0, set()
        for step in range(STEPS):
            pending = env._needs_reset.copy()
            a = torch.rand(N, 4, device="cuda:0", generator=gen) * 2 - 1
            _, _, te, tr, _ = env.step(a)
            done = te.numpy().astype(bool) | tr.numpy().astype(bool)
            mask = done if mode == "same_step" else pending
            count, lst = int(mask.sum()), env.step_reset_list
            order = lst[0][:count].cpu().numpy() if (count and lst is not None and lst[1] == count) else np.nonzero(mask)[0]
            assert sorted(order.tolist()) == np.nonzero(mask)[0].tolist()
            packed, acts_h = env.packed.cpu().numpy(), a.cpu().numpy()
            final = env.final_packed.cpu().numpy() if mode == "same_step" else None
            buf.append(a, env.packed, mask, final_rows=env.final_packed if mode == "same_step" else None)
            P.ref_archive(want, ring_rows, ring_acts, start, t, T, order, count, final, False, acts_h if final is not None else None)
            t += 1
            ring_rows[t % (T + 1)], ring_acts[t % (T + 1)] = packed, acts_h
            start[mask] = t
            assert buf.archived == want["count"]
            seen |= set(want["meta"][:, 0].tolist())
            got = _host_store(buf.store_views())
            assert _stores_equal(got, want), (step, int((got["meta"] != want["meta"]).sum()))
            for s, name in enumerate(STRATEGY_NAMES):
                buf.reseed_samples(3000 + 3 * step + s)
                rows = buf.sample(BATCH, 4, name)
                if want["count"] == 0:
                    assert len(rows) == 0
                    continue
                found = G._compare_rows(rows.cpu().numpy(), c, (want["rows"], want["acts"]), want["meta"][:, 0], want["count"], s, 4, 3000 + 3 * step + s, 0, BATCH, worst,
                                        (step, name))
                assert found.all() and int(buf._sample_valid.item()) == BATCH
                sampled += 1
        assert want["count"] > SLOTS and sampled > 30 and T in seen and any(0 < x < T for x in seen), seen      # the slots wrapped; whole and partial episodes were stored
        worst.report()
    finally:
        env.close()


# ================================================================================================================== the handle against the Python class
def _pair(env, c, mode, keep_final, maze, act_fn, obs):
    """STEPS x (env.step + EpisodicHerReplay.append + sample | grx_env_step + grx_replay_append + grx_episodes_sample): every batch compared, the whole store at the end"""
    import torch
    from gymnasium_robotics_amd.her import EpisodicHerReplay

    buf = EpisodicHerReplay(env, horizon=T, capacity=1024, episodes=SLOTS, seed=5, continuous=True)
    rp = H.Replay(c, T, 1024, seed=5, keep_final=keep_final, max_batch=256)
    st = Store(rp, SLOTS)
    try:
        assert st.dims == (buf.OW, T, buf.W, buf.act_dim)
        buf.begin_episode(env.packed)
        buf.set_episode_start(-env._elapsed)
        assert rp.begin() == 0, c.err()
        od, gd, W = buf.obs_dim, buf.goal_dim, buf.W
        track = mode == "same_step" and keep_final
        term = torch.zeros(N, W, device="cuda:0") if (maze and track) else None
        empty = batches = terminated = 0
        for t in range(STEPS):
            pending = env._needs_reset.copy()
            a = act_fn(t, obs)
            obs, _, te, tr, info = env.step(a)
            assert c.step(a) == 0, c.err()
            done = te.numpy().astype(bool) | tr.numpy().astype(bool)
            terminated += int(te.numpy().astype(bool).sum())
            if track and maze:      # a world-indexed buffer of whole terminal rows, put together from what the step returned
                if done.any():
                    ti, fo = torch.from_numpy(np.nonzero(done)[0]).to("cuda:0"), info["final_obs"]
                    term[ti, :od], term[ti, od: od + gd], term[ti, od + gd: od + 2 * gd] = fo["observation"], fo["achieved_goal"], fo["desired_goal"]
                    term[ti, W - 2:] = env.packed[ti, W - 2:]      # (same-step: the reset row keeps the finished episode's reward and success words)
                buf.append(a, env.packed, done, final_rows=term)
            elif track:
                buf.append(a, env.packed, done, final_rows=env.final_packed)
            else:
                buf.append(a, env.packed, done if mode == "same_step" else pending)
            assert rp.append() == 0, c.err()
            for s, name in enumerate(STRATEGY_NAMES):
                buf.reseed_samples(1000 + 3 * t + s)
                assert st.reseed(1000 + 3 * t + s) == 0
                want = buf.sample(BATCH, 4, name)
                rows, valid = st.sample(BATCH, 4, s)
                torch.cuda.synchronize()
                if len(want) == 0:      # nothing archived yet: the Python class launches nothing
                    empty += 1
                    assert int(valid.item()) == 0 and not H._bits(rows).any(), t
                else:      # (valid is 0 here too while every archived episode is empty: worlds that ended with no transition in the ring)
                    ok = int(buf._sample_valid.item())
                    batches += ok == BATCH
                    assert ok in (0, BATCH) and int(valid.item()) == ok and np.array_equal(H._bits(rows), H._bits(want)), (t, name)
        got, want = _host_store(st.views()), _host_store(buf.store_views())
        assert want["count"] == buf.archived > SLOTS and batches > 30
        assert _stores_equal(got, want), int((got["meta"] != want["meta"]).sum())
        lens = want["meta"][:, 0]
        assert (lens > 0).any() and (lens <= T).all()
        return dict(empty=empty, batches=batches, terminated=terminated, lens=np.bincount(lens, minlength=T + 1).tolist())
    finally:
        st.close()
        rp.close()


@pytest.mark.parametrize("keep_final", [0, 1])
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("env_id", FETCH_IDS)
def test_fetch_handle_store_is_the_python_store_bit_for_bit(env_id, mode, keep_final, tmp_path):
    import torch

    env, c = H._fetch_env(env_id, N, mode, T), H.Handle(env_id, N, tmp_path, mode, T)
    try:
        env.reset(seed=7)
        assert c.reset(seeds=7 + np.arange(N)) == 0
        _stagger(env, c)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)
        stats = _pair(env, c, mode, keep_final, False, lambda t, obs: torch.rand(N, 4, device="cuda:0", generator=gen) * 2 - 1, None)
        print(env_id, mode, keep_final, stats)
    finally:
        c.close()
        env.close()


@pytest.mark.parametrize("keep_final", [0, 1])
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("kw", list(H.MODE_SETS.values()), ids=list(H.MODE_SETS))
def test_maze_handle_store_is_the_python_store_bit_for_bit(kw, mode, keep_final, tmp_path):
    """default (host bookkeeping), continuing_task=False (the list of ended worlds and its length exist in device memory only) and reset_target=True.  With
    continuing_task=False the start and goal noise is widened to a whole cell, so that some worlds start inside the goal radius and end in their first step: episodes of
    different lengths (the recipe of test_gpu_env_replay.ANT_EPISODIC_NOISE)"""
    import torch

    episodic = kw.get("continuing_task") is False
    if episodic:
        kw = dict(kw, position_noise_range=1.0)
    env, c = H._maze_env(MAZE_ID, N, mode, T, **kw), H.Handle(MAZE_ID, N, tmp_path, mode, T, **kw)
    try:
        obs, _ = env.reset(seed=7)
        assert c.reset(seeds=7 + np.arange(N)) == 0
        _stagger(env, c)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)

        def act(t, obs):
            a = torch.rand(N, env.nu, device="cuda:0", generator=gen) * 2 - 1
            a[: N // 2] = torch.clamp(4.0 * (obs["desired_goal"] - obs["achieved_goal"]) - obs["observation"][:, 2:4], -1.0, 1.0)[: N // 2]
            return a.float().contiguous()

        stats = _pair(env, c, mode, keep_final, True, act, obs)
        print(MAZE_ID, kw, mode, keep_final, stats)
        assert not episodic or stats["terminated"] >= 1, stats      # episodes ended on the device's word, not only by the time limit
    finally:
        c.close()
        env.close()


# ================================================================================================================== a store changes nothing else
@pytest.mark.parametrize("mode,keep_final", [("same_step", 1), ("next_step", 0)])
def test_ring_and_relabel_are_untouched_by_a_store(mode, keep_final, tmp_path):
    """two handles with the same seeds and actions, one with a store attached: every relabel batch and the replay ring at the end are bit-identical"""
    import torch

    env_id = "FetchPickAndPlaceDense-v4"
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ca, cb = H.Handle(env_id, N, tmp_path / "a", mode, T), H.Handle(env_id, N, tmp_path / "b", mode, T)
    ra, rb = H.Replay(ca, T, 4 * 256 + 7, seed=5, keep_final=keep_final, max_batch=256), H.Replay(cb, T, 4 * 256 + 7, seed=5, keep_final=keep_final, max_batch=256)
    st = Store(rb, SLOTS)
    try:
        for c, r in ((ca, ra), (cb, rb)):
            assert c.reset(seeds=7 + np.arange(N)) == 0
            c.set_elapsed((np.arange(N) * 3) % T)
            assert r.begin() == 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)
        for t in range(STEPS):
            a = torch.rand(N, 4, device="cuda:0", generator=gen) * 2 - 1
            assert ca.step(a) == 0 and cb.step(a) == 0 and ra.append() == 0 and rb.append() == 0, (ca.err(), cb.err())
            st.sample(BATCH, 4, t % 3)
            (rows_a, valid_a, off_a), (rows_b, valid_b, off_b) = ra.relabel(256), rb.relabel(256)
            torch.cuda.synchronize()
            assert off_a == off_b and int(valid_a.item()) == int(valid_b.item()) and np.array_equal(H._bits(rows_a), H._bits(rows_b)), t
        (ring_a, head_a, size_a), (ring_b, head_b, size_b) = ra.ring(), rb.ring()
        assert (head_a, size_a) == (head_b, size_b) and np.array_equal(H._bits(ring_a), H._bits(ring_b))
        assert int(st.views()[3].item()) > SLOTS
    finally:
        st.close()
        ra.close()
        rb.close()
        ca.close()
        cb.close()


def test_partial_episodes_keep_what_the_ring_saw(tmp_path):
    """begin on a batch with non-zero elapsed counters: the first episode of a world that was e steps into it is stored with T - e transitions from row 0 (+ nothing
    before begin), the ones after it whole"""
    import torch

    c = H.Handle("FetchReach-v4", N, tmp_path, "same_step", T)
    rp = H.Replay(c, T, 1024, keep_final=1, max_batch=256)
    st = Store(rp, 4 * N)
    try:
        assert c.reset(seeds=np.arange(N)) == 0
        phase = (np.arange(N) * 3) % T
        c.set_elapsed(phase)
        assert rp.begin() == 0
        a = torch.zeros(N, 4, device="cuda:0")
        for _ in range(2 * T):
            assert c.step(a) == 0 and rp.append() == 0, c.err()
        torch.cuda.synchronize()
        s = _host_store(st.views())
        assert s["count"] == 2 * N
        meta = s["meta"][:2 * N]
        for w in range(N):
            mine = meta[meta[:, 1] == w]
            assert mine[:, 0].tolist() == [T - phase[w], T] and mine[:, 2].tolist() == [0, T - phase[w]], (w, mine)
    finally:
        st.close()
        rp.close()
        c.close()


# ================================================================================================================== no call waits
def test_append_with_a_store_and_sample_do_not_wait_for_the_device(tmp_path):
    """the method and the size of test_gpu_env_replay.test_append_and_relabel_do_not_wait_for_the_device (8 192 ants, continuing_task=False: the worlds a step ended are
    known to the device alone), ten step + append + sample groups enqueued back to back: the stream still has work queued when the last call returns"""
    import torch

    n = 8192
    c = H.Handle("AntMaze_Large_Diverse_GR-v5", n, tmp_path, "same_step", 40, continuing_task=False)
    rp = H.Replay(c, 40, 8 * n, seed=1, keep_final=1, max_batch=4 * n)
    st = Store(rp, n, max_batch=4 * n)
    try:
        assert c.reset(seeds=np.arange(n)) == 0
        c.set_elapsed((np.arange(n) * 7) % 40)      # some episodes end in every step
        assert rp.begin() == 0
        a = torch.rand(n, c.act_dim, device="cuda:0") * 2 - 1
        assert c.step(a) == 0 and rp.append() == 0
        st.sample(4 * n, 4, 0)
        torch.cuda.synchronize()
        for _ in range(10):
            assert c.step(a) == 0 and rp.append() == 0, c.err()
            rows, valid = st.sample(4 * n, 4, 0)
        busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        assert busy, "the stream was idle when the tenth grx_episodes_sample returned: a call waited for the device"
        assert int(valid.item()) == 4 * n and np.isfinite(rows.cpu().numpy()).all()
        assert int(st.views()[3].item()) >= 10 * (n // 40)
    finally:
        st.close()
        rp.close()
        c.close()


# ================================================================================================================== errors
def test_ordering_and_argument_errors(tmp_path):
    import torch

    E = _E()
    c = H.Handle("FetchReach-v4", N, tmp_path, "same_step", T)
    rp = H.Replay(c, T, 1024, max_batch=256)
    L = c.L
    p = ctypes.c_void_p()
    try:
        few = E.EpisodesConfig(episodes=N - 1, max_batch=64, seed=0)
        assert L.grx_episodes_create(rp.r, ctypes.byref(few), ctypes.byref(p)) == -1 and f"episodes {N - 1} is less than the number of worlds {N}" in c.err() and not p.value
        st = Store(rp, N, max_batch=64)
        try:
            good = E.EpisodesConfig(episodes=N, max_batch=64, seed=0)
            assert L.grx_episodes_create(rp.r, ctypes.byref(good), ctypes.byref(p)) == -1 and "already has a store" in c.err()
            assert L.grx_replay_destroy(rp.r) == -1 and "episode store is attached" in c.err() and "grx_episodes_destroy" in c.err()
            b = E.EpisodesBatch()
            assert L.grx_episodes_sample(st.p, 0, 4, 0, ctypes.byref(b), None) == -1 and "batch 0" in c.err()
            assert L.grx_episodes_sample(st.p, 65, 4, 0, ctypes.byref(b), None) == -1 and "larger than max_batch 64" in c.err()
            assert L.grx_episodes_sample(st.p, 64, -1, 0, ctypes.byref(b), None) == -1 and "negative k_future" in c.err()
            assert L.grx_episodes_sample(st.p, 64, 4, 3, ctypes.byref(b), None) == -1 and "unknown strategy 3" in c.err()
            # the replay and the store are still whole: a sample before anything was archived reports nothing, begin keeps the store
            a = torch.zeros(N, 4, device="cuda:0")
            assert c.reset(seeds=np.arange(N)) == 0 and rp.begin() == 0
            rows, valid = st.sample(64, 4, 0)
            torch.cuda.synchronize()
            assert int(valid.item()) == 0 and not H._bits(rows).any()
            for _ in range(T):
                assert c.step(a) == 0 and rp.append() == 0, c.err()
            assert rp.begin() == 0
            rows, valid = st.sample(64, 4, 1)
            torch.cuda.synchronize()
            assert int(valid.item()) == 64 and int(st.views()[3].item()) == N
        finally:
            st.close()
    finally:
        rp.close()      # (possible again once the store is gone)
        c.close()


# ================================================================================================================== the C example
def test_c99_episodes_example_matches_ctypes(tmp_path):
    import torch

    E = _E()
    E.lib()
    exe = tmp_path / "episodes_rollout"
    subprocess.check_call(C.example_build_line(exe))
    env_id, n, steps = "FetchPickAndPlace-v4", 64, 60
    desc = E.write_env_desc(env_id, str(tmp_path / "pick.grxenv"))
    res = subprocess.run(["timeout", "-k", "10", "300", str(exe), desc, str(n), str(steps)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split() for line in res.stdout.strip().splitlines())
    c = H.Handle(env_id, n, tmp_path, "same_step", 25)
    batch = 4 * n
    rp = H.Replay(c, 25, 16 * batch, seed=5, keep_final=1, max_batch=batch)
    st = Store(rp, 2 * n, max_batch=batch, seed=9)
    try:
        assert c.reset(seeds=1000 + np.arange(n)) == 0 and rp.begin() == 0
        i, j = np.meshgrid(np.arange(n), np.arange(4), indexing="ij")
        for t in range(steps):
            a = torch.from_numpy((((t * 11 + i * 7 + j * 3) % 17) / 8.0 - 1.0).astype(np.float32)).cuda()
            assert c.step(a) == 0 and rp.append() == 0
            rows, valid = st.sample(batch, 4, t % 3)
        torch.cuda.synchronize()
        assert int(lines["row_width"]) == st.dims[0] == 2 * c.obs_dim + 3 * 3 + 4 + 2
        assert int(lines["valid"]) == int(valid.item()) == batch
        assert int(lines["checksum"], 16) == H._fnv1a(rows.cpu().numpy().tobytes())
    finally:
        st.close()
        rp.close()
        c.close()
