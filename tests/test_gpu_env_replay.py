"""The HER replay of the env-level C ABI (include/grx_replay.h, libgrx_env.so) against the Python path it restates: the Python environment with
HerReplay(env, horizon, capacity, seed, continuous=True) around it, run beside the handle with the same seeds and the same actions.  Comparison is exact (tolerance 0,
np.array_equal on the float32 bit patterns): both sides run the same device arithmetic on identical inputs with the same counter-based draws.  Compared: the relabelled
batch of every step and, at the end, the whole replay ring with its head and size.

The one documented difference is applied to the Python side by hand (_py_relabel): when no world has a transition to sample HerReplay.relabel returns an empty view and
advances nothing, grx_replay_relabel takes the slot, zero-fills it and reports valid[0] = 0.  The call counters of the two index streams then differ (the library's
advances on every call), so the runs in which that can happen drive both sides with an explicit reseed before every relabel (seed 1000 + t, call counter 0); the
staggered Fetch runs, where some world always has a transition, let the two counters run."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FETCH_IDS = [f"{t}{d}-v4" for t in ("FetchReach", "FetchPush", "FetchSlide", "FetchPickAndPlace") for d in ("", "Dense")]
# a point mass that can be steered to its goal inside a short episode, and the ant; sparse and dense ids of each
POINT_IDS = ["PointMaze_Open_Diverse_G-v3", "PointMaze_Open_Diverse_GDense-v3"]
ANT_IDS = ["AntMaze_UMaze-v5", "AntMaze_UMazeDense-v5"]
MODE_SETS = {"default": {}, "episodic": {"continuing_task": False}, "reset_target": {"reset_target": True}}
# The ant cannot be steered 2 m (the least distance between a reset position and a goal at the default noise) inside an episode by any simple controller.  With the
# description's position_noise_range at 1.0 (4 m either way on both the goal and the start, cells 4 m apart) about one start in 150 lies inside the goal radius, and
# that world terminates in its first step whatever the actions are: that is how the ant runs with continuing_task=False get episodes that end by termination.
ANT_EPISODIC_NOISE = 1.0


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    """the default launch group on both sides: no experiment switch of the Python environment is set"""
    for k in list(os.environ):
        if k.startswith("GRX_"):
            monkeypatch.delenv(k)


def _E():
    from gymnasium_robotics_amd import env_capi

    return env_capi


class Handle:
    """a grx_env handle of either family (test plumbing only)"""

    def __init__(self, env_id, n, tmp_path, mode="next_step", horizon=50, **kw):
        import torch

        E = _E()
        self.L, self.n = E.lib(), n
        tag = "_".join(f"{k}{v}" for k, v in sorted(kw.items()))
        path = E.write_env_desc(env_id, str(tmp_path / f"{env_id}{tag}.grxenv"), **kw)
        cfg = E.EnvConfig(E.AUTORESET[mode], horizon, 0)
        self.h = ctypes.c_void_p()
        E.check(self.L.grx_env_create(path.encode(), n, 0, ctypes.byref(cfg), ctypes.byref(self.h)))
        od, gd, ad, dt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        E.check(self.L.grx_env_dims(self.h, ctypes.byref(od), ctypes.byref(gd), ctypes.byref(ad), ctypes.byref(dt)))
        self.obs_dim, self.goal_dim, self.act_dim = od.value, gd.value, ad.value
        self.width = self.obs_dim + 2 * self.goal_dim + 2
        self.stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def err(self):
        return self.L.grx_env_last_error().decode()

    def reset(self, seeds=None, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        return self.L.grx_env_reset(self.h, None if m is None else m.ctypes.data, None if s is None else s.ctypes.data, self.stream())

    def step(self, actions):
        return self.L.grx_env_step(self.h, actions.data_ptr(), self.stream())

    def state(self):
        E = _E()
        size = ctypes.c_size_t()
        E.check(self.L.grx_env_state_size(self.h, ctypes.byref(size)))
        buf = np.zeros(size.value, np.uint8)
        E.check(self.L.grx_env_get_state(self.h, buf.ctypes.data, buf.size))
        return buf

    def set_state(self, buf):
        return self.L.grx_env_set_state(self.h, buf.ctypes.data, buf.size)

    def set_elapsed(self, phase):
        """staggered episodes: the elapsed section of a state blob (tools/bench_env_capi.py)"""
        blob = self.state()
        off = _E().section_table(blob)[1]["elapsed"][0]
        blob[off: off + 8 * self.n] = np.frombuffer(np.asarray(phase, np.int64).tobytes(), np.uint8)
        assert self.set_state(blob) == 0, self.err()

    def close(self):
        if self.h:
            _E().check(self.L.grx_env_destroy(self.h))
            self.h = None


class Replay:
    """a grx_replay attached to a Handle; device pointers as torch views (env_capi.device_view)"""

    def __init__(self, c, horizon, capacity, seed=0, keep_final=0, max_batch=0):
        E = _E()
        self.c, self.L = c, c.L
        cfg = E.ReplayConfig(horizon=horizon, keep_final=keep_final, capacity=capacity, max_batch=max_batch, seed=seed)
        self.r = ctypes.c_void_p()
        E.check(self.L.grx_replay_create(c.h, ctypes.byref(cfg), ctypes.byref(self.r)))
        d = [ctypes.c_int() for _ in range(4)]
        E.check(self.L.grx_replay_dims(self.r, *[ctypes.byref(x) for x in d]))
        self.dims = tuple(x.value for x in d)      # row_width, obs_dim, goal_dim, act_dim

    def begin(self):
        return self.L.grx_replay_begin(self.r, self.c.stream())

    def append(self):
        return self.L.grx_replay_append(self.r, self.c.stream())

    def reseed(self, seed):
        return self.L.grx_replay_reseed(self.r, seed)

    def relabel(self, batch, k=4):
        E = _E()
        b = E.ReplayBatch()
        E.check(self.L.grx_replay_relabel(self.r, batch, k, ctypes.byref(b), self.c.stream()))
        assert b.batch == batch
        return E.device_view(b.rows, (batch, self.dims[0])), E.device_view(b.valid, (1,), np.int32), int(b.offset)

    def ring(self):
        E = _E()
        p, cap, head, size = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        E.check(self.L.grx_replay_ring(self.r, ctypes.byref(p), ctypes.byref(cap), ctypes.byref(head), ctypes.byref(size)))
        return E.device_view(p.value, (cap.value, self.dims[0])), head.value, size.value

    def close(self):
        if self.r:
            _E().check(self.L.grx_replay_destroy(self.r))
            self.r = None


def _fetch_env(env_id, n, mode, horizon=50):
    from gymnasium_robotics_amd.envs.fetch import FetchVecEnv

    return FetchVecEnv(env_id, num_envs=n, device="cuda:0", autoreset_mode=mode, max_episode_steps=horizon, output="torch")


def _maze_env(env_id, n, mode, horizon=40, **kw):
    from gymnasium_robotics_amd.envs.point_maze import AntMazeVecEnv, PointMazeVecEnv

    cls = AntMazeVecEnv if env_id.startswith("AntMaze_") else PointMazeVecEnv
    return cls(env_id, num_envs=n, device="cuda:0", autoreset_mode=mode, max_episode_steps=horizon, output="torch", **kw)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _py_relabel(buf, batch, k):
    """HerReplay.relabel with the documented difference of grx_replay_relabel applied by hand: with nothing to sample the slot is taken all the same, zero-filled"""
    v = buf.relabel(batch, k)
    if len(v):
        return v, batch
    view = buf.rows[buf.head: buf.head + batch]      # (relabel has wrapped the head already where the slot would not fit)
    view.zero_()
    buf.head += batch
    buf.size = min(buf.capacity, max(buf.size, buf.head))
    return view, 0


def _drive(env, c, mode, keep_final, steps, T, act_fn, obs, reseed, maze):
    """steps x (env.step + HerReplay.append + relabel | grx_env_step + grx_replay_append + grx_replay_relabel), every batch compared; then the whole ring.
    -> counts: steps with nothing to sample, episodes ended by termination, episodes ended"""
    import torch
    from gymnasium_robotics_amd.her import HerReplay

    n = c.n
    batch = 4 * n
    capacity = 10 * batch + 7      # not a multiple of the batch: the head wraps with a tail left over
    buf = HerReplay(env, horizon=T, capacity=capacity, seed=5, continuous=True)
    rp = Replay(c, T, capacity, seed=5, keep_final=keep_final, max_batch=batch)
    try:
        assert rp.dims == (buf.OW, buf.obs_dim, buf.goal_dim, buf.act_dim)
        buf.begin_episode(env.packed)
        buf.set_episode_start(-env._elapsed)
        assert rp.begin() == 0, c.err()
        od, gd = buf.obs_dim, buf.goal_dim
        term = torch.zeros(n, buf.W, device="cuda:0") if (maze and keep_final and mode == "same_step") else None
        stats = dict(empty=0, terminated=0, finished=0)
        for t in range(steps):
            pending = env._needs_reset.copy()
            a = act_fn(t, obs)
            obs, _, te, tr, info = env.step(a)
            assert c.step(a) == 0, c.err()
            te, tr = te.numpy().astype(bool), tr.numpy().astype(bool)
            done = te | tr
            stats["terminated"] += int(te.sum())
            stats["finished"] += int(done.sum())
            if mode == "same_step" and keep_final:
                if maze:      # a world-indexed [N, W] buffer of terminal rows, filled from info["final_obs"] (the relabel kernel reads their observation and achieved-goal words only)
                    if done.any():
                        ti, fo = torch.from_numpy(np.nonzero(done)[0]).to("cuda:0"), info["final_obs"]
                        term[ti, :od], term[ti, od: od + gd], term[ti, od + gd: od + 2 * gd] = fo["observation"], fo["achieved_goal"], fo["desired_goal"]
                    buf.append(a, env.packed, done, final_rows=term)
                else:
                    buf.append(a, env.packed, done, final_rows=env.final_packed)
            elif mode == "same_step":
                buf.append(a, env.packed, done)
            else:      # next-step: the worlds that were pending before the step were reset in place of it
                buf.append(a, env.packed, pending)
            assert rp.append() == 0, c.err()
            if reseed:
                buf.reseed(1000 + t)
                assert rp.reseed(1000 + t) == 0
            want, want_valid = _py_relabel(buf, batch, 4)
            rows, valid, offset = rp.relabel(batch, 4)
            torch.cuda.synchronize()
            assert offset == buf.head - batch, t
            assert int(valid.item()) == want_valid, (t, int(valid.item()), want_valid)
            got = _bits(rows)
            assert np.array_equal(got, _bits(want)), (t, int((got != _bits(want)).sum()))
            if want_valid == 0:
                stats["empty"] += 1
                assert not got.any(), t
        ring, head, size = rp.ring()
        torch.cuda.synchronize()
        assert (head, size) == (buf.head, buf.size)
        assert size == capacity - 7 and steps * batch > capacity      # the ring wrapped
        assert np.array_equal(_bits(ring), _bits(buf.rows))
        return stats
    finally:
        rp.close()


def _fetch_rollout(env_id, n, mode, tmp_path, steps=130, horizon=50):
    import torch

    env, c = _fetch_env(env_id, n, mode, horizon), Handle(env_id, n, tmp_path, mode, horizon)
    try:
        env.reset(seed=7)
        assert c.reset(seeds=7 + np.arange(n)) == 0
        phase = (np.arange(n) * 7) % horizon      # staggered: world i is at step 7 i mod 50 of its episode
        env._elapsed[:] = phase
        c.set_elapsed(phase)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)
        act = lambda t, obs: torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1
        stats = _drive(env, c, mode, 1, steps, horizon, act, None, reseed=False, maze=False)
        assert stats["empty"] == 0 and stats["finished"] >= 2 * n      # every world crossed two episode ends
    finally:
        c.close()
        env.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("env_id", FETCH_IDS)
def test_fetch_replay_is_her_replay_bit_for_bit(env_id, mode, tmp_path):
    """64 worlds, staggered phases, 130 steps with horizon 50; same-step keeps the finished episodes' last transitions (keep_final = 1 against final_rows=env.final_packed)"""
    _fetch_rollout(env_id, 64, mode, tmp_path)


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_fetch_replay_is_her_replay_bit_for_bit_at_4096(mode, tmp_path):
    """the headline shape: FetchPickAndPlace-v4, 4 096 worlds, batches of 16 384 transitions"""
    _fetch_rollout("FetchPickAndPlace-v4", 4096, mode, tmp_path)


def _maze_rollout(env_id, n, mode, keep_final, kw, tmp_path, steps=130, horizon=40):
    import torch

    ant = env_id.startswith("AntMaze_")
    kw = dict(kw)
    if ant and kw.get("continuing_task") is False:
        kw["position_noise_range"] = ANT_EPISODIC_NOISE
    env, c = _maze_env(env_id, n, mode, horizon, **kw), Handle(env_id, n, tmp_path, mode, horizon, **kw)
    try:
        obs, _ = env.reset(seed=7)
        assert c.reset(seeds=7 + np.arange(n)) == 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)

        def act(t, obs):
            a = torch.rand(n, env.nu, device="cuda:0", generator=gen) * 2 - 1
            if not ant:      # the first half of the batch is steered to its goals (tests/test_gpu_env_capi_maze.py), from the Python environment's observation
                a[: n // 2] = torch.clamp(4.0 * (obs["desired_goal"] - obs["achieved_goal"]) - obs["observation"][:, 2:4], -1.0, 1.0)[: n // 2]
            return a.float().contiguous()

        stats = _drive(env, c, mode, keep_final, steps, horizon, act, obs, reseed=True, maze=True)
        print(f"{env_id} {kw} {mode} keep_final={keep_final} n={n}: {stats}")
        assert stats["finished"] >= 2 * n
        if kw.get("continuing_task") is False:
            assert stats["terminated"] >= 1, stats      # episodes ended on the device's word, not only by the time limit
        return stats
    finally:
        c.close()
        env.close()


SAME_AND_NEXT = [("same_step", 0), ("same_step", 1), ("next_step", 0)]


@pytest.mark.parametrize("mode,keep_final", SAME_AND_NEXT, ids=["same_step", "same_step_keep_final", "next_step"])
@pytest.mark.parametrize("kw", list(MODE_SETS.values()), ids=list(MODE_SETS))
@pytest.mark.parametrize("env_id", POINT_IDS + ANT_IDS)
def test_maze_replay_is_her_replay_bit_for_bit(env_id, kw, mode, keep_final, tmp_path):
    """64 worlds: host bookkeeping (default), then the two device-bookkeeping modes, where the reset list and its length exist only in device memory"""
    _maze_rollout(env_id, 64, mode, keep_final, kw, tmp_path)


@pytest.mark.parametrize("mode,keep_final", [("same_step", 1), ("next_step", 0)], ids=["same_step_keep_final", "next_step"])
@pytest.mark.parametrize("kw", list(MODE_SETS.values()), ids=list(MODE_SETS))
@pytest.mark.parametrize("env_id", [POINT_IDS[0], ANT_IDS[0]])
def test_maze_replay_is_her_replay_bit_for_bit_at_8192(env_id, kw, mode, keep_final, tmp_path):
    """8 192 worlds: the episode-end kernel's list holds thousands of worlds, the append grid is bounded below that"""
    _maze_rollout(env_id, 8192, mode, keep_final, kw, tmp_path, steps=90)


def test_append_and_relabel_do_not_wait_for_the_device(tmp_path):
    """continuing_task=False (device bookkeeping: the worlds a step reset are known to the device alone), 8 192 ants: twenty step + append + relabel groups are enqueued back
    to back; when the last call returns the stream still has work queued, so none of them waited for the device (the technique of
    tests/test_gpu_env_capi_maze.py::test_step_does_not_wait_for_the_device)"""
    import torch

    n = 8192
    c = Handle("AntMaze_Large_Diverse_GR-v5", n, tmp_path, "same_step", 40, continuing_task=False)
    rp = Replay(c, 40, 64 * n, seed=1, keep_final=1, max_batch=4 * n)
    try:
        assert c.reset(seeds=np.arange(n)) == 0
        assert rp.begin() == 0
        a = torch.rand(n, c.act_dim, device="cuda:0") * 2 - 1
        assert c.step(a) == 0 and rp.append() == 0
        rp.relabel(4 * n)
        torch.cuda.synchronize()
        for _ in range(20):
            assert c.step(a) == 0 and rp.append() == 0, c.err()
            rows, valid, _ = rp.relabel(4 * n)
        busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        assert busy, "the stream was idle when the twentieth grx_replay_relabel returned: a call waited for the device"
        assert int(valid.item()) == 4 * n and np.isfinite(rows.cpu().numpy()).all()
    finally:
        rp.close()
        c.close()


def test_nothing_to_sample_is_decided_on_the_device(tmp_path):
    """an unstaggered next-step batch with horizon = time limit: at the step that resets every world no world has a transition; valid[0] = 0, the slot is zero-filled and
    HerReplay.relabel returns an empty view (asserted inside _drive); the steps after it match again.  Both sides are reseeded before every relabel (see the module docstring)."""
    import torch

    n, horizon = 64, 10
    env, c = _fetch_env("FetchPush-v4", n, "next_step", horizon), Handle("FetchPush-v4", n, tmp_path, "next_step", horizon)
    try:
        env.reset(seed=3)
        assert c.reset(seeds=3 + np.arange(n)) == 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(2)
        act = lambda t, obs: torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1
        stats = _drive(env, c, "next_step", 0, 50, horizon, act, None, reseed=True, maze=False)
        assert stats["empty"] == 4, stats      # steps 11, 22, 33, 44: every world reset in place of stepping
    finally:
        c.close()
        env.close()


def test_relabel_before_any_append_samples_nothing(tmp_path):
    import torch

    c = Handle("FetchReach-v4", 64, tmp_path)
    rp = Replay(c, 50, 1024, max_batch=256)
    try:
        assert c.reset(seeds=np.arange(64)) == 0 and rp.begin() == 0
        rows, valid, offset = rp.relabel(256)
        torch.cuda.synchronize()
        assert int(valid.item()) == 0 and offset == 0 and not _bits(rows).any()
    finally:
        rp.close()
        c.close()


def test_ordering_errors(tmp_path):
    import torch

    E = _E()
    c = Handle("FetchReach-v4", 64, tmp_path, "same_step", 50)
    rp = Replay(c, 50, 1024, max_batch=256)
    try:
        a = torch.zeros(64, 4, device="cuda:0")
        assert c.reset(seeds=np.arange(64)) == 0 and c.step(a) == 0
        assert rp.append() == -1 and "before grx_replay_begin" in c.err()
        assert rp.begin() == 0
        assert rp.append() == -1 and "double append" in c.err()      # no step since begin
        assert c.step(a) == 0 and rp.append() == 0
        assert rp.append() == -1 and "double append" in c.err()
        assert c.step(a) == 0 and c.step(a) == 0
        assert rp.append() == -1 and "every step is appended" in c.err()
        assert rp.begin() == 0 and c.step(a) == 0 and rp.append() == 0
        assert c.reset(seeds=np.arange(64)) == 0 and c.step(a) == 0
        assert rp.append() == -1 and "grx_env_reset" in c.err() and "grx_replay_begin" in c.err()
        assert rp.begin() == 0 and c.step(a) == 0 and rp.append() == 0
        assert c.set_state(c.state()) == 0 and c.step(a) == 0
        assert rp.append() == -1 and "grx_env_set_state" in c.err()
        b = E.ReplayBatch()
        assert c.L.grx_replay_relabel(rp.r, 257, 4, ctypes.byref(b), None) == -1 and "max_batch" in c.err()
        assert c.L.grx_replay_relabel(rp.r, 2048, 4, ctypes.byref(b), None) == -1 and "capacity" in c.err()
        assert c.L.grx_replay_relabel(rp.r, 0, 4, ctypes.byref(b), None) == -1
        second = ctypes.c_void_p()
        cfg = E.ReplayConfig(horizon=50, keep_final=0, capacity=1024, max_batch=0, seed=0)
        assert c.L.grx_replay_create(c.h, ctypes.byref(cfg), ctypes.byref(second)) == -1 and "already" in c.err()
        assert c.L.grx_env_destroy(c.h) == -1 and "replay is attached" in c.err()
        # the handle is still whole: it steps, and is destroyed once the replay is
        assert rp.begin() == 0 and c.step(a) == 0 and rp.append() == 0
        rows, valid, _ = rp.relabel(256)
        torch.cuda.synchronize()
        assert int(valid.item()) == 256 and np.isfinite(rows.cpu().numpy()).all()
    finally:
        rp.close()
        c.close()


def _fnv1a(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c99_replay_example_matches_ctypes(tmp_path):
    import torch

    E = _E()
    E.lib()
    cc = shutil.which("cc") or shutil.which("gcc")
    libdir = os.path.dirname(E.LIB_PATH)
    exe = tmp_path / "replay_rollout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "replay_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    env_id, n, steps = "FetchPickAndPlace-v4", 64, 60
    desc = E.write_env_desc(env_id, str(tmp_path / "pick.grxenv"))
    res = subprocess.run(["timeout", "-k", "10", "300", str(exe), desc, str(n), str(steps)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split() for line in res.stdout.strip().splitlines())
    c = Handle(env_id, n, tmp_path, "same_step", 25)
    batch = 4 * n
    rp = Replay(c, 25, 16 * batch, seed=5, keep_final=1, max_batch=batch)
    try:
        assert c.reset(seeds=1000 + np.arange(n)) == 0 and rp.begin() == 0
        i, j = np.meshgrid(np.arange(n), np.arange(4), indexing="ij")
        for t in range(steps):
            a = torch.from_numpy((((t * 11 + i * 7 + j * 3) % 17) / 8.0 - 1.0).astype(np.float32)).cuda()
            assert c.step(a) == 0 and rp.append() == 0
            rows, valid, offset = rp.relabel(batch)
        torch.cuda.synchronize()
        assert int(lines["row_width"]) == rp.dims[0] == 2 * c.obs_dim + 3 * 3 + 4 + 2
        assert int(lines["valid"]) == int(valid.item()) == batch
        assert int(lines["offset"]) == offset == ((steps - 1) % 16) * batch
        assert int(lines["checksum"], 16) == _fnv1a(rows.cpu().numpy().tobytes())
    finally:
        rp.close()
        c.close()
