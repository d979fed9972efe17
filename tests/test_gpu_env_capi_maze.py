"""The maze handle of the env-level C ABI (include/grx_env.h, libgrx_env.so) against PointMazeVecEnv / AntMazeVecEnv(output="torch") with the same seeds and the
same actions, bit for bit after every step: outputs, flags, the parked terminal rows and the state sections, in both autoreset modes and in every mode of the maze
environments (continuing_task=False, reset_target=True); that grx_env_step does not wait for the device; checkpoint / resume across an autoreset; the batched reward;
and the C99 worked example (tests/capi/maze_rollout.c) against the same rollout driven through ctypes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
M64 = (1 << 64) - 1


def _maze_ids():
    import gymnasium_robotics_amd as grx

    return [i for i in grx.registered_env_ids() if i.startswith("PointMaze_") or i.startswith("AntMaze_")]


MAZE_IDS = _maze_ids()


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
    """a grx_env handle and host copies of what it holds (test plumbing only)"""

    def __init__(self, env_id, n, tmp_path, mode="next_step", horizon=40, **kw):
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
        self.obs_dim, self.goal_dim, self.act_dim, self.dt = od.value, gd.value, ad.value, dt.value
        self.width = self.obs_dim + 2 * self.goal_dim + 2
        self.stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reset(self, seeds=None, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        return self.L.grx_env_reset(self.h, None if m is None else m.ctypes.data, None if s is None else s.ctypes.data, self.stream())

    def step(self, actions):
        return self.L.grx_env_step(self.h, actions.data_ptr(), self.stream())

    def host(self):
        E, n, w, g = _E(), self.n, self.width, self.goal_dim
        o = dict(obs=np.zeros((n, self.obs_dim), np.float32), achieved=np.zeros((n, g), np.float32), desired=np.zeros((n, g), np.float32), reward=np.zeros(n, np.float32),
                 success=np.zeros(n, np.uint8), status=np.zeros(n, np.int32), packed=np.zeros((n, w), np.float32), terminated=np.zeros(n, np.uint8), truncated=np.zeros(n, np.uint8),
                 n_final=np.zeros(1, np.int32), final_idx=np.zeros(n, np.int32), final_rows=np.zeros((n, w), np.float32))
        E.check(self.L.grx_env_copy_outputs(self.h, ctypes.byref(E.EnvHostOutputs(**{k: v.ctypes.data for k, v in o.items()}))))
        k = int(o["n_final"][0])
        o["final_idx"], o["final_rows"] = o["final_idx"][:k], o["final_rows"][:k]
        return o

    def state(self):
        E = _E()
        size = ctypes.c_size_t()
        E.check(self.L.grx_env_state_size(self.h, ctypes.byref(size)))
        buf = np.zeros(size.value, np.uint8)
        E.check(self.L.grx_env_get_state(self.h, buf.ctypes.data, buf.size))
        return buf

    def set_state(self, buf):
        return self.L.grx_env_set_state(self.h, buf.ctypes.data, buf.size)

    def close(self):
        if self.h:
            _E().check(self.L.grx_env_destroy(self.h))
            self.h = None


def _py_env(env_id, n, mode, horizon=40, **kw):
    from gymnasium_robotics_amd.envs.point_maze import AntMazeVecEnv, PointMazeVecEnv

    cls = AntMazeVecEnv if env_id.startswith("AntMaze_") else PointMazeVecEnv
    return cls(env_id, num_envs=n, device="cuda:0", autoreset_mode=mode, max_episode_steps=horizon, output="torch", **kw)


def _row5(gen):
    """a numpy generator's PCG64 position as the device row: state_hi, state_lo, inc_hi, inc_lo, has_uint32 << 32 | uinteger (the stale half of a consumed buffer is not state)"""
    s = gen.bit_generator.state
    st, inc, has = s["state"]["state"], s["state"]["inc"], int(s["has_uint32"])
    return [st >> 64, st & M64, inc >> 64, inc & M64, (has << 32) | (int(s["uinteger"]) if has else 0)]


def _py_rng_rows(env):
    if env._device_draws:
        return env._rng_dev.cpu().numpy().view(np.uint64)
    return np.array([_row5(g) for g in env.np_randoms], dtype=np.uint64)


def _py_reseed(env, idx, seeds):
    import torch
    from gymnasium_robotics_amd.core import np_random

    if env._device_draws:
        rows = np.array([_row5(np_random(int(seeds[i]))[0]) for i in idx], dtype=np.uint64)
        env._rng_dev[torch.from_numpy(np.asarray(idx, np.int64)).to(env.device)] = torch.from_numpy(rows.view(np.int64)).to(env.device)
    else:
        for i in idx:
            env.np_randoms[i] = np_random(int(seeds[i]))[0]
    with torch.cuda.device(env.device):
        env._reset_worlds(np.asarray(idx))


def _compare_step(env, c, t, step_out, o):
    import torch

    E = _E()
    obs, r, te, tr, info = step_out
    torch.cuda.synchronize()
    for key, ck in (("observation", "obs"), ("achieved_goal", "achieved"), ("desired_goal", "desired")):
        assert np.array_equal(obs[key].cpu().numpy(), o[ck]), (t, key)
    assert np.array_equal(r.cpu().numpy(), o["reward"]), t
    assert np.array_equal(info["success"].cpu().numpy(), o["success"].astype(bool)), t
    assert np.array_equal(env.status.cpu().numpy(), o["status"]), t
    assert np.array_equal(env.packed.cpu().numpy(), o["packed"]), t
    assert np.array_equal(te.numpy(), o["terminated"].astype(bool)), t
    assert np.array_equal(tr.numpy(), o["truncated"].astype(bool)), t
    if "final_obs" in info:
        assert np.array_equal(o["final_idx"], np.nonzero(te.numpy() | tr.numpy())[0]), t
        fo, d = info["final_obs"], c.obs_dim
        assert np.array_equal(fo["observation"].cpu().numpy(), o["final_rows"][:, :d]), t
        assert np.array_equal(fo["achieved_goal"].cpu().numpy(), o["final_rows"][:, d: d + 2]), t
        assert np.array_equal(fo["desired_goal"].cpu().numpy(), o["final_rows"][:, d + 2: d + 4]), t
    else:
        assert len(o["final_idx"]) == 0, t
    head, s = E.state_arrays(c.state())
    for name in ("qpos", "qvel", "qacc_ws", "goal"):
        assert np.array_equal(s[name], getattr(env, name).cpu().numpy()), (t, name)
    assert np.array_equal(s["rng"], _py_rng_rows(env)), t
    assert np.array_equal(s["elapsed"].ravel(), env._elapsed), t
    assert np.array_equal(s["needs_reset"].ravel().astype(bool), env._needs_reset), t
    return "final_obs" in info


def _rollout_compare(env_id, n, mode, tmp_path, steps=130, horizon=40, steer=False, partial_resets=True, **kw):
    """-> (steps with finished worlds, worlds that reached a goal at least once, times a world reached its goal in the very step that truncated it)"""
    import torch

    env, c = _py_env(env_id, n, mode, horizon, **kw), Handle(env_id, n, tmp_path, mode, horizon, **kw)
    try:
        assert (c.goal_dim, c.act_dim, c.obs_dim) == (2, env.nu, env.obs_dim)
        obs, _ = env.reset(seed=7)
        assert c.reset(seeds=7 + np.arange(n)) == 0
        o = c.host()
        assert np.array_equal(obs["observation"].cpu().numpy(), o["obs"]) and np.array_equal(obs["desired_goal"].cpu().numpy(), o["desired"])
        rs = np.random.default_rng(3)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)
        finals = partial = 0
        reached = np.zeros(n, bool)
        both = 0
        for t in range(steps):
            if partial_resets and t % 9 == 4:      # staggered episodes: partial resets with fresh seeds (gymnasium's reset_mask)
                idx = np.sort(rs.choice(n, max(1, n // 10), replace=False))
                mask, seeds = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
                mask[idx], seeds[idx] = 1, 100000 + 1000 * t + idx
                assert c.reset(seeds=seeds, mask=mask) == 0
                _py_reseed(env, idx, seeds)
                obs = env._obs_dict()
                partial += 1
            if steer:      # towards the goal: a = clip(4 (desired - achieved) - velocity, -1, 1), from the Python environment's observation
                a = torch.clamp(4.0 * (obs["desired_goal"] - obs["achieved_goal"]) - obs["observation"][:, 2:4], -1.0, 1.0).float().contiguous()
            else:
                a = torch.rand(n, env.nu, device="cuda:0", generator=gen) * 2 - 1
            out = env.step(a)
            assert c.step(a) == 0, c.L.grx_env_last_error()
            finals += _compare_step(env, c, t, out, c.host())
            obs = out[0]
            reached |= out[4]["success"].cpu().numpy()
            both += int((out[4]["success"].cpu().numpy() & out[3].numpy()).sum())
        if partial_resets:
            assert partial >= steps // 9
        return finals, int(reached.sum()), both
    finally:
        c.close()
        env.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("env_id", MAZE_IDS)
def test_c_abi_is_maze_vec_env_bit_for_bit(env_id, mode, tmp_path):
    """every registered maze id, 64 worlds, a horizon of 40 steps: three episodes roll over, with partial resets in between"""
    finals, _, _ = _rollout_compare(env_id, 64, mode, tmp_path)
    if mode == "same_step":
        assert finals > 2


@pytest.mark.parametrize("env_id", ["PointMaze_Medium-v3", "AntMaze_Open-v5"])
def test_disabled_autoreset_reports_flags_only(env_id, tmp_path):
    finals, _, _ = _rollout_compare(env_id, 64, "disabled", tmp_path, steps=100)
    assert finals == 0


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("kw", [{}, {"continuing_task": False}], ids=["default", "episodic"])
@pytest.mark.parametrize("env_id", ["AntMaze_Large_Diverse_GR-v5", "PointMaze_Large-v3"])
def test_c_abi_is_maze_vec_env_bit_for_bit_at_8192(env_id, kw, mode, tmp_path):
    """8 192 worlds: the ant's split step is in play; with continuing_task=False the bookkeeping is the device's and the episode-end kernel walks 8 chunks, its
    reset list holding all 8 192 worlds when the time limit comes"""
    env = _py_env(env_id, 8192, mode, **kw)
    assert env._split == (5 if env_id.startswith("AntMaze_") else 1)
    env.close()
    _rollout_compare(env_id, 8192, mode, tmp_path, steps=90, **kw)


@pytest.mark.parametrize("mode", ["same_step", "next_step", "disabled"])
@pytest.mark.parametrize("env_id", ["PointMaze_Medium_Diverse_GR-v3", "AntMaze_UMaze-v5"])
def test_device_bookkeeping_with_partial_resets(env_id, mode, tmp_path):
    """continuing_task=False: the counters, flags and reset lists are the device's (in the default mode the host keeps them); staggered by partial resets"""
    _rollout_compare(env_id, 64, mode, tmp_path, continuing_task=False)


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("kw", [{"continuing_task": False}, {"reset_target": True}], ids=["episodic", "reset_target"])
@pytest.mark.parametrize("env_id", ["PointMaze_Open_Diverse_G-v3", "PointMaze_Open_Diverse_GR-v3"])
def test_goal_reaching_modes_bit_for_bit(env_id, kw, mode, tmp_path):
    """Worlds steered to their goals: termination (continuing_task=False) and update_goal's redraw (reset_target=True) decided on the device against the Python
    environment's host logic.  With reset_target=True the Python side draws from per-world numpy generators on the host: the goals and the PCG64 rows are compared with
    them after every step.  At least half of the worlds must reach a goal, or the rollout proves nothing."""
    n = 256
    _, reached, both = _rollout_compare(env_id, n, mode, tmp_path, steps=120, horizon=100, steer=True, partial_resets=False, **kw)
    print(f"{env_id} {kw} {mode}: {reached} of {n} worlds reached a goal, {both} times in the step that truncated the world")
    assert reached >= n // 2, reached
    if kw.get("reset_target"):      # the redraw's draws of a world that is also done in this step (consumed ahead of its reset draws) were in the rollout
        assert both >= 1, both


def test_step_does_not_wait_for_the_device(tmp_path):
    """continuing_task=False (where PointMazeVecEnv.step reads the termination flags back every step): twenty 8 192-world AntMaze steps (about 2 ms of device time
    each) are enqueued back to back; when the last grx_env_step returns the stream still has work queued, so no call in it waited for the device."""
    import torch

    n = 8192
    c = Handle("AntMaze_Large_Diverse_GR-v5", n, tmp_path, "same_step", 40, continuing_task=False)
    try:
        assert c.reset(seeds=np.arange(n)) == 0
        a = torch.rand(n, c.act_dim, device="cuda:0") * 2 - 1
        assert c.step(a) == 0
        torch.cuda.synchronize()
        for _ in range(20):
            assert c.step(a) == 0
        busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        assert busy, "the stream was idle when the twentieth grx_env_step returned: a call in it waited for the device"
        o = c.host()
        assert np.isfinite(o["obs"]).all()
    finally:
        c.close()


@pytest.mark.parametrize("env_id,kw", [("PointMaze_Medium-v3", {}), ("PointMaze_UMazeDense-v3", {}), ("AntMaze_UMaze-v5", {}), ("AntMaze_MediumDense-v5", {})])
def test_reward_is_compute_reward(env_id, kw, tmp_path):
    import torch

    env, c = _py_env(env_id, 64, "next_step"), Handle(env_id, 64, tmp_path)
    try:
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(2)
        ag = torch.rand(4096, 2, device="cuda:0", generator=gen) * 2 - 1
        dg = ag + (torch.rand(4096, 2, device="cuda:0", generator=gen) - 0.5)
        out = torch.empty(4096, device="cuda:0")
        _E().check(c.L.grx_env_compute_reward(c.h, ag.data_ptr(), dg.data_ptr(), 4096, out.data_ptr(), c.stream()))
        want = env.compute_reward(ag, dg)
        assert np.array_equal(out.cpu().numpy(), want.cpu().numpy())
        assert 0 < int((want > 0.5).sum()) < 4096
    finally:
        c.close()
        env.close()


def test_state_round_trip_across_an_autoreset(tmp_path):
    import torch

    n = 128
    c = Handle("AntMaze_Medium_Diverse_GR-v5", n, tmp_path, "same_step", 40)
    other_id, other_n, fetch = Handle("AntMaze_Medium-v5", n, tmp_path, "same_step", 40), Handle("AntMaze_Medium_Diverse_GR-v5", 64, tmp_path), None
    try:
        E = _E()
        fpath = E.write_env_desc("FetchReach-v4", str(tmp_path / "reach.grxenv"))
        fh = ctypes.c_void_p()
        E.check(c.L.grx_env_create(fpath.encode(), n, 0, None, ctypes.byref(fh)))
        fetch = fh
        assert c.reset(seeds=np.arange(n)) == 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(4)
        acts = [torch.rand(n, c.act_dim, device="cuda:0", generator=gen) * 2 - 1 for _ in range(50)]
        for a in acts[:30]:
            assert c.step(a) == 0
        blob = c.state()

        def run():
            outs = []
            for a in acts[30:]:
                assert c.step(a) == 0
                o = c.host()
                outs.append((o["packed"].copy(), o["status"].copy(), o["truncated"].copy(), o["final_idx"].copy(), o["final_rows"].copy()))
            return outs, c.state()

        first, end1 = run()
        assert sum(len(x[3]) for x in first) == n      # every world finished its episode at step 40 inside the window
        assert c.set_state(blob) == 0
        second, end2 = run()
        for t, (x, y) in enumerate(zip(first, second)):
            for u, v in zip(x, y):
                assert np.array_equal(u, v), t
        assert np.array_equal(end1, end2)
        assert other_id.set_state(blob) == -5 and b"does not fit" in c.L.grx_env_last_error()
        assert other_n.set_state(blob) == -5 and b"does not fit" in c.L.grx_env_last_error()
        # a Fetch blob is refused by a maze handle and a maze blob by a Fetch handle
        size = ctypes.c_size_t()
        E.check(c.L.grx_env_state_size(fetch, ctypes.byref(size)))
        fblob = np.zeros(size.value, np.uint8)
        E.check(c.L.grx_env_get_state(fetch, fblob.ctypes.data, fblob.size))
        assert c.set_state(fblob) == -5
        assert c.L.grx_env_set_state(fetch, blob.ctypes.data, blob.size) == -5
    finally:
        for h in (c, other_id, other_n):
            h.close()
        if fetch is not None:
            c.L.grx_env_destroy(fetch)


def test_errors_leave_the_device_healthy(tmp_path):
    import torch

    c = Handle("PointMaze_UMaze-v3", 64, tmp_path)
    try:
        a = torch.zeros(64, 2, device="cuda:0")
        assert c.step(a) == -1 and b"before" in c.L.grx_env_last_error()
        assert c.L.grx_env_step(c.h, None, None) == -1 and b"NULL" in c.L.grx_env_last_error()
        junk = np.frombuffer(b"not a state blob" * 8, np.uint8).copy()
        assert c.set_state(junk) == -5 and b"wrong magic" in c.L.grx_env_last_error()
        assert c.reset(seeds=np.arange(64)) == 0 and c.step(a) == 0
        o = c.host()
        torch.cuda.synchronize()
        assert np.isfinite(o["obs"]).all() and int(np.abs(o["status"] & 0xFFFF).max()) == 0
        assert c.dt > 0
    finally:
        c.close()


def _fnv1a(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c99_rollout_example_matches_ctypes(tmp_path):
    import torch

    E = _E()
    E.lib()
    cc = shutil.which("cc") or shutil.which("gcc")
    libdir = os.path.dirname(E.LIB_PATH)
    exe = tmp_path / "maze_rollout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "maze_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    env_id = "AntMaze_UMaze-v5"
    desc = E.write_env_desc(env_id, str(tmp_path / "ant.grxenv"))
    n, steps = 64, 60
    res = subprocess.run(["timeout", "-k", "10", "300", str(exe), desc, str(n), str(steps)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split() for line in res.stdout.strip().splitlines())
    c = Handle(env_id, n, tmp_path, "same_step", 20)
    try:
        assert c.reset(seeds=1000 + np.arange(n)) == 0
        i, j = np.meshgrid(np.arange(n), np.arange(c.act_dim), indexing="ij")
        finished = 0
        for t in range(steps):
            a = torch.from_numpy((((t * 11 + i * 7 + j * 3) % 17) / 8.0 - 1.0).astype(np.float32)).cuda()
            assert c.step(a) == 0
            finished += len(c.host()["final_idx"])
        packed = c.host()["packed"]
    finally:
        c.close()
    assert int(lines["finished"]) == finished == 3 * n
    assert int(lines["checksum"], 16) == _fnv1a(packed.tobytes())
