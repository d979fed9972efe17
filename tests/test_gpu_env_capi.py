"""The env-level C ABI of the Fetch family (include/grx_env.h, libgrx_env.so) against FetchVecEnv(output="torch") -- the Python launch group it restates --
bit for bit: outputs, flags, the parked terminal rows and the state rows, after every step of staggered rollouts in both autoreset modes; the batched reward;
checkpoint / resume across an autoreset; argument errors; and the C99 worked example (tests/capi/fetch_rollout.c) against the same rollout driven through ctypes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FETCH_IDS = [f"{t}{d}-v4" for t in ("FetchReach", "FetchPush", "FetchSlide", "FetchPickAndPlace") for d in ("", "Dense")]


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

    def __init__(self, env_id, n, tmp_path, mode="next_step", horizon=50):
        import torch

        E = _E()
        self.L, self.n = E.lib(), n
        path = E.write_env_desc(env_id, str(tmp_path / f"{env_id}.grxenv"))
        cfg = E.EnvConfig(E.AUTORESET[mode], horizon, 0)
        self.h = ctypes.c_void_p()
        E.check(self.L.grx_env_create(path.encode(), n, 0, ctypes.byref(cfg), ctypes.byref(self.h)))
        od, gd, ad, dt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        E.check(self.L.grx_env_dims(self.h, ctypes.byref(od), ctypes.byref(gd), ctypes.byref(ad), ctypes.byref(dt)))
        self.obs_dim = od.value
        assert (gd.value, ad.value) == (3, 4)
        self.stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reset(self, seeds=None, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        s = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        return self.L.grx_env_reset(self.h, None if m is None else m.ctypes.data, None if s is None else s.ctypes.data, self.stream())

    def step(self, actions):
        return self.L.grx_env_step(self.h, actions.data_ptr(), self.stream())

    def host(self):
        E, n, w = _E(), self.n, self.obs_dim + 8
        o = dict(obs=np.zeros((n, self.obs_dim), np.float32), achieved=np.zeros((n, 3), np.float32), desired=np.zeros((n, 3), np.float32), reward=np.zeros(n, np.float32),
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


def _py_env(env_id, n, mode, horizon=50):
    from gymnasium_robotics_amd.envs.fetch import FetchVecEnv

    return FetchVecEnv(env_id, num_envs=n, device="cuda:0", autoreset_mode=mode, max_episode_steps=horizon, output="torch")


def _rows(seed):
    from gymnasium_robotics_amd.core import np_random

    s = np_random(seed)[0].bit_generator.state["state"]
    m = (1 << 64) - 1
    return [s["state"] >> 64, s["state"] & m, s["inc"] >> 64, s["inc"] & m]


def _rollout_compare(env_id, n, mode, tmp_path, steps=130, horizon=50):
    import torch

    E = _E()
    env, c = _py_env(env_id, n, mode, horizon), Handle(env_id, n, tmp_path, mode, horizon)
    try:
        env.reset(seed=7)
        assert c.reset(seeds=7 + np.arange(n)) == 0
        rs = np.random.default_rng(3)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(11)
        finals = partial = 0
        for t in range(steps):
            if t % 9 == 4:      # staggered episodes: partial resets with fresh seeds (gymnasium's reset_mask)
                idx = np.sort(rs.choice(n, max(1, n // 10), replace=False))
                mask, seeds = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
                mask[idx], seeds[idx] = 1, 100000 + 1000 * t + idx
                assert c.reset(seeds=seeds, mask=mask) == 0
                st = env._rng_state
                for i in idx:
                    st[i] = _rows(int(seeds[i]))
                env._rng_state = st
                with torch.cuda.device(env.device):
                    env._reset_worlds(idx)
                partial += 1
            a = torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1
            obs, r, te, tr, info = env.step(a)
            assert c.step(a) == 0, c.L.grx_env_last_error()
            o = c.host()
            torch.cuda.synchronize()
            for key, ck in (("observation", "obs"), ("achieved_goal", "achieved"), ("desired_goal", "desired")):
                assert np.array_equal(obs[key].cpu().numpy(), o[ck]), (t, key)
            assert np.array_equal(r.cpu().numpy(), o["reward"]), t
            assert np.array_equal(env.success.cpu().numpy(), o["success"]), t
            assert np.array_equal(env.status.cpu().numpy(), o["status"]), t
            assert np.array_equal(env.packed.cpu().numpy(), o["packed"]), t
            assert np.array_equal(te.numpy(), o["terminated"].astype(bool)) and np.array_equal(tr.numpy(), o["truncated"].astype(bool)), t
            if "final_obs" in info:
                finals += 1
                assert np.array_equal(o["final_idx"], np.nonzero(tr.numpy())[0]), t
                fo, d = info["final_obs"], c.obs_dim
                assert np.array_equal(fo["observation"].cpu().numpy(), o["final_rows"][:, :d]), t
                assert np.array_equal(fo["achieved_goal"].cpu().numpy(), o["final_rows"][:, d: d + 3]), t
                assert np.array_equal(fo["desired_goal"].cpu().numpy(), o["final_rows"][:, d + 3: d + 6]), t
            else:
                assert len(o["final_idx"]) == 0, t
            head, s = E.state_arrays(c.state())
            for name in ("qpos", "qvel", "qacc_ws", "mocap", "aux", "goal"):
                assert np.array_equal(s[name], getattr(env, name).cpu().numpy()), (t, name)
            assert np.array_equal(s["rng"], env._rng_state), t
            assert np.array_equal(s["elapsed"].ravel(), env._elapsed), t
        assert partial > 10
        if mode == "same_step":
            assert finals > 2
    finally:
        c.close()
        env.close()


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("env_id", FETCH_IDS)
def test_c_abi_is_fetch_vec_env_bit_for_bit(env_id, mode, tmp_path):
    _rollout_compare(env_id, 64, mode, tmp_path)


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("env_id", ["FetchPickAndPlace-v4", "FetchPush-v4"])
def test_c_abi_is_fetch_vec_env_bit_for_bit_at_4096(env_id, mode, tmp_path):
    """4 096 worlds: split step launches, cost-ordered dispatch and the ahead-of-step reset are all in play"""
    env = _py_env(env_id, 4096, mode)
    assert env._split > 1 and env.balance and env._ahead is not None
    env.close()
    _rollout_compare(env_id, 4096, mode, tmp_path)


@pytest.mark.parametrize("env_id", ["FetchPush-v4", "FetchPushDense-v4", "FetchReachDense-v4"])
def test_reward_is_compute_reward(env_id, tmp_path):
    import torch

    c = Handle(env_id, 64, tmp_path)
    try:
        assert c.reset(seeds=np.arange(64)) == 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(2)
        for _ in range(12):
            assert c.step(torch.rand(64, 4, device="cuda:0", generator=gen) * 2 - 1) == 0
        o = c.host()
        ag, dg = torch.from_numpy(o["achieved"]).cuda(), torch.from_numpy(o["desired"]).cuda()
        out = torch.empty(64, device="cuda:0")
        _E().check(c.L.grx_env_compute_reward(c.h, ag.data_ptr(), dg.data_ptr(), 64, out.data_ptr(), c.stream()))
        assert np.array_equal(out.cpu().numpy(), o["reward"])
    finally:
        c.close()


def test_state_round_trip_across_an_autoreset(tmp_path):
    import torch

    n = 128
    c = Handle("FetchPickAndPlace-v4", n, tmp_path, "same_step", 50)
    other_id, other_n = Handle("FetchPush-v4", n, tmp_path), Handle("FetchPickAndPlace-v4", 64, tmp_path)
    try:
        assert c.reset(seeds=np.arange(n)) == 0
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(4)
        acts = [torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1 for _ in range(60)]
        for a in acts[:40]:
            assert c.step(a) == 0
        blob = c.state()

        def run():
            outs = []
            for a in acts[40:]:
                assert c.step(a) == 0
                o = c.host()
                outs.append((o["packed"].copy(), o["status"].copy(), o["truncated"].copy(), o["final_rows"].copy()))
            return outs, c.state()

        first, end1 = run()
        assert sum(len(x[3]) for x in first) == n      # every world finished its episode at step 50 inside the window
        assert c.set_state(blob) == 0
        second, end2 = run()
        for t, (x, y) in enumerate(zip(first, second)):
            for u, v in zip(x, y):
                assert np.array_equal(u, v), t
        assert np.array_equal(end1, end2)
        assert other_id.set_state(blob) == -5 and b"does not fit" in c.L.grx_env_last_error()
        assert other_n.set_state(blob) == -5 and b"does not fit" in c.L.grx_env_last_error()
    finally:
        for h in (c, other_id, other_n):
            h.close()


def test_errors_leave_the_device_healthy(tmp_path):
    import torch

    c = Handle("FetchReach-v4", 64, tmp_path)
    try:
        a = torch.zeros(64, 4, device="cuda:0")
        assert c.step(a) == -1 and b"before" in c.L.grx_env_last_error()
        assert c.L.grx_env_step(c.h, None, None) == -1 and b"NULL" in c.L.grx_env_last_error()
        assert c.L.grx_env_outputs(c.h, None) == -1
        assert c.L.grx_env_compute_reward(c.h, None, None, 4, None, None) == -1
        junk = np.frombuffer(b"not a state blob" * 8, np.uint8).copy()
        assert c.set_state(junk) == -5 and b"wrong magic" in c.L.grx_env_last_error()
        blob = c.state()
        assert c.set_state(blob[: blob.size - 16]) == -5 and b"truncated" in c.L.grx_env_last_error()
        assert c.reset(seeds=np.arange(64)) == 0 and c.step(a) == 0
        o = c.host()
        torch.cuda.synchronize()
        assert np.isfinite(o["obs"]).all() and int(np.abs(o["status"] & 0xFFFF).max()) == 0
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
    exe = tmp_path / "fetch_rollout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "fetch_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    desc = E.write_env_desc("FetchPickAndPlace-v4", str(tmp_path / "pick.grxenv"))
    n, steps = 64, 60
    res = subprocess.run(["timeout", "-k", "10", "300", str(exe), desc, str(n), str(steps)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split() for line in res.stdout.strip().splitlines())
    c = Handle("FetchPickAndPlace-v4", n, tmp_path, "same_step", 50)
    try:
        assert c.reset(seeds=1000 + np.arange(n)) == 0
        i, j = np.meshgrid(np.arange(n), np.arange(4), indexing="ij")
        finished = 0
        for t in range(steps):
            a = torch.from_numpy((((t * 11 + i * 7 + j * 3) % 17) / 8.0 - 1.0).astype(np.float32)).cuda()
            assert c.step(a) == 0
            finished += len(c.host()["final_idx"])
        packed = c.host()["packed"]
    finally:
        c.close()
    assert int(lines["finished"]) == finished == n
    assert int(lines["checksum"], 16) == _fnv1a(packed.tobytes())
