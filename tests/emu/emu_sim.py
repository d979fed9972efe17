"""ctypes harness for tests/emu/libgrx_emu.so (sequential lane emulator of the device engine).
TEST INFRASTRUCTURE ONLY -- lets the kernel source be checked against the oracle without a GPU."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.abspath(os.path.join(_HERE, "..", ".."))


def build(force=False):
    so = os.path.join(_HERE, "libgrx_emu.so")
    import glob

    srcs = [os.path.join(_HERE, "grx_emu.cpp")] + sorted(glob.glob(os.path.join(_ROOT, "gymnasium_robotics_amd", "csrc", "*.h"))) + sorted(
        glob.glob(os.path.join(_ROOT, "include", "*")))
    stale = lambda: force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale():
        import fcntl

        with open(so + ".lock", "w") as lk:      # pytest-xdist workers: one builds, the others wait and find the fresh library
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = f"{so}.{os.getpid()}.tmp"
                subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-Wno-misleading-indentation", "-o", tmp, srcs[0]], cwd=_HERE)
                os.replace(tmp, so)
                force = False
    return so


class EmuSim:
    def __init__(self, model, task_struct):
        self.model, self.task = model, task_struct
        self.L = ctypes.CDLL(build())
        self.L.emu_create.restype = ctypes.c_void_p
        self.L.emu_create.argtypes = [ctypes.c_void_p] * 3
        self.L.emu_ctx_ptr.restype = ctypes.POINTER(ctypes.c_float)
        self.L.emu_ctx_ptr.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        self.L.emu_set_table.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int]
        self.L.emu_ctx_words.argtypes = [ctypes.c_void_p]
        H, I, F = model.pack()
        self._keep = (H, I, F)
        self.h = self.L.emu_create(H.ctypes.data, I.ctypes.data, F.ctypes.data)
        self.nq, self.nv, self.nmocap = model.dim("nq"), model.dim("nv"), model.dim("nmocap")
        self.qpos = np.zeros(self.nq, np.float32)
        self.qvel = np.zeros(self.nv, np.float32)
        self.qacc_ws = np.zeros(self.nv, np.float32)
        self.mocap = np.zeros(7 * self.nmocap, np.float32)
        self.aux = np.zeros(8, np.float32)
        self.obs = np.zeros(getattr(task_struct, "obs_dim", self.nq + self.nv - (2 if getattr(task_struct, "agent", 0) else 0)), np.float32)
        self.achieved = np.zeros(3, np.float32)
        self.status = ctypes.c_int(0)

    def load_world(self, g, i, keys=("qpos", "qvel", "qacc_ws")):
        """state of fixture snapshot i -- recorded by the oracle in the MJCF's world frame -- into the emulated world's rows, which live in the MODEL's frame
        (CompiledModel.rows_from_world: the subtraction in fp64, one rounding to fp32)"""
        for k in keys:
            getattr(self, k)[:] = self.model.rows_from_world(k, g[k][i])

    def set_table(self, name, data):
        data = np.ascontiguousarray(data, dtype=np.float64)
        assert self.L.emu_set_table(ctypes.c_void_p(self.h), name.encode(), data.ctypes.data, data.size) == 0

    def _args(self):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        return [ctypes.c_void_p(self.h), ctypes.byref(self.task), p(self.qpos), p(self.qvel), p(self.qacc_ws), p(self.mocap), p(self.aux)]

    def step(self, action):
        a = np.ascontiguousarray(action, dtype=np.float32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        self.L.emu_fetch_step(*self._args(), p(a), p(self.obs), p(self.achieved), ctypes.byref(self.status))

    def forward(self, nstep=0):
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        self.L.emu_forward(*self._args(), p(self.obs), p(self.achieved), ctypes.byref(self.status), ctypes.c_int(nstep))

    def ctx(self, name, n, dtype=np.float32):
        ptr = self.L.emu_ctx_ptr(ctypes.c_void_p(self.h), name.encode())
        a = np.ctypeslib.as_array(ptr, shape=(n,)).copy()
        return a.view(np.int32) if dtype == np.int32 else a


    def physics_steps(self, nstep=1, ctrl=None):
        """nstep raw physics steps of the loaded state (self.qpos / qvel / qacc_ws); returns (ncon, nefc) of the last one"""
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        c = None if ctrl is None else p(np.ascontiguousarray(ctrl, dtype=np.float32))
        ncon, nefc = ctypes.c_int(0), ctypes.c_int(0)
        self.L.emu_physics_steps(ctypes.c_void_p(self.h), p(self.qpos), p(self.qvel), p(self.qacc_ws), c, ctypes.byref(self.status), ctypes.byref(ncon), ctypes.byref(nefc),
                                 ctypes.c_int(nstep))
        return ncon.value, nefc.value

    def contact_list(self, cap=64):
        """the contact list of the loaded state (self.qpos / qvel), copied out between the constraint and the velocity stage, where the device's contact outputs read it;
        returns dict(ncon, nefc, status, pair [n], dist [n], pos [n, 3], normal [n, 3]) in the order of the device's contact outputs: by candidate pair, a pair's
        contacts in the engine's order"""
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        cnt, pair = np.zeros(3, np.int32), np.zeros(cap, np.int32)
        dist, pos, nrm = np.zeros(cap, np.float32), np.zeros(3 * cap, np.float32), np.zeros(3 * cap, np.float32)
        n = self.L.emu_contact_list(ctypes.c_void_p(self.h), p(self.qpos), p(self.qvel), ctypes.c_int(cap), p(cnt), p(pair), p(dist), p(pos), p(nrm))
        return dict(ncon=int(cnt[0]), nefc=int(cnt[1]), status=int(cnt[2]), pair=pair[:n].copy(), dist=dist[:n].copy(), pos=pos.reshape(cap, 3)[:n].copy(),
                    normal=nrm.reshape(cap, 3)[:n].copy())

    def touch(self, mode=1, nstep=0, ncon_max=64):
        """the touch readings of the loaded state (self.qpos / qvel, zero warm start) on the generic engine: mode 1 raw, 2 value > 0, 3 log(value + 1), 4 clip(value, -1, 1);
        nstep = 0 after one forward pass, nstep > 0 after nstep physics steps (those of the last pass, as BatchedSim's sensordata).  Returns dict(sensordata [ntouch], ncon,
        nefc, status) and, of the SAME pass, what the readings were made from: xpos [nbody, 3], xquat [nbody, 4], the engine's contact list in its own order -- pair [ncon],
        pos [ncon, 3], normal [ncon, 3], efc_address [ncon] (-1: no rows), force [ncon] (the sum of the contact's rows of efc_force)"""
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        nt = len(np.asarray(self.model.tables.get("touch_body", [])).reshape(-1))
        out, cnt = np.zeros(max(nt, 1), np.float32), np.zeros(3, np.int32)
        self.L.emu_touch(ctypes.c_void_p(self.h), p(self.qpos), p(self.qvel), ctypes.c_int(mode), p(out), ctypes.c_int(nstep), p(cnt))
        ncon, nefc, nb = int(cnt[0]), int(cnt[1]), self.model.dim("nbody")
        assert ncon <= ncon_max
        adr, nr = self.ctx("con_efc", ncon_max, np.int32)[:ncon], self.ctx("con_nr", ncon_max, np.int32)[:ncon]
        f = self.ctx("efc_force", max(nefc, 1))

        def rows_sum(a, n):      # fp32, row by row: contact_force[..., 0] of the device's contact outputs (grx_sim_contact_force)
            acc = np.float32(0.0)
            for x in f[a:min(a + n, nefc)]:
                acc = np.float32(acc + x)
            return float(acc)

        force = np.array([rows_sum(a, n) if a >= 0 else 0.0 for a, n in zip(adr, nr)])
        return dict(sensordata=out[:nt].copy(), ncon=ncon, nefc=nefc, status=int(cnt[2]), xpos=self.ctx("xpos", 3 * nb).reshape(nb, 3), xquat=self.ctx("xquat", 4 * nb).reshape(nb, 4),
                    pair=self.ctx("con_pair", ncon_max, np.int32)[:ncon], pos=self.ctx("con_pos", 3 * ncon_max).reshape(-1, 3)[:ncon],
                    normal=self.ctx("con_frame", 3 * ncon_max).reshape(-1, 3)[:ncon], efc_address=adr, force=force)

    def kitchen_step(self, action, last_qpos, noise=None, forward_only=False):
        """FrankaKitchen env.step() (or the reset-time forward pass) of one world; last_qpos is updated in place; returns (obs[59], completed mask)"""
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        a = np.ascontiguousarray(action, dtype=np.float32)
        nz = None if noise is None else p(np.ascontiguousarray(noise, dtype=np.float32))
        obs, done = np.zeros(int(self.task.obs_dim), np.float32), ctypes.c_int(0)
        assert last_qpos.dtype == np.float32 and last_qpos.shape == (9,)
        self.L.emu_kitchen_step(ctypes.c_void_p(self.h), ctypes.byref(self.task), p(self.qpos), p(self.qvel), p(self.qacc_ws), p(last_qpos), p(a), nz, p(obs),
                                ctypes.byref(done), ctypes.byref(self.status), ctypes.c_int(int(forward_only)))
        return obs, done.value

    def point_step(self, action):
        a = np.ascontiguousarray(action, dtype=np.float32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        self.L.emu_point_step(ctypes.c_void_p(self.h), ctypes.byref(self.task), p(self.qpos), p(self.qvel), p(self.qacc_ws), p(a), p(self.obs),
                              p(self.achieved), ctypes.byref(self.status))

    def hand_step(self, action, forward_only=False):
        a = np.ascontiguousarray(action, dtype=np.float32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        if not hasattr(self, "hand_obs"):
            self.hand_obs = np.zeros(256, np.float32)
            self.hand_achieved = np.zeros(15, np.float32)
            self.palm = np.zeros(3, np.float32)
        self.L.emu_hand_step(ctypes.c_void_p(self.h), ctypes.byref(self.task), p(self.qpos), p(self.qvel), p(self.qacc_ws), p(a), p(self.hand_obs),
                             p(self.hand_achieved), p(self.palm), ctypes.byref(self.status), ctypes.c_int(int(forward_only)))

    def adroit_step(self, action, shift, act_mean, act_rng, forward_only=False, target=None):
        """Adroit env.step() (or the reset-time forward pass) of one world; shift = the world's 7-vector group pose; returns (obs, reward, success)"""
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        a, sh = np.ascontiguousarray(action, dtype=np.float32), np.ascontiguousarray(shift, dtype=np.float32)
        assert sh.shape == (7,)
        tg = np.ascontiguousarray(np.zeros(3) if target is None else target, dtype=np.float32)
        am, ar = np.ascontiguousarray(act_mean, dtype=np.float32), np.ascontiguousarray(act_rng, dtype=np.float32)
        obs, rew, suc = np.zeros(int(self.task.obs_dim), np.float32), ctypes.c_float(0), ctypes.c_ubyte(0)
        self.L.emu_adroit_step(ctypes.c_void_p(self.h), ctypes.byref(self.task), p(self.qpos), p(self.qvel), p(self.qacc_ws), p(sh), p(tg), p(a), p(am), p(ar), p(obs),
                               ctypes.byref(rew), ctypes.byref(suc), ctypes.byref(self.status), ctypes.c_int(int(forward_only)))
        return obs, float(rew.value), int(suc.value)
