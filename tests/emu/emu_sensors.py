"""ctypes harness for tests/emu/libgrx_emu_sensors.so: the lane emulator with the sensor block (csrc/grx_sim_sensors.h).
TEST INFRASTRUCTURE ONLY -- lets the sensor routines be checked against the fp64 reference (tests/sensor_refs.py) without a GPU."""
import ctypes
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.abspath(os.path.join(_HERE, "..", ".."))
_CSRC = os.path.join(_ROOT, "gymnasium_robotics_amd", "csrc")
HEADER = os.path.join(_CSRC, "grx_sim_sensors.h")
_LIB = None
PHASE = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)


def _compile(so, src, flags=()):
    import fcntl

    with open(so + ".lock", "w") as lk:      # pytest-xdist workers: one builds, the others wait and find the fresh library
        fcntl.flock(lk, fcntl.LOCK_EX)
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-Wno-misleading-indentation", *flags, "-o", tmp, src], cwd=_HERE)
        os.replace(tmp, so)


def build(force=False):
    so = os.path.join(_HERE, "libgrx_emu_sensors.so")
    srcs = [os.path.join(_HERE, "grx_emu_sensors.cpp"), os.path.join(_HERE, "grx_emu.cpp")] + sorted(glob.glob(os.path.join(_CSRC, "*.h"))) + sorted(glob.glob(os.path.join(_ROOT, "include", "*")))
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        _compile(so, srcs[0])
    return so


def build_phases(header, so):
    """the two phases alone, compiled from the header text at `header` (a mutated copy: tests/test_cpu_sensors.py) into `so`; returns the loaded library"""
    _compile(so, os.path.join(_HERE, "grx_emu_sensors.cpp"), ("-DGRX_EMU_SENSORS_ONLY=1", f'-DGRX_SENSORS_HEADER="{header}"', "-I", _CSRC))
    return ctypes.CDLL(so)


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        _LIB.emu_create.restype = ctypes.c_void_p
        _LIB.emu_create.argtypes = [ctypes.c_void_p] * 3
        _LIB.emu_destroy.argtypes = [ctypes.c_void_p]
    return _LIB


class EmuSensors:
    """one emulated world of `model` with the sensor table spec [n, 4] / cutoff [n] (sim._sensor_spec / sim._sensor_cut)"""

    def __init__(self, model, spec, cutoff):
        self.L, self.model = lib(), model
        H, I, F = model.pack()
        self._keep = (H, I, F)
        self.h = self.L.emu_create(H.ctypes.data, I.ctypes.data, F.ctypes.data)
        self.spec = np.ascontiguousarray(spec, dtype=np.int32).reshape(-1, 4)
        self.cutoff = np.ascontiguousarray(cutoff, dtype=np.float32)
        self.ndata = int(sum(4 if t == 7 else (3 if t >= 6 else 1) for t in self.spec[:, 0]))
        self.nv, self.nu = model.dim("nv"), model.dim("nu")

    def run(self, qpos, qvel, ctrl=None, nstep=0, phases=None, fill=np.nan):
        """(sensordata [ndata], qacc [nv]) of the pass the readings belong to; phases: a library of build_phases, or None for the header as it is"""
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        q, v = np.ascontiguousarray(qpos, dtype=np.float32), np.ascontiguousarray(qvel, dtype=np.float32)
        u = None if ctrl is None or not self.nu else np.ascontiguousarray(ctrl, dtype=np.float32)
        out, qacc = np.full(max(self.ndata, 1), fill, np.float32), np.zeros(max(self.nv, 1), np.float32)
        p1 = p2 = None
        if phases is not None:
            p1, p2 = ctypes.cast(phases.emu_sns_p1, ctypes.c_void_p), ctypes.cast(phases.emu_sns_p2, ctypes.c_void_p)
        self.L.emu_sensors(ctypes.c_void_p(self.h), p(q), p(v), None if u is None else p(u), p(self.spec), p(self.cutoff), ctypes.c_int(len(self.spec)), ctypes.c_int(self.ndata), p(out),
                           ctypes.c_int(nstep), p1, p2, p(qacc))
        return out[:self.ndata].copy(), qacc[:self.nv].copy()

    def close(self):
        if self.h:
            self.L.emu_destroy(ctypes.c_void_p(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
