"""CPU checks of the HER replay of the env-level C ABI (include/grx_replay.h, libgrx_env.so): the exported symbols, that grx_env.h kept its thirteen calls, the argument
checks that need no device, and a C99 build of the worked example (tests/capi/replay_rollout.c) against both headers.  None of these needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENV_HEADER = os.path.join(ROOT, "include", "grx_env.h")
REPLAY_HEADER = os.path.join(ROOT, "include", "grx_replay.h")
CALLS = {"create", "destroy", "dims", "begin", "append", "relabel", "reseed", "ring"}


def _E():
    from gymnasium_robotics_amd import env_capi

    return env_capi


def test_every_declared_replay_entry_point_is_exported():
    E = _E()
    E.lib()
    names = set(re.findall(r"\b(grx_replay_\w+)\s*\(", open(REPLAY_HEADER).read()))
    assert names == {"grx_replay_" + c for c in CALLS}, names
    raw = ctypes.CDLL(E.LIB_PATH)
    missing = [n for n in sorted(names) if not hasattr(raw, n)]
    assert not missing, missing


def test_env_header_keeps_its_thirteen_calls():
    text = open(ENV_HEADER).read()
    assert len(set(re.findall(r"\b(grx_env_\w+)\s*\(", text))) == 13
    assert "grx_replay_" not in text.replace("grx_replay.h", "")      # the headers cross-reference each other by file name only
    assert '#include "grx_env.h"' in open(REPLAY_HEADER).read()


def test_struct_mirrors_match_the_header_layout():
    E = _E()
    assert ctypes.sizeof(E.ReplayConfig) == 32 and E.ReplayConfig.capacity.offset == 8 and E.ReplayConfig.seed.offset == 24
    assert ctypes.sizeof(E.ReplayBatch) == 32 and E.ReplayBatch.valid.offset == 24


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    E = _E()
    L = E.lib()
    err = lambda: L.grx_env_last_error().decode()
    r = ctypes.c_void_p()
    good = E.ReplayConfig(horizon=50, keep_final=1, capacity=1024, max_batch=256, seed=0)
    assert L.grx_replay_create(None, ctypes.byref(good), ctypes.byref(r)) == -1 and "NULL handle" in err() and not r.value
    assert L.grx_replay_create(None, ctypes.byref(good), None) == -1 and "out is NULL" in err()
    assert L.grx_replay_create(None, None, ctypes.byref(r)) == -1 and "NULL config" in err()
    for field, value, want in (("horizon", 0, "horizon 0"), ("horizon", -3, "horizon -3"), ("capacity", 0, "capacity 0"), ("max_batch", 1025, "batch 1025 larger than the replay capacity 1024")):
        cfg = E.ReplayConfig(horizon=50, keep_final=1, capacity=1024, max_batch=256, seed=0)
        setattr(cfg, field, value)
        assert L.grx_replay_create(None, ctypes.byref(cfg), ctypes.byref(r)) == -1 and want in err(), (field, err())
        assert not r.value
    batch = E.ReplayBatch()
    for rc in (L.grx_replay_destroy(None), L.grx_replay_begin(None, None), L.grx_replay_append(None, None), L.grx_replay_relabel(None, 4, 4, ctypes.byref(batch), None),
               L.grx_replay_reseed(None, 1), L.grx_replay_dims(None, None, None, None, None), L.grx_replay_ring(None, None, None, None, None)):
        assert rc == -1 and "NULL replay" in err(), err()


def test_replay_example_builds_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    E = _E()
    E.lib()
    libdir = os.path.dirname(E.LIB_PATH)
    exe = tmp_path / "replay_rollout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "replay_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert exe.exists()
