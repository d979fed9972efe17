"""CPU checks of the env-level C ABI of the Fetch family (include/grx_env.h, libgrx_env.so, gymnasium_robotics_amd/env_capi.py):
the exported symbols, numpy-exact PCG64 seeding, the description file round trip, the parse errors of grx_env_create and a C99 build of
the worked example (tests/capi/fetch_rollout.c).  None of these needs a GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "grx_env.h")
FETCH_IDS = [f"{t}{d}-v4" for t in ("FetchReach", "FetchPush", "FetchSlide", "FetchPickAndPlace") for d in ("", "Dense")]


def _env_capi():
    from gymnasium_robotics_amd import env_capi

    return env_capi


def test_every_declared_entry_point_is_exported():
    import ctypes

    E = _env_capi()
    E.lib()
    names = set(re.findall(r"\b(grx_env_\w+)\s*\(", open(HEADER).read()))
    assert len(names) == 13, names
    raw = ctypes.CDLL(E.LIB_PATH)
    missing = [n for n in sorted(names) if not hasattr(raw, n)]
    assert not missing, missing


def test_seed_pcg64_is_numpys_seed_sequence():
    E = _env_capi()
    rng = np.random.default_rng(1234)
    seeds = [0, 1, 2**32 - 1, 2**32, 2**64 - 1] + [int(x) for x in rng.integers(0, 2**63, 50, dtype=np.int64)] + [int(x) for x in rng.integers(0, 2**32, 50, dtype=np.int64)]
    got = E.seed_pcg64(np.array(seeds, dtype=np.uint64))
    mask = (1 << 64) - 1
    for s, row in zip(seeds, got):
        st = np.random.PCG64(np.random.SeedSequence(s)).state["state"]
        want = [st["state"] >> 64, st["state"] & mask, st["inc"] >> 64, st["inc"] & mask]
        assert [int(x) for x in row] == want, s


@pytest.mark.parametrize("env_id", FETCH_IDS)
def test_description_file_round_trips(env_id, tmp_path):
    from gymnasium_robotics_amd.core import RERUN_CAPACITY
    from gymnasium_robotics_amd.envs.fetch import load_fetch_model
    from gymnasium_robotics_amd.envs.fetch_spec import DISTANCE_THRESHOLD, FETCH_TASKS, MAX_EPISODE_STEPS, make_fetch_task, parse_env_id

    E = _env_capi()
    path = E.write_env_desc(env_id, str(tmp_path / "env.grxenv"))
    head, d = E.read_env_desc(path)
    assert head["magic"] == E.DESC_MAGIC and head["version"] == E.DESC_VERSION and head["env_id"] == env_id and head["total_bytes"] == os.path.getsize(path)
    task, rt = parse_env_id(env_id)
    cfg = FETCH_TASKS[task]
    m = load_fetch_model(task).copy()
    m.tables["eq_data"][m.tables["eq_type"] == 1, :7] = [0, 0, 0, 0, 0, 0, 1]
    for suffix, model in (("", m), ("_rerun", m.with_capacity(**RERUN_CAPACITY))):
        H, I, F = model.pack()
        assert np.array_equal(d["H" + suffix], H) and np.array_equal(d["I" + suffix], I) and np.array_equal(d["F" + suffix], F), suffix
    assert d["task"] == bytes(make_fetch_task(m, task, rt))
    c = d["consts"]
    assert list(c[:4]) == [float(cfg["has_object"]), float(cfg["block_gripper"]), float(cfg["target_in_the_air"]), cfg["gripper_extra_height"]]
    assert np.array_equal(c[4:7], np.broadcast_to(np.asarray(cfg["target_offset"], np.float64), (3,)))
    assert list(c[7:10]) == [cfg["obj_range"], cfg["target_range"], DISTANCE_THRESHOLD]
    nq = m.dim("nq")
    assert list(d["dims"][:5]) == [nq, m.dim("nv"), m.dim("nmocap"), m.dim("nu"), 25 if cfg["has_object"] else 10]
    assert d["dims"][6] == MAX_EPISODE_STEPS
    jq = m.tables["jnt_qposadr"].ravel()
    for name, v in cfg["initial_qpos"].items():
        a = int(jq[m.names["joint"][name]])
        assert np.array_equal(d["q0"][a: a + len(np.atleast_1d(v))], np.atleast_1d(np.asarray(v, np.float64))), name
    assert d["dims"][5] == (int(jq[m.names["joint"]["object0:joint"]]) if cfg["has_object"] else -1)


def _create(path, n=8):
    import ctypes

    E = _env_capi()
    h = ctypes.c_void_p()
    rc = E.lib().grx_env_create(str(path).encode(), n, 0, None, ctypes.byref(h))
    return rc, E.lib().grx_env_last_error().decode(), h


def _rewrite(blob, **fields):
    """the description with header fields replaced"""
    E = _env_capi()
    magic, version, n, env_id, num_envs, total = E.HEADER.unpack_from(blob, 0)
    vals = dict(magic=magic, version=version, n=n, env_id=env_id, num_envs=num_envs, total=total)
    vals.update(fields)
    out = bytearray(blob)
    E.HEADER.pack_into(out, 0, vals["magic"], vals["version"], vals["n"], vals["env_id"], vals["num_envs"], vals["total"])
    return bytes(out)


def test_create_without_a_device_and_parse_errors(tmp_path):
    import torch

    E = _env_capi()
    blob = E.describe("FetchPush-v4")
    good = tmp_path / "good.grxenv"
    good.write_bytes(blob)
    rc, msg, h = _create(good)
    if torch.cuda.device_count() == 0:
        assert rc == -3 and "no HIP device" in msg, (rc, msg)
    else:      # (the suite also runs on the GPU machines: there the valid file makes a handle)
        assert rc == 0, msg
        assert E.lib().grx_env_destroy(h) == 0

    _, sec = E.parse_sections(blob)
    names = list(sec)
    bad_q0 = E.pack_sections(E.DESC_MAGIC, E.DESC_VERSION, "FetchPush-v4", 0, [(k, sec[k][:-8] if k == "q0" else sec[k]) for k in names])
    bad_rerun = E.pack_sections(E.DESC_MAGIC, E.DESC_VERSION, "FetchPush-v4", 0, [(k, sec[k][:-4] if k == "I_rerun" else sec[k]) for k in names])
    missing = E.pack_sections(E.DESC_MAGIC, E.DESC_VERSION, "FetchPush-v4", 0, [(k, sec[k]) for k in names if k != "task"])
    cases = {
        "magic": (_rewrite(blob, magic=b"NOTADESC"), "wrong magic"),
        "version": (_rewrite(blob, version=E.DESC_VERSION + 1), "unsupported version"),
        "truncated": (blob[: len(blob) // 2], "truncated"),
        "tiny": (blob[:40], "truncated"),
        "q0 size": (bad_q0, "inconsistent sizes"),
        "rerun size": (bad_rerun, "inconsistent sizes"),
        "section": (missing, "section 'task' is missing"),
    }
    for name, (data, want) in cases.items():
        p = tmp_path / f"{name.replace(' ', '_')}.grxenv"
        p.write_bytes(data)
        rc, msg, h = _create(p)
        assert rc == -2 and want in msg, (name, rc, msg)
        assert not h.value, name
    rc, msg, _ = _create(tmp_path / "does_not_exist.grxenv")
    assert rc == -2 and "cannot open" in msg


def test_null_arguments_are_refused():
    import ctypes

    L = _env_capi().lib()
    h = ctypes.c_void_p()
    assert L.grx_env_create(None, 4, 0, None, ctypes.byref(h)) == -1 and b"NULL" in L.grx_env_last_error()
    assert L.grx_env_step(None, None, None) == -1
    assert L.grx_env_reset(None, None, None, None) == -1
    assert L.grx_env_destroy(None) == -1


def test_rollout_example_builds_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    E = _env_capi()
    E.lib()
    libdir = os.path.dirname(E.LIB_PATH)
    exe = tmp_path / "fetch_rollout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "fetch_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert exe.exists()
