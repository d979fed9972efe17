"""CPU checks of the maze half of the env-level C ABI (include/grx_env.h, libgrx_env.so, gymnasium_robotics_amd/env_capi.py): the description file of every
registered PointMaze / AntMaze id, the unchanged bytes of the Fetch descriptions, the parse errors of grx_env_create on maze descriptions and a C99 build of the
worked example (tests/capi/maze_rollout.c).  None of these needs a GPU."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# sha256 of describe(id) at the commit before the maze family was added: a Fetch description does not change
FETCH_SHA256 = {
    "FetchReach-v4": (1071800, "6ecc483e8558bef5d87f9c957161d68d993a005fc722f59d138b770dd5ac2913"),
    "FetchReachDense-v4": (1071800, "c5ea337f4df7d9257d92992c2de8cb90d502258c738446dcdcb1dc5b26860226"),
    "FetchPush-v4": (1080976, "ceac9f69c0c9ea3585c2ede11e6e29528175c825a0260548fd6b364c131891e1"),
    "FetchPushDense-v4": (1080976, "a10bef0afedaa43ed7ac5f91b51ce41b8aa550128c3be8b903a34a3b8f70f4e3"),
    "FetchSlide-v4": (1080976, "70fb5a93020222cc2db05597455b177725689a515da5e6874506f43703bad302"),
    "FetchSlideDense-v4": (1080976, "5fde83db441ccd5118064163946d07196b8d05b2a227e9c7fa7d33fe7f3e8259"),
    "FetchPickAndPlace-v4": (1081424, "e81de0e19c4d4f487347c48ef6f00e30b91390b1aafbd557255501ab76113e52"),
    "FetchPickAndPlaceDense-v4": (1081424, "078708744a3d6597650423fb71617d0481f18c09f954ca37af294d0692b2c095"),
}


def _env_capi():
    from gymnasium_robotics_amd import env_capi

    return env_capi


def _maze_ids():
    import gymnasium_robotics_amd as grx

    return [i for i in grx.registered_env_ids() if i.startswith("PointMaze_") or i.startswith("AntMaze_")]


MAZE_IDS = _maze_ids()


def test_every_registered_maze_id_is_covered():
    assert len(MAZE_IDS) >= 40 and any(i.startswith("AntMaze_") for i in MAZE_IDS) and any(i.startswith("PointMaze_") for i in MAZE_IDS)


@pytest.mark.parametrize("kw", [{}, {"continuing_task": False}, {"reset_target": True, "position_noise_range": 0.125}], ids=["default", "episodic", "reset_target"])
@pytest.mark.parametrize("env_id", MAZE_IDS)
def test_maze_description_round_trips(env_id, kw, tmp_path):
    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd.envs import maze_spec as ms
    from gymnasium_robotics_amd.envs.point_maze import ANT_CAPACITY, AntMazeVecEnv, PointMazeVecEnv, load_point_maze_model

    E = _env_capi()
    path = E.write_env_desc(env_id, str(tmp_path / "env.grxenv"), **kw)
    head, d = E.read_env_desc(path)
    assert head["magic"] == E.DESC_MAGIC and head["version"] == E.DESC_VERSION == 1 and head["env_id"] == env_id and head["total_bytes"] == os.path.getsize(path)
    assert d["family"] == "maze"
    cls = AntMazeVecEnv if env_id.startswith("AntMaze_") else PointMazeVecEnv
    layout, reward_type, horizon = cls._parse_id(env_id)
    maze = ms.Maze(ms.MAPS[layout], *cls.MAZE_GEOMETRY)
    model = load_point_maze_model(maze, layout, None, cls.AGENT)      # what the Python environment steps
    if cls.AGENT == "ant":
        assert all(model.dim(k + "_req") == ANT_CAPACITY[k] for k in ("maxcon", "maxefc", "jpool"))
    H, I, F = model.pack()
    assert np.array_equal(d["H"], H) and np.array_equal(d["I"], I) and np.array_equal(d["F"], F)
    continuing, reset_target, noise = kw.get("continuing_task", True), kw.get("reset_target", False), kw.get("position_noise_range", 0.25)
    task = _native.PointTaskStruct(cls.N_SUBSTEPS, int(reward_type == "sparse"), int(continuing), int(cls.AGENT == "ant"), ms.GOAL_RADIUS, 5.0)      # PointMazeVecEnv.__init__
    assert d["task"] == bytes(task)
    nq, nv = model.dim("nq"), model.dim("nv")
    assert list(d["dims"]) == [nq, nv, model.dim("nu"), nq + nv - cls.OBS_SKIP, cls.OBS_SKIP, len(maze.unique_goal_locations), len(maze.unique_reset_locations), horizon]
    assert list(d["consts"]) == [ms.GOAL_RADIUS, noise, maze.maze_size_scaling, cls.N_SUBSTEPS * model.opt("timestep"), float(continuing), float(reset_target),
                                 float(reward_type == "sparse"), 0.0]
    assert np.array_equal(d["qpos0"], model.tables["qpos0"].astype(np.float64).ravel())
    assert np.array_equal(d["goal_xy"], np.asarray(maze.unique_goal_locations, np.float64).reshape(-1, 2))
    assert np.array_equal(d["reset_xy"], np.asarray(maze.unique_reset_locations, np.float64).reshape(-1, 2))


@pytest.mark.parametrize("env_id", sorted(FETCH_SHA256))
def test_fetch_descriptions_are_byte_identical(env_id):
    blob = _env_capi().describe(env_id)
    size, sha = FETCH_SHA256[env_id]
    assert len(blob) == size and hashlib.sha256(blob).hexdigest() == sha


def test_describe_arguments():
    E = _env_capi()
    with pytest.raises(TypeError):
        E.describe("PointMaze_UMaze-v3", maze_map=[[1, 1], [1, 1]])      # custom maps need the asset tree: not part of a description
    with pytest.raises(TypeError):
        E.describe("FetchReach-v4", continuing_task=False)
    with pytest.raises(KeyError):
        E.describe("PointMaze_Nowhere-v3")


def test_describe_command_line(tmp_path):
    E = _env_capi()
    path = str(tmp_path / "cli.grxenv")
    assert E.main(["describe", "PointMaze_Open_Diverse_G-v3", path, "continuing_task=False", "position_noise_range=0.125"]) == 0
    assert open(path, "rb").read() == E.describe("PointMaze_Open_Diverse_G-v3", continuing_task=False, position_noise_range=0.125)
    for bad in ("reset_target", "continuing_task=flase", "reset_target=maybe", "maze_map=1", "position_noise_range=wide"):
        assert E.main(["describe", "PointMaze_Open-v3", path, bad]) == 2, bad
    assert E.main(["describe", "FetchReach-v4", path, "continuing_task=false"]) == 2


def _create(path, n=8):
    E = _env_capi()
    h = ctypes.c_void_p()
    rc = E.lib().grx_env_create(str(path).encode(), n, 0, None, ctypes.byref(h))
    return rc, E.lib().grx_env_last_error().decode(), h


@pytest.mark.parametrize("env_id", ["PointMaze_Medium_Diverse_GR-v3", "AntMaze_UMaze-v5"])
def test_create_without_a_device_and_parse_errors(env_id, tmp_path):
    import torch

    E = _env_capi()
    blob = E.describe(env_id)
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
    pack = lambda pairs: E.pack_sections(E.DESC_MAGIC, E.DESC_VERSION, env_id, 0, pairs)
    dims = np.frombuffer(sec["dims"], np.int32).copy()
    dims[3] += 1      # obs_dim no longer nq + nv - obs_skip
    cases = {
        "truncated": (blob[: len(blob) // 2], "truncated"),
        "tiny": (blob[:40], "truncated"),
        "qpos0 size": (pack([(k, sec[k][:-8] if k == "qpos0" else sec[k]) for k in names]), "inconsistent sizes"),
        "goal cells": (pack([(k, sec[k][:-16] if k == "goal_xy" else sec[k]) for k in names]), "inconsistent sizes"),
        "task size": (pack([(k, sec[k] + b"\0" * 8 if k == "task" else sec[k]) for k in names]), "inconsistent sizes"),
        "dims": (pack([(k, dims.tobytes() if k == "dims" else sec[k]) for k in names]), "inconsistent sizes"),
        "task": (pack([(k, sec[k]) for k in names if k != "task"]), "section 'task' is missing"),
        "reset cells": (pack([(k, sec[k]) for k in names if k != "reset_xy"]), "section 'reset_xy' is missing"),
        "modes": (pack([(k, (sec[k][:32] + np.float64(0.0).tobytes() + sec[k][40:]) if k == "consts" else sec[k]) for k in names]), "disagree with the task struct"),
        "family": (pack([(k, b"mazes\0\0\0" if k == "family" else sec[k]) for k in names]), "unknown family 'mazes'"),
    }
    for name, (data, want) in cases.items():
        p = tmp_path / f"{name.replace(' ', '_')}.grxenv"
        p.write_bytes(data)
        rc, msg, h = _create(p)
        assert rc == -2 and want in msg, (name, rc, msg)
        assert not h.value, name


def test_maze_rollout_example_builds_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    E = _env_capi()
    E.lib()
    libdir = os.path.dirname(E.LIB_PATH)
    exe = tmp_path / "maze_rollout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "capi", "maze_rollout.c"), "-L", libdir, "-lgrx_env", "-lgrx_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert exe.exists()
