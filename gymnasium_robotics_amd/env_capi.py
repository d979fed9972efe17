"""Python side of the env-level C ABI (include/grx_env.h, libgrx_env.so): the Fetch family and the maze family (PointMaze-v3, AntMaze).

    python -m gymnasium_robotics_amd.env_capi describe FetchPickAndPlace-v4 pick.grxenv
    python -m gymnasium_robotics_amd.env_capi describe AntMaze_Large_Diverse_GR-v5 ant.grxenv continuing_task=False

writes the environment description file grx_env_create reads.  The file is built from the packaged model (models/*.npz) alone:
no GPU, no asset tree.  This module also holds the ctypes loader of libgrx_env.so, struct mirrors of grx_env.h and a parser of the
section tables both files use, and the struct mirrors of grx_replay.h (the HER replay attached to a handle: ReplayConfig, ReplayBatch) and of grx_episodes.h (the
store of finished episodes attached to a replay: EpisodesConfig, EpisodesBatch) and of grx_norm.h (the observation / goal normalizer attached to a handle: NormConfig,
NormStateHeader and the helpers of its state blob).

Container (little endian; the description file and the state blob of grx_env_get_state share it):

    header   80 bytes   magic[8] ("GRXENVD\\0" description / "GRXENVS\\0" state), u32 version, u32 n_sections, env_id[48] (NUL-padded),
                        i64 num_envs (0 in a description), u64 total_bytes (the whole file)
    table    n_sections x 40 bytes: name[24] (NUL-padded), u64 offset (from the start of the file), u64 bytes
    payload  the sections, each at an 8-byte aligned offset

Sections of a description (version 1):

    H I F                 model.pack() of the model after FetchVecEnv.__init__'s mocap-weld eq_data edit, at FETCH_CAPACITY (int32, int32, float64)
    H_rerun I_rerun F_rerun   the same model at RERUN_CAPACITY (the overflow re-run's tables)
    task                  the FetchTaskStruct bytes (struct grx_fetch_task)
    dims                  int32 [8]: nq, nv, nmocap, nu, obs_dim, obj_qadr (-1: no object), max_episode_steps, 0
    consts                float64 [11]: has_object, block_gripper, target_in_the_air, gripper_extra_height, target_offset[3], obj_range, target_range,
                          distance_threshold (FETCH_TASKS), dt (N_SUBSTEPS x timestep)
    fast_caps             int32 [3]: maxefc, jpool, maxcon of the FETCH_CAPACITY tables (the overflow re-run's soft thresholds)
    q0                    float64 [nq]: qpos0 with the task's initial_qpos applied
    mocap0                float64 [7 nmocap]: mocap_pos0 | mocap_quat0

Sections of a maze description (same version; told apart by the `family` section, which a Fetch description does not have):

    family                "maze" (NUL-padded to 8 bytes)
    H I F                 model.pack() of the model PointMazeVecEnv / AntMazeVecEnv steps (the ant at ANT_CAPACITY)
    task                  the PointTaskStruct bytes (struct grx_point_task)
    dims                  int32 [8]: nq, nv, nu, obs_dim, obs_skip (2 for the ant), number of goal cells, number of reset cells, max_episode_steps
    consts                float64 [8]: goal radius, position_noise_range, maze_size_scaling, dt (frame skip x timestep), continuing_task, reset_target, sparse reward, 0
    qpos0                 float64 [nq]
    goal_xy reset_xy      float64 [cells, 2]: Maze.unique_goal_locations / unique_reset_locations (cell centres)
"""
import ctypes
import os
import struct
import sys

import numpy as np

DESC_MAGIC, STATE_MAGIC = b"GRXENVD\0", b"GRXENVS\0"
DESC_VERSION, STATE_VERSION = 1, 1
HEADER = struct.Struct("<8sII48sqQ")       # 80 bytes
ENTRY = struct.Struct("<24sQQ")            # 40 bytes

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libgrx_env.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "grx_env.h")
REPLAY_HEADER_PATH = os.path.join(_HERE, "..", "include", "grx_replay.h")
EPISODES_HEADER_PATH = os.path.join(_HERE, "..", "include", "grx_episodes.h")
NORM_HEADER_PATH = os.path.join(_HERE, "..", "include", "grx_norm.h")
_lib = None

AUTORESET = {"next_step": 0, "same_step": 1, "disabled": 2}


# ------------------------------------------------------------------ container
def pack_sections(magic, version, env_id, num_envs, sections):
    """sections: list of (name, bytes-like) -> the whole file as bytes"""
    n = len(sections)
    off = HEADER.size + n * ENTRY.size
    table, payload = [], []
    for name, data in sections:
        data = bytes(data)
        off = -(-off // 8) * 8
        table.append((name, off, len(data)))
        payload.append((off, data))
        off += len(data)
    buf = bytearray(off)
    HEADER.pack_into(buf, 0, magic, version, n, env_id.encode(), int(num_envs), off)
    for k, (name, o, b) in enumerate(table):
        ENTRY.pack_into(buf, HEADER.size + k * ENTRY.size, name.encode(), o, b)
    for o, data in payload:
        buf[o: o + len(data)] = data
    return bytes(buf)


def section_table(blob):
    """-> (header dict, {name: (offset, bytes)}) of a description file or a state blob (no validation beyond the bounds)"""
    blob = bytes(blob)
    magic, version, n, env_id, num_envs, total = HEADER.unpack_from(blob, 0)
    head = dict(magic=magic, version=version, env_id=env_id.rstrip(b"\0").decode(), num_envs=num_envs, total_bytes=total)
    table = {}
    for k in range(n):
        name, off, size = ENTRY.unpack_from(blob, HEADER.size + k * ENTRY.size)
        if off + size > len(blob):
            raise ValueError(f"section {name!r} runs past the end of the blob")
        table[name.rstrip(b"\0").decode()] = (off, size)
    return head, table


def parse_sections(blob):
    """-> (header dict, {name: bytes})"""
    blob = bytes(blob)
    head, table = section_table(blob)
    return head, {k: blob[o: o + b] for k, (o, b) in table.items()}


def state_arrays(blob, obs_dim=None):
    """the sections of a grx_env_get_state blob as numpy arrays (float32 rows, int32 / uint8 / int64 / uint64 where the state holds those)"""
    head, sec = parse_sections(blob)
    n = head["num_envs"]
    dtypes = {"success": np.uint8, "status": np.int32, "cost": np.int32, "order": np.int32, "rng": np.uint64, "elapsed": np.int64, "needs_reset": np.uint8, "has_reset": np.uint8, "mask": np.uint8,
              "split_state": np.int32}
    out = {}
    for k, v in sec.items():
        a = np.frombuffer(v, dtype=dtypes.get(k, np.float32))
        out[k] = a if k == "has_reset" else a.reshape(n, -1)
    return head, out


# ------------------------------------------------------------------ description file
MAZE_KWARGS = {"continuing_task": True, "reset_target": False, "position_noise_range": 0.25}


def is_maze_id(env_id):
    return env_id.startswith("PointMaze_") or env_id.startswith("AntMaze_")


def describe_maze(env_id, **kwargs):
    """the description of a registered PointMaze / AntMaze id in the given mode (MAZE_KWARGS: the keyword arguments of PointMazeVecEnv with their defaults)"""
    from . import _native
    from .envs import maze_spec as ms
    from .envs.point_maze import AntMazeVecEnv, PointMazeVecEnv, load_point_maze_model

    unknown = set(kwargs) - set(MAZE_KWARGS)
    if unknown:
        raise TypeError(f"describe({env_id!r}): unknown keyword arguments {sorted(unknown)} (a maze description takes {sorted(MAZE_KWARGS)})")
    kw = dict(MAZE_KWARGS, **kwargs)
    cls = AntMazeVecEnv if env_id.startswith("AntMaze_") else PointMazeVecEnv
    layout, reward_type, max_episode_steps = cls._parse_id(env_id)
    maze = ms.Maze(ms.MAPS[layout], *cls.MAZE_GEOMETRY)
    model = load_point_maze_model(maze, layout, None, cls.AGENT)
    task = _native.PointTaskStruct(cls.N_SUBSTEPS, int(reward_type == "sparse"), int(bool(kw["continuing_task"])), int(cls.AGENT == "ant"), ms.GOAL_RADIUS, 5.0)
    nq, nv, nu = model.dim("nq"), model.dim("nv"), model.dim("nu")
    goal_xy = np.ascontiguousarray(np.asarray(maze.unique_goal_locations, dtype=np.float64).reshape(-1, 2))
    reset_xy = np.ascontiguousarray(np.asarray(maze.unique_reset_locations, dtype=np.float64).reshape(-1, 2))
    dims = np.array([nq, nv, nu, nq + nv - cls.OBS_SKIP, cls.OBS_SKIP, len(goal_xy), len(reset_xy), max_episode_steps or 0], np.int32)
    consts = np.array([ms.GOAL_RADIUS, float(kw["position_noise_range"]), maze.maze_size_scaling, cls.N_SUBSTEPS * model.opt("timestep"), float(bool(kw["continuing_task"])),
                       float(bool(kw["reset_target"])), float(reward_type == "sparse"), 0.0], np.float64)
    H, I, F = model.pack()
    f = lambda a, dt: np.ascontiguousarray(a, dtype=dt).tobytes()
    sections = [("family", b"maze\0\0\0\0"), ("H", f(H, np.int32)), ("I", f(I, np.int32)), ("F", f(F, np.float64)), ("task", bytes(task)), ("dims", dims.tobytes()),
                ("consts", consts.tobytes()), ("qpos0", f(model.tables["qpos0"], np.float64)), ("goal_xy", goal_xy.tobytes()), ("reset_xy", reset_xy.tobytes())]
    return pack_sections(DESC_MAGIC, DESC_VERSION, env_id, 0, sections)


def describe(env_id, **kwargs):
    """the description file of `env_id` as bytes (packaged model; no GPU).  Maze ids take the mode of the environment as keyword arguments (MAZE_KWARGS)."""
    if is_maze_id(env_id):
        return describe_maze(env_id, **kwargs)
    if kwargs:
        raise TypeError(f"describe({env_id!r}): a Fetch description takes no keyword arguments")
    from .core import RERUN_CAPACITY
    from .envs.fetch import FETCH_CAPACITY, load_fetch_model
    from .envs.fetch_spec import DISTANCE_THRESHOLD, FETCH_TASKS, MAX_EPISODE_STEPS, make_fetch_task, parse_env_id

    task, reward_type = parse_env_id(env_id)
    cfg = FETCH_TASKS[task]
    model = load_fetch_model(task).copy()
    eq = model.tables["eq_data"]      # reset_mocap_welds, as FetchVecEnv.__init__
    eq[model.tables["eq_type"] == 1, :7] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    t = make_fetch_task(model, task, reward_type)
    T, names = model.tables, model.names
    jq = T["jnt_qposadr"].ravel()
    q0 = T["qpos0"].astype(np.float64).copy()      # FetchVecEnv._env_setup
    for name, v in cfg["initial_qpos"].items():
        v = np.atleast_1d(np.asarray(v, dtype=np.float64))
        a = int(jq[names["joint"][name]])
        q0[a: a + len(v)] = v
    mocap0 = np.concatenate([T["mocap_pos0"].ravel(), T["mocap_quat0"].ravel()]).astype(np.float64)
    obj_qadr = int(jq[names["joint"]["object0:joint"]]) if cfg["has_object"] else -1
    H, I, F = model.pack()
    Hr, Ir, Fr = model.with_capacity(**RERUN_CAPACITY).pack()
    toff = np.broadcast_to(np.asarray(cfg["target_offset"], dtype=np.float64), (3,))
    dims = np.array([model.dim("nq"), model.dim("nv"), model.dim("nmocap"), model.dim("nu"), int(t.obs_dim), obj_qadr, MAX_EPISODE_STEPS, 0], np.int32)
    consts = np.array([cfg["has_object"], cfg["block_gripper"], cfg["target_in_the_air"], cfg["gripper_extra_height"], *toff, cfg["obj_range"], cfg["target_range"],
                       DISTANCE_THRESHOLD, float(t.n_substeps) * model.opt("timestep")], np.float64)
    caps = np.array([FETCH_CAPACITY["maxefc"], FETCH_CAPACITY["jpool"], FETCH_CAPACITY["maxcon"]], np.int32)
    f = lambda a, dt: np.ascontiguousarray(a, dtype=dt).tobytes()
    sections = [("H", f(H, np.int32)), ("I", f(I, np.int32)), ("F", f(F, np.float64)), ("H_rerun", f(Hr, np.int32)), ("I_rerun", f(Ir, np.int32)), ("F_rerun", f(Fr, np.float64)),
                ("task", bytes(t)), ("dims", dims.tobytes()), ("consts", consts.tobytes()), ("fast_caps", caps.tobytes()), ("q0", f(q0, np.float64)),
                ("mocap0", f(mocap0, np.float64))]
    return pack_sections(DESC_MAGIC, DESC_VERSION, env_id, 0, sections)


def write_env_desc(env_id, path, **kwargs):
    blob = describe(env_id, **kwargs)
    with open(path, "wb") as fh:
        fh.write(blob)
    return path


def read_env_desc(path):
    """-> (header, dict of numpy arrays / bytes) of a description file"""
    with open(path, "rb") as fh:
        head, sec = parse_sections(fh.read())
    if sec.get("family", b"").rstrip(b"\0") == b"maze":
        out = {k: np.frombuffer(sec[k], np.int32) for k in ("H", "I", "dims")}
        out.update({k: np.frombuffer(sec[k], np.float64) for k in ("F", "consts", "qpos0")})
        out.update({k: np.frombuffer(sec[k], np.float64).reshape(-1, 2) for k in ("goal_xy", "reset_xy")})
        out.update(task=sec["task"], family="maze")
        return head, out
    out = {k: np.frombuffer(sec[k], np.int32) for k in ("H", "I", "H_rerun", "I_rerun", "dims", "fast_caps")}
    out.update({k: np.frombuffer(sec[k], np.float64) for k in ("F", "F_rerun", "consts", "q0", "mocap0")})
    out["task"] = sec["task"]
    return head, out


# ------------------------------------------------------------------ grx_env.h mirrors
class EnvConfig(ctypes.Structure):
    _fields_ = [("autoreset_mode", ctypes.c_int), ("max_episode_steps", ctypes.c_int), ("seed_offset", ctypes.c_uint64)]


class EnvOutputs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("num_envs", "obs_dim", "goal_dim", "packed_dim")] + [
        (n, ctypes.c_void_p) for n in ("obs", "achieved", "desired", "reward", "success", "status", "packed", "terminated", "truncated")] + [
        ("n_final", ctypes.c_int), ("final_idx", ctypes.c_void_p), ("final_rows", ctypes.c_void_p)]


class EnvHostOutputs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("obs", "achieved", "desired", "reward", "success", "status", "packed", "terminated", "truncated", "n_final", "final_idx", "final_rows")]


# ------------------------------------------------------------------ grx_replay.h mirrors
class ReplayConfig(ctypes.Structure):
    _fields_ = [("horizon", ctypes.c_int), ("keep_final", ctypes.c_int), ("capacity", ctypes.c_int64), ("max_batch", ctypes.c_int64), ("seed", ctypes.c_uint64)]


class ReplayBatch(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_void_p), ("batch", ctypes.c_int64), ("offset", ctypes.c_int64), ("valid", ctypes.c_void_p)]


# ------------------------------------------------------------------ grx_episodes.h mirrors
EPISODES_STRATEGY = {"future": 0, "final": 1, "episode": 2}      # GRX_EPISODES_FUTURE / _FINAL / _EPISODE


class EpisodesConfig(ctypes.Structure):
    _fields_ = [("episodes", ctypes.c_int64), ("max_batch", ctypes.c_int64), ("seed", ctypes.c_uint64)]


class EpisodesBatch(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_void_p), ("batch", ctypes.c_int64), ("valid", ctypes.c_void_p)]


# ------------------------------------------------------------------ grx_norm.h mirrors
NORM_MAGIC, NORM_VERSION = b"GRXNORM\0", 1


class NormConfig(ctypes.Structure):
    _fields_ = [("eps", ctypes.c_double), ("clip", ctypes.c_float)]


class NormStateHeader(ctypes.Structure):
    """the first 40 bytes of a grx_norm_get_state blob; sum[D] f64, sumsq[D] f64, count i64, skipped i64 follow (D = obs_dim + goal_dim)"""
    _fields_ = [("magic", ctypes.c_char * 8), ("version", ctypes.c_uint32), ("obs_dim", ctypes.c_int32), ("goal_dim", ctypes.c_int32), ("zero0", ctypes.c_uint32),
                ("eps", ctypes.c_double), ("clip", ctypes.c_float), ("zero1", ctypes.c_uint32)]


def norm_state_size(obs_dim, goal_dim):
    return ctypes.sizeof(NormStateHeader) + 16 * (obs_dim + goal_dim) + 16


def pack_norm_state(obs_dim, goal_dim, eps, clip, total, sumsq, count, skipped):
    """the blob grx_norm_set_state reads (her.Normalizer.state_dict holds the same fields)"""
    D = obs_dim + goal_dim
    total, sumsq = np.ascontiguousarray(total, np.float64).reshape(D), np.ascontiguousarray(sumsq, np.float64).reshape(D)
    h = NormStateHeader(NORM_MAGIC, NORM_VERSION, obs_dim, goal_dim, 0, float(eps), float(clip), 0)
    return bytes(h) + total.tobytes() + sumsq.tobytes() + struct.pack("<qq", int(count), int(skipped))


def parse_norm_state(blob):
    """-> dict(obs_dim, goal_dim, eps, clip, sum, sumsq, count, skipped) of a grx_norm_get_state blob"""
    blob = bytes(blob)
    hs = ctypes.sizeof(NormStateHeader)
    if len(blob) < hs:
        raise ValueError("normalizer state blob shorter than its header")
    h = NormStateHeader.from_buffer_copy(blob[:hs])
    if bytes(h.magic).ljust(8, b"\0") != NORM_MAGIC or h.version != NORM_VERSION:
        raise ValueError("not a version-1 normalizer state blob")
    D = h.obs_dim + h.goal_dim
    if len(blob) != norm_state_size(h.obs_dim, h.goal_dim):
        raise ValueError(f"normalizer state blob of {len(blob)} bytes, expected {norm_state_size(h.obs_dim, h.goal_dim)}")
    count, skipped = struct.unpack_from("<qq", blob, hs + 16 * D)
    return dict(obs_dim=h.obs_dim, goal_dim=h.goal_dim, eps=h.eps, clip=h.clip, sum=np.frombuffer(blob, np.float64, D, hs).copy(),
                sumsq=np.frombuffer(blob, np.float64, D, hs + 8 * D).copy(), count=count, skipped=skipped)


def lib():
    """libgrx_env.so with its argument types (loads libgrx_hip.so first, through the package loader: one HIP runtime, the one torch uses)"""
    global _lib
    if _lib is None:
        from . import _native

        _native.lib()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, P = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER
        L.grx_env_create.argtypes = [ctypes.c_char_p, ci, ci, P(EnvConfig), P(vp)]
        L.grx_env_destroy.argtypes = [vp]
        L.grx_env_dims.argtypes = [vp, P(ci), P(ci), P(ci), P(ctypes.c_double)]
        L.grx_env_reset.argtypes = [vp, vp, vp, vp]
        L.grx_env_step.argtypes = [vp, vp, vp]
        L.grx_env_outputs.argtypes = [vp, P(EnvOutputs)]
        L.grx_env_copy_outputs.argtypes = [vp, P(EnvHostOutputs)]
        L.grx_env_compute_reward.argtypes = [vp, vp, vp, ctypes.c_int64, vp, vp]
        L.grx_env_state_size.argtypes = [vp, P(ctypes.c_size_t)]
        L.grx_env_get_state.argtypes = [vp, vp, ctypes.c_size_t]
        L.grx_env_set_state.argtypes = [vp, vp, ctypes.c_size_t]
        L.grx_env_seed_pcg64.argtypes = [vp, ci, vp]
        L.grx_env_last_error.restype = ctypes.c_char_p
        i64, u64 = ctypes.c_int64, ctypes.c_uint64
        L.grx_replay_create.argtypes = [vp, P(ReplayConfig), P(vp)]
        L.grx_replay_destroy.argtypes = [vp]
        L.grx_replay_dims.argtypes = [vp, P(ci), P(ci), P(ci), P(ci)]
        L.grx_replay_begin.argtypes = [vp, vp]
        L.grx_replay_append.argtypes = [vp, vp]
        L.grx_replay_relabel.argtypes = [vp, i64, ci, P(ReplayBatch), vp]
        L.grx_replay_reseed.argtypes = [vp, u64]
        L.grx_replay_ring.argtypes = [vp, P(vp), P(i64), P(i64), P(i64)]
        L.grx_episodes_create.argtypes = [vp, P(EpisodesConfig), P(vp)]
        L.grx_episodes_destroy.argtypes = [vp]
        L.grx_episodes_dims.argtypes = [vp, P(ci), P(ci), P(ci), P(ci)]
        L.grx_episodes_sample.argtypes = [vp, i64, ci, ci, P(EpisodesBatch), vp]
        L.grx_episodes_reseed.argtypes = [vp, u64]
        L.grx_episodes_store.argtypes = [vp, P(vp), P(vp), P(vp), P(vp), P(i64)]
        L.grx_norm_create.argtypes = [vp, P(NormConfig), P(vp)]
        L.grx_norm_destroy.argtypes = [vp]
        L.grx_norm_dims.argtypes = [vp, P(ci), P(ci), P(ci), P(ci)]
        L.grx_norm_update.argtypes = [vp, vp, i64, vp, vp]
        L.grx_norm_apply_batch.argtypes = [vp, vp, i64, vp, vp]
        L.grx_norm_policy_input.argtypes = [vp, P(vp), vp]
        L.grx_norm_stats.argtypes = [vp, P(vp), P(vp), P(vp), P(vp), P(vp), P(vp), P(ci)]
        L.grx_norm_state_size.argtypes = [vp, P(ctypes.c_size_t)]
        L.grx_norm_get_state.argtypes = [vp, vp, ctypes.c_size_t]
        L.grx_norm_set_state.argtypes = [vp, vp, ctypes.c_size_t]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(f"libgrx_env ({rc}): " + lib().grx_env_last_error().decode())


class _DeviceArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def device_view(ptr, shape, dtype=np.float32, device="cuda:0"):
    """a torch tensor over device memory the library owns (grx_env_outputs / grx_replay_relabel pointers): no copy, valid as long as the pointer is"""
    import torch

    return torch.as_tensor(_DeviceArray(ptr, shape, np.dtype(dtype).str), device=device)


def seed_pcg64(seeds):
    """numpy's PCG64(SeedSequence(s)) positions through the library: uint64 [n, 4] (state_hi, state_lo, inc_hi, inc_lo)"""
    s = np.ascontiguousarray(seeds, dtype=np.uint64)
    out = np.zeros((len(s), 4), np.uint64)
    check(lib().grx_env_seed_pcg64(s.ctypes.data, len(s), out.ctypes.data))
    return out


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) < 3 or argv[0] != "describe" or any("=" not in a for a in argv[3:]):
        print("usage: python -m gymnasium_robotics_amd.env_capi describe <env id> <path> [key=value ...]   (maze ids: " + ", ".join(MAZE_KWARGS) + ")", file=sys.stderr)
        return 2
    kwargs = {}
    words = {"1": True, "true": True, "0": False, "false": False}
    for a in argv[3:]:
        k, v = a.split("=", 1)
        try:
            if k not in MAZE_KWARGS or not is_maze_id(argv[1]):
                raise ValueError(f"unknown key {k!r}")
            kwargs[k] = float(v) if k == "position_noise_range" else words[v.strip().lower()]
        except (KeyError, ValueError):
            print(f"describe: cannot use {a!r} (keys: {', '.join(MAZE_KWARGS)}, for maze ids; flags take true / false / 1 / 0, position_noise_range a number)", file=sys.stderr)
            return 2
    write_env_desc(argv[1], argv[2], **kwargs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
