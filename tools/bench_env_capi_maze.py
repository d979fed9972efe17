"""A/B of the two maze step paths in one process: PointMazeVecEnv / AntMazeVecEnv(output="torch").step (Python, episode bookkeeping on the host) against
grx_env_step on a maze handle (the env-level C ABI, include/grx_env.h), alternating, three rounds each, in the default mode (both sides keep the time limit on the
host) and with continuing_task=False (the Python step reads the termination flags back every step, the handle decides them on the device).  Next-step autoreset, the
ids' own time limits, the same device actions on all paths.  Three paths: `python` (its step returns the flags on the host every step), `c_abi` (grx_env_step alone: a
caller that reads the flags later or not at all) and `c_abi+flags` (grx_env_step then grx_env_outputs every step: a rollout collector that needs terminated /
truncated of step t before it enqueues step t + 1 -- the like-for-like partner of `python`).

    python tools/bench_env_capi_maze.py [--env-ids PointMaze_Large-v3 AntMaze_Large_Diverse_GR-v5] [--worlds 8192] [--rounds 3] [--warmup 100] [--steps 1000]
                                        [--out profiles/ab_env_capi_maze.txt]

Per round: `warmup` untimed steps, then `steps` timed steps ending in a device synchronise.  Reported per path: env-steps/s (worlds x steps / wall time of the
timed window), host time per step call (perf_counter around the call alone) and the spread (max - min) across rounds."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-ids", nargs="+", default=["PointMaze_Large-v3", "AntMaze_Large_Diverse_GR-v5"])
    ap.add_argument("--worlds", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from gymnasium_robotics_amd import _native, env_capi as E
    from gymnasium_robotics_amd.envs.point_maze import AntMazeVecEnv, PointMazeVecEnv

    if not torch.cuda.is_available():
        raise SystemExit("bench_env_capi_maze: no HIP device")
    L = E.lib()
    n = args.worlds
    lines = [f"# tools/bench_env_capi_maze.py: {n} worlds, next_step autoreset, default time limits; {args.rounds} rounds x ({args.warmup} warm-up + {args.steps} timed steps) "
             f"per path, alternating; libgrx_hip build {_native.build_id()}"]
    tmpdir = tempfile.TemporaryDirectory()
    tmp = tmpdir.name
    for env_id in args.env_ids:
        cls = AntMazeVecEnv if env_id.startswith("AntMaze_") else PointMazeVecEnv
        for continuing in (True, False):
            env = cls(env_id, num_envs=n, device="cuda:0", output="torch", continuing_task=continuing)
            env.reset(seed=0)
            desc = E.write_env_desc(env_id, os.path.join(tmp, f"{env_id}_{int(continuing)}.grxenv"), continuing_task=continuing)
            h = ctypes.c_void_p()
            E.check(L.grx_env_create(desc.encode(), n, 0, None, ctypes.byref(h)))
            E.check(L.grx_env_reset(h, None, np.arange(n, dtype=np.uint64).ctypes.data, None))
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            gen = torch.Generator(device="cuda:0")
            gen.manual_seed(0)
            acts = [torch.rand(n, env.nu, device="cuda:0", generator=gen) * 2 - 1 for _ in range(16)]

            def py_step(a):
                env.step(a)

            def c_step(a):
                rc = L.grx_env_step(h, a.data_ptr(), stream)
                if rc:
                    E.check(rc)

            outs = E.EnvOutputs()

            def c_step_flags(a):
                c_step(a)
                rc = L.grx_env_outputs(h, ctypes.byref(outs))
                if rc:
                    E.check(rc)

            res = {"python": [], "c_abi": [], "c_abi+flags": []}
            for r in range(args.rounds):
                for name, fn in (("python", py_step), ("c_abi", c_step), ("c_abi+flags", c_step_flags)):
                    for k in range(args.warmup):
                        fn(acts[k % 16])
                    torch.cuda.synchronize()
                    host = 0.0
                    t0 = time.perf_counter()
                    for k in range(args.steps):
                        a = acts[k % 16]
                        c0 = time.perf_counter()
                        fn(a)
                        host += time.perf_counter() - c0
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                    res[name].append((n * args.steps / wall, 1e3 * host / args.steps))
                    print(f"{env_id} continuing_task={continuing} round {r} {name}: {n * args.steps / wall / 1e6:.4f} M env-steps/s, host {1e3 * host / args.steps:.4f} ms per step call", flush=True)
            E.check(L.grx_env_destroy(h))
            env.close()
            lines.append(f"{env_id}, continuing_task={continuing}")
            for name in ("python", "c_abi", "c_abi+flags"):
                rate = np.array([x[0] for x in res[name]]) / 1e6
                hst = np.array([x[1] for x in res[name]])
                lines.append(f"  {name:11s} env-steps/s median {np.median(rate):.4f} M (rounds {', '.join(f'{x:.4f}' for x in rate)}; spread {rate.max() - rate.min():.4f} M)  "
                             f"host per step call median {np.median(hst):.4f} ms (spread {hst.max() - hst.min():.4f} ms)")
            py = np.median([x[0] for x in res["python"]])
            for name in ("c_abi", "c_abi+flags"):
                cc = np.median([x[0] for x in res[name]])
                lines.append(f"  {name} / python = {cc / py:.4f}; difference {(cc - py) / 1e6:+.4f} M against a spread of {np.ptp([x[0] for x in res['python']]) / 1e6:.4f} M between the python rounds")
    tmpdir.cleanup()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
