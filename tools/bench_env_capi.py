"""A/B of the two Fetch step paths in one process: FetchVecEnv(output="torch").step (Python launch group) against grx_env_step (the env-level
C ABI, include/grx_env.h), alternating, three rounds each.  FetchPickAndPlace-v4, same-step autoreset, staggered episodes (world i starts at
phase 7 i mod 50), the same device actions on both paths.

    python tools/bench_env_capi.py [--worlds 4096 8192] [--rounds 3] [--warmup 100] [--steps 1000] [--out profiles/ab_env_capi.txt]

Per round: `warmup` untimed steps, then `steps` timed steps ending in a device synchronise.  Reported per path: env-steps/s (worlds x steps / wall
time of the timed window), host time per step call (perf_counter around the call alone), and the spread (min - max) across rounds.  In the timed
window the GPU is the bottleneck, so the host time of a call there includes waiting for room in the launch queue; the host time per call with the
queue drained (a device synchronise before each of `--drained` more calls) is the enqueue cost itself."""
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
    ap.add_argument("--env-id", default="FetchPickAndPlace-v4")
    ap.add_argument("--worlds", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--drained", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from gymnasium_robotics_amd import _native, env_capi as E
    from gymnasium_robotics_amd.envs.fetch import FetchVecEnv

    if not torch.cuda.is_available():
        raise SystemExit("bench_env_capi: no HIP device")
    L = E.lib()
    lines = [f"# tools/bench_env_capi.py: {args.env_id}, same_step, horizon {args.horizon}, staggered; {args.rounds} rounds x ({args.warmup} warm-up + {args.steps} timed steps) "
             f"per path, alternating; libgrx_hip build {_native.build_id()}"]
    tmp = tempfile.mkdtemp()
    desc = E.write_env_desc(args.env_id, os.path.join(tmp, "env.grxenv"))
    for n in args.worlds:
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(0)
        acts = [torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1 for _ in range(16)]
        phase = (np.arange(n) * 7) % args.horizon

        env = FetchVecEnv(args.env_id, num_envs=n, device="cuda:0", autoreset_mode="same_step", max_episode_steps=args.horizon, output="torch")
        env.reset(seed=0)
        env._elapsed[:] = phase

        h = ctypes.c_void_p()
        cfg = E.EnvConfig(E.AUTORESET["same_step"], args.horizon, 0)
        E.check(L.grx_env_create(desc.encode(), n, 0, ctypes.byref(cfg), ctypes.byref(h)))
        E.check(L.grx_env_reset(h, None, (np.arange(n, dtype=np.uint64)).ctypes.data, None))
        size = ctypes.c_size_t()
        E.check(L.grx_env_state_size(h, ctypes.byref(size)))
        blob = np.zeros(size.value, np.uint8)
        E.check(L.grx_env_get_state(h, blob.ctypes.data, blob.size))
        off = E.section_table(blob)[1]["elapsed"][0]      # the elapsed section: the same staggered phases as the Python environment
        blob[off: off + 8 * n] = np.frombuffer(phase.astype(np.int64).tobytes(), np.uint8)
        E.check(L.grx_env_set_state(h, blob.ctypes.data, blob.size))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def py_step(a):
            env.step(a)

        def c_step(a):
            rc = L.grx_env_step(h, a.data_ptr(), stream)
            if rc:
                E.check(rc)

        res = {"python": [], "c_abi": []}
        for r in range(args.rounds):
            for name, fn in (("python", py_step), ("c_abi", c_step)):
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
                drained = 0.0
                for k in range(args.drained):
                    torch.cuda.synchronize()
                    c0 = time.perf_counter()
                    fn(acts[k % 16])
                    drained += time.perf_counter() - c0
                torch.cuda.synchronize()
                res[name].append((n * args.steps / wall, 1e3 * host / args.steps, 1e3 * drained / max(args.drained, 1)))
                print(f"n={n} round {r} {name}: {n * args.steps / wall / 1e6:.4f} M env-steps/s, host {1e3 * host / args.steps:.4f} ms per step call, "
                      f"{res[name][-1][2]:.4f} ms with the queue drained", flush=True)
        E.check(L.grx_env_destroy(h))
        env.close()
        for name in ("python", "c_abi"):
            rate = np.array([x[0] for x in res[name]]) / 1e6
            hst = np.array([x[1] for x in res[name]])
            dr = np.array([x[2] for x in res[name]])
            lines.append(f"n={n:5d} {name:7s} env-steps/s median {np.median(rate):.4f} M (rounds {', '.join(f'{x:.4f}' for x in rate)}; spread {rate.max() - rate.min():.4f} M)  "
                         f"host per step call median {np.median(hst):.4f} ms (spread {hst.max() - hst.min():.4f} ms), queue drained {np.median(dr):.4f} ms (spread {dr.max() - dr.min():.4f} ms)")
        py = np.median([x[0] for x in res["python"]])
        cc = np.median([x[0] for x in res["c_abi"]])
        spread = max(np.ptp([x[0] for x in res["python"]]), np.ptp([x[0] for x in res["c_abi"]]))
        lines.append(f"n={n:5d} c_abi / python = {cc / py:.4f}; difference {(cc - py) / 1e6:+.4f} M against a round spread of {spread / 1e6:.4f} M")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
