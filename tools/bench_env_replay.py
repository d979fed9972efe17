"""A/B of the two ways a caller of the env-level C ABI can run the headline workload -- step + HER append + HER relabel -- in one process, alternating, three rounds each:

  python_her   grx_env_step on a handle with the Python HerReplay (gymnasium_robotics_amd/her.py) around it: what a caller had before grx_replay.h.  The replay needs the
               reset mask on the host and a world-indexed buffer of terminal rows, so every step reads the flags (grx_env_outputs: for a maze handle with device-side
               bookkeeping that waits for the flags copy), stages the mask and scatters the handle's compact final_rows.
  grx_replay   grx_env_step + grx_replay_append + grx_replay_relabel (include/grx_replay.h): nothing read back.

    python tools/bench_env_replay.py [--cases fetch:4096 fetch:8192 maze:8192] [--rounds 3] [--steps 500] [--drained 100] [--legs python_her grx_replay]
                                     [--out profiles/ab_env_replay.txt]

fetch:N = FetchPickAndPlace-v4, same-step autoreset, horizon 50, staggered (world i at phase 7 i mod 50); maze:N = AntMaze_Large_Diverse_GR-v5, continuing_task=False
(device bookkeeping), same-step, horizon 50.  Relabel batch 4 N per step, k_future 4, the finished episodes' last transitions kept: the shape of bench.py.  Each leg has
its own handle (same seeds, same device actions).  After one horizon of pre-roll on both: per round `steps` timed steps ending in a device synchronise (env-steps/s),
then `drained` steps with a device synchronise between the step call and the replay calls: the host time of the replay calls alone with the queue drained."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
HORIZON, K = 50, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["fetch:4096", "fetch:8192", "maze:8192"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--drained", type=int, default=100)
    ap.add_argument("--legs", nargs="+", default=["python_her", "grx_replay"], choices=["python_her", "grx_replay"], help="one leg alone: for a profiler run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from gymnasium_robotics_amd import _native, env_capi as E
    from gymnasium_robotics_amd.her import HerReplay

    if not torch.cuda.is_available():
        raise SystemExit("bench_env_replay: no HIP device")
    L = E.lib()
    lines = [f"# tools/bench_env_replay.py: same_step, horizon {HORIZON}, batch 4 N, k_future {K}, keep_final; one horizon of pre-roll, then {args.rounds} rounds x ({args.steps} timed + "
             f"{args.drained} drained steps) per leg, alternating; libgrx_hip build {_native.build_id()}"]
    tmp = tempfile.mkdtemp()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for case in args.cases:
        family, n = case.split(":")
        n = int(n)
        env_id, kw = ("FetchPickAndPlace-v4", {}) if family == "fetch" else ("AntMaze_Large_Diverse_GR-v5", {"continuing_task": False})
        desc = E.write_env_desc(env_id, os.path.join(tmp, f"{family}.grxenv"), **kw)
        cfg = E.EnvConfig(E.AUTORESET["same_step"], HORIZON, 0)
        phase = (np.arange(n) * 7) % HORIZON if family == "fetch" else np.zeros(n, np.int64)

        def make():
            h = ctypes.c_void_p()
            E.check(L.grx_env_create(desc.encode(), n, 0, ctypes.byref(cfg), ctypes.byref(h)))
            E.check(L.grx_env_reset(h, None, np.arange(n, dtype=np.uint64).ctypes.data, None))
            if phase.any():      # the elapsed section of a state blob: staggered episodes
                size = ctypes.c_size_t()
                E.check(L.grx_env_state_size(h, ctypes.byref(size)))
                blob = np.zeros(size.value, np.uint8)
                E.check(L.grx_env_get_state(h, blob.ctypes.data, blob.size))
                off = E.section_table(blob)[1]["elapsed"][0]
                blob[off: off + 8 * n] = np.frombuffer(phase.astype(np.int64).tobytes(), np.uint8)
                E.check(L.grx_env_set_state(h, blob.ctypes.data, blob.size))
            return h

        ha, hb = make(), make()
        od, gd, ad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        E.check(L.grx_env_dims(ha, ctypes.byref(od), ctypes.byref(gd), ctypes.byref(ad), None))
        od, gd, ad = od.value, gd.value, ad.value
        W, batch = od + 2 * gd + 2, 4 * n
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(0)
        acts = [torch.rand(n, ad, device="cuda:0", generator=gen) * 2 - 1 for _ in range(16)]

        # leg (a): HerReplay over the handle's device rows.  reward_spec() dispatches on the class name of the environment, so the handle is presented under that name.
        out = E.EnvOutputs()
        E.check(L.grx_env_outputs(ha, ctypes.byref(out)))
        shim = type("FetchVecEnv" if family == "fetch" else "AntMazeVecEnv", (), {})()
        shim.num_envs, shim.device, shim.packed = n, torch.device("cuda:0"), E.device_view(out.packed, (n, W))
        shim.single_action_space = type("Box", (), {"shape": (ad,)})()
        shim.reward_type = "sparse"
        shim.task = type("Task", (), {"distance_threshold": 0.05})()
        buf = HerReplay(shim, horizon=HORIZON, capacity=8 * batch, obs_dim=od, goal_dim=gd, seed=0, continuous=True)
        buf.begin_episode(shim.packed)
        buf.set_episode_start(-phase)
        term = torch.zeros(n, W, device="cuda:0")
        final_rows = E.device_view(out.final_rows, (n, W))
        idx_pin = [torch.empty(n, dtype=torch.int64, pin_memory=True) for _ in range(8)]
        idx_ev = [None] * 8
        idx_dev = torch.empty(n, dtype=torch.int64, device="cuda:0")
        slot = [0]

        def replay_a():
            E.check(L.grx_env_outputs(ha, ctypes.byref(out)))      # the flags of this step on the host
            k = out.n_final
            mask = np.zeros(n, bool)
            if k:
                idx = np.ctypeslib.as_array(ctypes.cast(out.final_idx, ctypes.POINTER(ctypes.c_int32)), (k,))
                mask[idx] = True
                s = slot[0] = (slot[0] + 1) % 8
                if idx_ev[s] is not None:
                    idx_ev[s].synchronize()
                idx_pin[s][:k] = torch.from_numpy(idx.astype(np.int64))
                idx_dev[:k].copy_(idx_pin[s][:k], non_blocking=True)
                idx_ev[s] = torch.cuda.Event()
                idx_ev[s].record()
                term.index_copy_(0, idx_dev[:k], final_rows[:k])
            buf.append(acts[0], shim.packed, mask, final_rows=term)      # (the action tensor's values do not matter to the timing)
            buf.relabel(batch, K)

        # leg (b)
        rcfg = E.ReplayConfig(horizon=HORIZON, keep_final=1, capacity=8 * batch, max_batch=batch, seed=0)
        rp = ctypes.c_void_p()
        E.check(L.grx_replay_create(hb, ctypes.byref(rcfg), ctypes.byref(rp)))
        E.check(L.grx_replay_begin(rp, stream))
        rb = E.ReplayBatch()

        def replay_b():
            rc = L.grx_replay_append(rp, stream) or L.grx_replay_relabel(rp, batch, K, ctypes.byref(rb), stream)
            if rc:
                E.check(rc)

        legs = [leg for leg in (("python_her", ha, replay_a), ("grx_replay", hb, replay_b)) if leg[0] in args.legs]

        def step(h, a):
            rc = L.grx_env_step(h, a.data_ptr(), stream)
            if rc:
                E.check(rc)

        for name, h, rep in legs:      # one horizon of pre-roll
            for k in range(HORIZON):
                step(h, acts[k % 16])
                rep()
        torch.cuda.synchronize()
        res = {name: [] for name, _, _ in legs}
        for r in range(args.rounds):
            for name, h, rep in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    step(h, acts[k % 16])
                    rep()
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                drained = 0.0
                for k in range(args.drained):
                    step(h, acts[k % 16])
                    torch.cuda.synchronize()
                    c0 = time.perf_counter()
                    rep()
                    drained += time.perf_counter() - c0
                torch.cuda.synchronize()
                res[name].append((n * args.steps / wall, 1e3 * drained / max(args.drained, 1)))
                print(f"{case} round {r} {name}: {n * args.steps / wall / 1e6:.4f} M env-steps/s, replay calls {res[name][-1][1]:.4f} ms per step with the queue drained", flush=True)
        valid = int(E.device_view(rb.valid, (1,), np.int32).item())
        E.check(L.grx_replay_destroy(rp))
        E.check(L.grx_env_destroy(ha))
        E.check(L.grx_env_destroy(hb))
        for name, _, _ in legs:
            rate = np.array([x[0] for x in res[name]]) / 1e6
            dr = np.array([x[1] for x in res[name]])
            lines.append(f"{case:11s} {name:10s} env-steps/s median {np.median(rate):.4f} M (rounds {', '.join(f'{x:.4f}' for x in rate)}; spread {rate.max() - rate.min():.4f} M)  "
                         f"replay calls, queue drained: median {np.median(dr):.4f} ms per step (rounds {', '.join(f'{x:.4f}' for x in dr)}; spread {dr.max() - dr.min():.4f} ms)")
        if len(legs) < 2:
            continue
        a, b = np.median([x[0] for x in res["python_her"]]), np.median([x[0] for x in res["grx_replay"]])
        spread = max(np.ptp([x[0] for x in res["python_her"]]), np.ptp([x[0] for x in res["grx_replay"]]))
        lines.append(f"{case:11s} grx_replay / python_her = {b / a:.4f}; difference {(b - a) / 1e6:+.4f} M against a round spread of {spread / 1e6:.4f} M; last batch valid = {valid}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
