"""What the episode store (include/grx_episodes.h) costs and how fast its sampler runs, in one process:

  (a) step rate of grx_env_step + grx_replay_append + grx_replay_relabel on two handles, alternating, three rounds each after one horizon of pre-roll (the method of
      tools/bench_env_replay.py): `replay` has no store, `replay+store` has one of 65 536 episodes, so its append first archives the episodes each step ended.
  (b) device-event time of grx_episodes_sample alone at batch 4 N over the store the rounds of (a) have filled, and the bytes/s it achieves counted from the algorithmic
      bytes per sample, 4 (3 W + act_dim + OW): three gathered store rows, one action row, one output row.  A kernel rate, not a share of peak.

    python tools/bench_episode_replay.py [--worlds 4096 8192] [--rounds 3] [--steps 500] [--episodes 65536] [--legs replay replay+store] [--out profiles/ab_episode_replay.txt]

FetchPickAndPlace-v4, same-step autoreset, horizon 50, staggered (world i at phase 7 i mod 50), relabel batch 4 N, k_future 4, keep_final."""
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
    ap.add_argument("--worlds", nargs="+", type=int, default=[4096, 8192])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--episodes", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=30, help="timed grx_episodes_sample launches per strategy")
    ap.add_argument("--legs", nargs="+", default=["replay", "replay+store"], choices=["replay", "replay+store"], help="one leg alone: for a profiler run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from gymnasium_robotics_amd import _native, env_capi as E

    if not torch.cuda.is_available():
        raise SystemExit("bench_episode_replay: no HIP device")
    L = E.lib()
    lines = [f"# tools/bench_episode_replay.py: FetchPickAndPlace-v4, same_step, horizon {HORIZON}, staggered, relabel batch 4 N, k_future {K}, keep_final; store of {args.episodes} "
             f"episodes; one horizon of pre-roll, then {args.rounds} rounds x {args.steps} timed steps per leg, alternating; libgrx_hip build {_native.build_id()}"]
    tmp = tempfile.mkdtemp()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    desc = E.write_env_desc("FetchPickAndPlace-v4", os.path.join(tmp, "pick.grxenv"))
    for n in args.worlds:
        cfg = E.EnvConfig(E.AUTORESET["same_step"], HORIZON, 0)
        phase = (np.arange(n) * 7) % HORIZON
        batch = 4 * n

        def make(store):
            h = ctypes.c_void_p()
            E.check(L.grx_env_create(desc.encode(), n, 0, ctypes.byref(cfg), ctypes.byref(h)))
            E.check(L.grx_env_reset(h, None, np.arange(n, dtype=np.uint64).ctypes.data, None))
            size = ctypes.c_size_t()      # the elapsed section of a state blob: staggered episodes
            E.check(L.grx_env_state_size(h, ctypes.byref(size)))
            blob = np.zeros(size.value, np.uint8)
            E.check(L.grx_env_get_state(h, blob.ctypes.data, blob.size))
            off = E.section_table(blob)[1]["elapsed"][0]
            blob[off: off + 8 * n] = np.frombuffer(phase.astype(np.int64).tobytes(), np.uint8)
            E.check(L.grx_env_set_state(h, blob.ctypes.data, blob.size))
            rcfg = E.ReplayConfig(horizon=HORIZON, keep_final=1, capacity=8 * batch, max_batch=batch, seed=0)
            rp, st = ctypes.c_void_p(), ctypes.c_void_p()
            E.check(L.grx_replay_create(h, ctypes.byref(rcfg), ctypes.byref(rp)))
            if store:
                ecfg = E.EpisodesConfig(episodes=max(args.episodes, n), max_batch=batch, seed=0)
                E.check(L.grx_episodes_create(rp, ctypes.byref(ecfg), ctypes.byref(st)))
            E.check(L.grx_replay_begin(rp, stream))
            return h, rp, st

        legs = [(name, *make(name == "replay+store")) for name in args.legs]
        od, gd, ad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        E.check(L.grx_env_dims(legs[0][1], ctypes.byref(od), ctypes.byref(gd), ctypes.byref(ad), None))
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(0)
        acts = [torch.rand(n, ad.value, device="cuda:0", generator=gen) * 2 - 1 for _ in range(16)]
        rb = E.ReplayBatch()

        def group(h, rp, a):
            rc = L.grx_env_step(h, a.data_ptr(), stream) or L.grx_replay_append(rp, stream) or L.grx_replay_relabel(rp, batch, K, ctypes.byref(rb), stream)
            if rc:
                E.check(rc)

        for name, h, rp, st in legs:      # one horizon of pre-roll
            for k in range(HORIZON):
                group(h, rp, acts[k % 16])
        torch.cuda.synchronize()
        res = {name: [] for name, *_ in legs}
        for r in range(args.rounds):
            for name, h, rp, st in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    group(h, rp, acts[k % 16])
                torch.cuda.synchronize()
                res[name].append(n * args.steps / (time.perf_counter() - t0))
                print(f"N = {n} round {r} {name}: {res[name][-1] / 1e6:.4f} M env-steps/s", flush=True)
        for name, *_ in legs:
            rate = np.array(res[name]) / 1e6
            lines.append(f"N = {n:5d} {name:13s} env-steps/s median {np.median(rate):.4f} M (rounds {', '.join(f'{x:.4f}' for x in rate)}; spread {rate.max() - rate.min():.4f} M)")
        if len(legs) == 2:
            a, b = np.median(res["replay"]), np.median(res["replay+store"])
            spread = max(np.ptp(res["replay"]), np.ptp(res["replay+store"]))
            verdict = "within the round spread" if abs(b - a) <= spread else "MORE than the round spread: take a kernel trace of the replay+store leg in a run of its own"
            lines.append(f"N = {n:5d} replay+store / replay = {b / a:.4f}; difference {(b - a) / 1e6:+.4f} M against a round spread of {spread / 1e6:.4f} M: {verdict}")
        for name, h, rp, st in legs:      # (b): the sampler alone, over the store the rounds have filled
            if not st:
                continue
            ow, hz, w, adim = (ctypes.c_int() for _ in range(4))
            E.check(L.grx_episodes_dims(st, ctypes.byref(ow), ctypes.byref(hz), ctypes.byref(w), ctypes.byref(adim)))
            cnt, slots = ctypes.c_void_p(), ctypes.c_int64()
            E.check(L.grx_episodes_store(st, None, None, None, ctypes.byref(cnt), ctypes.byref(slots)))
            archived = int(E.device_view(cnt.value, (1,), np.int64).item())
            eb = E.EpisodesBatch()
            per_sample = 4 * (3 * w.value + adim.value + ow.value)
            for strategy, sname in enumerate(("future", "final", "episode")):
                ms = []
                for i in range(args.samples + 5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    E.check(L.grx_episodes_sample(st, batch, K, strategy, ctypes.byref(eb), stream))
                    e1.record()
                    e1.synchronize()
                    if i >= 5:
                        ms.append(e0.elapsed_time(e1))
                ms = np.array(ms)
                valid = int(E.device_view(eb.valid, (1,), np.int32).item())
                lines.append(f"N = {n:5d} grx_episodes_sample {sname:7s} batch {batch}: median {1e3 * np.median(ms):.1f} us (min {1e3 * ms.min():.1f}, max {1e3 * ms.max():.1f}; {len(ms)} launches, "
                             f"device events), {per_sample} algorithmic bytes per sample -> {batch * per_sample / (np.median(ms) * 1e-3) / 1e9:.1f} GB/s (kernel rate); "
                             f"{archived} episodes archived into {slots.value} slots, valid = {valid}")
        for name, h, rp, st in legs:
            if st:
                E.check(L.grx_episodes_destroy(st))
            E.check(L.grx_replay_destroy(rp))
            E.check(L.grx_env_destroy(h))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
