"""What the normaliser's kernels cost beside a plain copy of the same bytes (her.Normalizer / grx_normstat_*, include/grx_capi.h).

    python tools/norm_probe.py [--out profiles/norm_probe.txt]

For Fetch dimensions (obs 25, goal 3, act 4: replay rows of 65 words) and batches of 16 384 and 1 048 576 rows, one process times three things with device events,
after a warm-up of every shape, in alternating rounds:
    update        grx_normstat_update: reads the batch once, writes a few KB (two launches)
    apply_batch   grx_normstat_apply_batch: reads the batch, writes a batch (one launch)
    copy          a device-to-device copy of the batch: the yardstick, reading and writing the same bytes as apply_batch
and reports the median time per call over the rounds, the spread, and the two ratios to the copy.  Needs a GPU; there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

OD, GD, AD = 25, 3, 4
BATCHES = ((16384, 5000), (1048576, 300))      # (rows, calls per timed window)
ROUNDS, WARMUP = 7, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_probe.txt"))
    args = ap.parse_args()
    import torch

    from gymnasium_robotics_amd import _native

    if not torch.cuda.is_available():
        raise SystemExit("norm_probe: no GPU visible; nothing is measured on a CPU")
    L = _native.lib()
    dev = "cuda:0"
    W = 2 * OD + 3 * GD + AD + 2
    lay = (ctypes.c_int64 * 8)()
    _native.check(L.grx_normstat_layout(OD, GD, lay))
    R, G = ctypes.c_int(), ctypes.c_int()
    L.grx_normstat_geometry(ctypes.byref(R), ctypes.byref(G))
    lines = [f"# tools/norm_probe.py on {torch.cuda.get_device_name(0)}; libgrx_hip.so build {_native.build_id()}",
             f"# Fetch dimensions: obs {OD}, goal {GD}, act {AD}, row width {W} words; update partition: {R.value} rows per chunk, at most {G.value} workgroups",
             f"# median us per call over {ROUNDS} alternating rounds (min .. max), device events, {WARMUP} warm-up calls of every shape; copy = Tensor.copy_ device to device",
             f"{'batch':>9} {'MB':>7} {'calls':>5}  {'update us':>24} {'apply_batch us':>24} {'copy us':>24}  {'update/copy':>11} {'apply/copy':>10}  {'copy GB/s':>9}"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for batch, calls in BATCHES:
        gen = torch.Generator(device=dev)
        gen.manual_seed(batch)
        rows = torch.randn(batch, W, device=dev, generator=gen)
        out = torch.empty_like(rows)
        block = torch.zeros(int(lay[7]), dtype=torch.uint8, device=dev)
        work = {
            "update": lambda: _native.check(L.grx_normstat_update(block.data_ptr(), rows.data_ptr(), batch, W, OD, GD, None, 1e-2, stream)),
            "apply": lambda: _native.check(L.grx_normstat_apply_batch(block.data_ptr(), rows.data_ptr(), batch, W, OD, GD, AD, 5.0, out.data_ptr(), stream)),
            "copy": lambda: out.copy_(rows),
        }
        for fn in work.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in work}
        for _ in range(ROUNDS):
            for k, fn in work.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / calls)
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = lambda k: f"{med[k]:9.2f} ({min(times[k]):.2f} .. {max(times[k]):.2f})"
        nbytes = batch * W * 4
        lines.append(f"{batch:>9} {nbytes / 1e6:>7.1f} {calls:>5}  {cell('update'):>24} {cell('apply'):>24} {cell('copy'):>24}  {med['update'] / med['copy']:>11.2f} "
                     f"{med['apply'] / med['copy']:>10.2f}  {2 * nbytes / med['copy'] / 1e3:>9.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
