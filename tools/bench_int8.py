"""The int8-slice precision against the FP64 path on the metric workload (bench.py --config metric: K = 128,
N = M = 64, 1 bit, B = 100 000; observations and results resident in HBM, the prepare outside the timed window).

Four prepared models in one process -- precision 'f64' and 'int8' at S = 5, 7, 8 digit planes -- take turns window by
window (HIP events on the stream every launch goes to, each window at least --min-window-s long after a warm-up of
every model); the medians of the windows are compared and the spread (min, max) is kept.  Every int8 result is also
compared with the f64 result of the same process (relative Frobenius error over the whole batch).

Paper bound of an int8 line: the MACs the kernel issues, K B (2 MP + 2 NP) max(2 MP, 64) S, over the dense I8 rate:
v_mfma_i32_16x16x64_i8 is 16384 MACs in the cycles of the BF16 16x16x32 form (16 per SIMD), so 4096 MACs per clock
and CU, times --cus CUs at --clock-ghz (an assumed sustained clock: the number says so).  --parent-kernel-ms adds the
ratio to a kernel time of another build measured on the same card (bench.py's kernel_ms of the parent commit).

One JSON line per configuration; --out DIR also writes them to DIR/bench_int8.jsonl.  A missing GPU is an error."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from quantized_channel_estimation_amd import _lib  # noqa: E402

MACS_PER_CLK_CU = 4 * 16384 / 16  # four SIMDs, one 16x16x64 i8 MFMA per 16 cycles each


def window(fn, reps, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=0, help="override B")
    ap.add_argument("--components", type=int, default=0, help="override K")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--min-window-s", type=float, default=0.5)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--parent-kernel-ms", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_int8.py needs a GPU: nothing is measured without one")
    cfg = dict(bench.CONFIGS["metric"])
    if args.batch:
        cfg["B"] = args.batch
    if args.components:
        cfg["K"] = args.components
    K, N, B = cfg["K"], cfg["N"], cfg["B"]
    means, covs, w, _, y, _ = bench.make_inputs(cfg, 0)
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sptr = stream.cuda_stream

    configs = [("f64", None), ("int8", 5), ("int8", 7), ("int8", 8)]
    models, outs, fns = {}, {}, {}
    for prec, S in configs:
        name = prec if S is None else f"int8_S{S}"
        dm = _lib.DeviceModel(means, covs, w)
        if prec == "int8":
            dm.set_precision("int8", slices=S)
        dm.prepare(None, cfg["snr"], cfg["n_bits"], stream=sptr)
        out = torch.empty((B, N), dtype=torch.complex128, device=dev)
        models[name], outs[name] = dm, out
        fns[name] = (lambda dm=dm, out=out: dm.estimate(yd, _lib.MODE_ALL, 0.0, out=out, stream=sptr))
    reps = {}
    for name, fn in fns.items():  # warm-up, then size the windows
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(3, int(math.ceil(args.min_window_s * 1e3 / window(fn, 3, stream))))
    times = {name: [] for name in fns}
    for _ in range(args.windows):  # the configurations alternate window by window
        for name, fn in fns.items():
            times[name].append(window(fn, reps[name], stream))
    h64 = outs["f64"].cpu().numpy()
    MP = NP = next(p for p in (16, 32, 64) if N <= p)
    lines = []
    for (prec, S), name in zip(configs, fns):
        t = np.array(times[name])
        med = float(np.median(t))
        rec = {"tool": "bench_int8", "config": name, "kernel": models[name].kernel(), "K": K, "N": N, "B": B,
               "n_bits": cfg["n_bits"], "ms_median": round(med, 4), "ms_min": round(float(t.min()), 4),
               "ms_max": round(float(t.max()), 4), "spread_rel": round(float((t.max() - t.min()) / med), 4),
               "ms_windows": [round(float(x), 4) for x in t], "reps": reps[name],
               "estimates_per_s": round(B / (med * 1e-3), 1), "build_id": _lib.build_id()}
        if S is not None:
            macs = float(K) * B * (2 * MP + 2 * NP) * max(2 * MP, 64) * S
            bound_ms = macs / (MACS_PER_CLK_CU * args.cus * args.clock_ghz * 1e9) * 1e3
            h = outs[name].cpu().numpy()
            rec.update(slices=S, int8_macs=macs, paper_bound_ms=round(bound_ms, 4),
                       assumed_clock_ghz=args.clock_ghz, cus=args.cus,
                       frac_of_paper_bound=round(bound_ms / med, 4),
                       f64_over_int8_same_process=round(float(np.median(times["f64"])) / med, 3),
                       rel_fro_vs_f64=float(np.linalg.norm(h - h64) / np.linalg.norm(h64)))
        if args.parent_kernel_ms > 0:
            rec.update(parent_kernel_ms=args.parent_kernel_ms, parent_over_this=round(args.parent_kernel_ms / med, 3))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_int8.jsonl"), "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    for dm in models.values():
        dm.close()


if __name__ == "__main__":
    main()
