"""A/B of the Fourier-domain path with pilots (QCE_OPT_FOURIER_PILOTS, csrc/qce_fft_pilot_kernel.h) against the dense
families the same call takes without the option.  Per shape, on device-resident y at B = 10^5: one prepare plus one
'all' estimate per step, (a) option off and (b) option on, in one process on the same build and inputs.  HIP events
on the stream the calls are launched on, warm-up steps first, the mean and the spread over repeated steps.

Prints one JSON line per (shape, variant): the kernel family qce_model_kernel reports, ms per step, estimates per
second, h rel_fro of (b) against (a), and for (b) the achieved fraction of HBM for the 16 (P + 1) N B bytes an
estimate has to move.  --out FILE appends the lines to FILE; --off-only times (a) alone (e.g. under QCE_LIB=<another
build> to show that the option-off path is unchanged); PILOTS_B / PILOTS_REPS override the batch and the repeats."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantized_channel_estimation_amd import _lib, inputs  # noqa: E402

HBM_PEAK = 8000.0  # GB/s, MI355X

# name, K, N, blocks, P, n_bits, quantizer
SHAPES = [
    ("cfg3_P2_1bit", 128, 64, None, 2, 1, "uniform"),
    ("cfg3_P2_3bit_lloyd", 128, 64, None, 2, 3, "lloyd"),
    ("cfg3_P4_1bit", 128, 64, None, 4, 1, "uniform"),
    ("cfg3_P4_3bit_lloyd", 128, 64, None, 4, 3, "lloyd"),
    ("cfg5_P2_2bit", 128, 256, (4, 64), 2, 2, "uniform"),
]


def timed(step, stream, warmup, reps):
    """ms of each of `reps` steps (HIP events on `stream`), after `warmup` untimed ones."""
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            step()
        stream.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record(stream)
        for r in range(reps):
            step()
            ev[r + 1].record(stream)
        stream.synchronize()
    return [ev[r].elapsed_time(ev[r + 1]) for r in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    args = ap.parse_args()
    B = int(os.environ.get("PILOTS_B", 100_000))
    reps = int(os.environ.get("PILOTS_REPS", 5))
    snr = 5.0
    stream = torch.cuda.Stream()
    lines = []
    for name, K, N, blocks, P, n_bits, qtype in SHAPES:
        if args.shapes and name not in args.shapes.split(","):
            continue
        cov = "circulant" if blocks is None else "block-circulant"
        means, covs, w = inputs.synthetic_model(K, N, cov_type=cov, seed=K + N, blocks=blocks)
        A = inputs.get_pilot_matrix(N, P, n_bits)
        qz = inputs.get_quantizer([snr], n_bits, qtype)[snr]
        qkind = _lib.QUANT_LLOYD if (qtype == "lloyd" and n_bits != 1) else _lib.QUANT_UNIFORM
        # quantiser outputs as observations, drawn on the device: 1 bit +-1/sqrt(2), else labels
        g = torch.Generator(device="cuda").manual_seed(N + P)
        if n_bits == 1:
            lab = torch.tensor([-np.sqrt(0.5), np.sqrt(0.5)], dtype=torch.float64, device="cuda")
        else:
            lab = torch.tensor(qz[1], dtype=torch.float64, device="cuda")
        idx = torch.randint(0, lab.numel(), (2, B, P * N), device="cuda", generator=g)
        y = torch.complex(lab[idx[0]], lab[idx[1]]).contiguous()
        torch.cuda.synchronize()
        out = {}
        res = {}
        for variant in ("off",) if args.off_only else ("off", "on"):
            dm = _lib.DeviceModel(means, covs, w)
            if variant == "on":
                dm.set_fourier_pilots(True)
            h = torch.empty((B, N), dtype=torch.complex128, device="cuda")

            def step():
                dm.prepare(A, snr, float(n_bits), qkind, qz[0], qz[1], stream=stream.cuda_stream)
                dm.estimate(y, out=h, stream=stream.cuda_stream)

            ms = timed(step, stream, 2, reps)
            dm.synchronize()
            out[variant] = h.clone()
            res[variant] = dict(shape=name, variant=variant, K=K, N=N, P=P, n_bits=n_bits, quantizer=qtype, B=B,
                                kernel=dm.kernel(), ms=round(float(np.mean(ms)), 4),
                                ms_min=round(float(np.min(ms)), 4), ms_max=round(float(np.max(ms)), 4),
                                est_per_s=round(B / (float(np.mean(ms)) * 1e-3), 1), lib=os.path.basename(_lib.LIB_PATH))
            dm.close()
        if "on" in res:
            num = torch.linalg.norm(out["on"] - out["off"]).item()
            res["on"]["h_rel_fro_vs_off"] = num / torch.linalg.norm(out["off"]).item()
            gbs = 16.0 * (P + 1) * N * B / (res["on"]["ms"] * 1e-3) / 1e9
            res["on"].update(achieved_GBs=round(gbs, 1), peak_GBs=HBM_PEAK, hbm_frac=round(gbs / HBM_PEAK, 4),
                             speedup_vs_off=round(res["off"]["ms"] / res["on"]["ms"], 2))
        for variant in res:
            line = json.dumps(res[variant])
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
