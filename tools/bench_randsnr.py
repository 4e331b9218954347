"""Fused random-SNR observations + encoder features (qce_observe_randsnr, csrc/qce_observe_rows.hip) against the same
step composed from the functions the package had before it, on the reference training set's own shape
(Bussgang_VAE.py:41-44): B = 100 000 rows of N = 64, snrs -10 ... 20 dB in 5 dB steps, 3-bit uniform quantiser,
noise generated on the device; one line for P = 1 pilot and one for P = 2.

  fused     get_observation_nbit_randSNR(..., features="fft"): one launch, 16 bytes read + 8 written per complex value.
  composed  an index draw, rows grouped by SNR with index_select, one get_observation_nbit per SNR, index_copy back,
            torch.fft.fft, cat, .float().
  y         get_observation_nbit_randSNR(...) with the complex128 y as output (16 + 16 bytes), timed on its own.

The step is HBM-bound: the figure of merit is GB/s from the algorithmic bytes and its share of the 8 TB/s peak.
HIP events on torch's current stream (the stream every launch goes to), after a warm-up of every variant; the
repetitions are sized so that each timed window lasts at least 0.5 s; fused and composed alternate in one process
and the medians of the windows are compared.  Inputs are resident in HBM.  One JSON line per variant and a summary
line per P; --out also writes them to a file.  A missing GPU is an error."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantized_channel_estimation_amd import inputs, observe  # noqa: E402

HBM_PEAK = 8000.0  # GB/s, spec
SNRS = [-10, -5, 0, 5, 10, 15, 20]
N_BITS = 3


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn, min_s):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = window(fn, 5)
    return max(5, int(math.ceil(min_s * 1e3 / ms)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--antennas", type=int, default=64)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_randsnr.py needs a GPU: nothing is measured without one")
    B, N, S = args.rows, args.antennas, len(SNRS)
    quantizer = inputs.get_quantizer(SNRS, N_BITS, "uniform")
    g = torch.Generator(device="cuda").manual_seed(0)
    h = torch.randn((B, N), dtype=torch.complex128, device="cuda", generator=g)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for P in (1, 2):
        x = np.exp(1j * np.linspace(0, np.pi / 2, num=P, endpoint=False))
        A = None if P == 1 else np.kron(x[:, None], np.eye(N))
        M = P * N
        n_elem = B * M

        def fused():
            return observe.get_observation_nbit_randSNR(h, SNRS, A, N_BITS, quantizer, seed=1, features="fft")

        def fused_y():
            return observe.get_observation_nbit_randSNR(h, SNRS, A, N_BITS, quantizer, seed=1)

        def composed():
            idx = torch.randint(0, S, (B,), device=h.device)
            y = torch.empty((B, M), dtype=torch.complex128, device=h.device)
            for i, s in enumerate(SNRS):
                rows = (idx == i).nonzero().squeeze(1)
                ys = observe.get_observation_nbit(h.index_select(0, rows), s, A, N_BITS, quantizer[s][0],
                                                  quantizer[s][1], seed=1, offset=i * n_elem)
                y.index_copy_(0, rows, ys.reshape(-1, M))
            v = torch.fft.fft(y.reshape(B, P, N), dim=-1) / np.sqrt(N)
            return torch.cat([v.real, v.imag], dim=-1).float()

        variants = {"fused_features_fft": (fused, 24), "composed_parent_functions": (composed, 24)}
        reps = {k: reps_for(fn, args.min_window_s) for k, (fn, _) in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.windows):  # alternate the variants window by window
            for k, (fn, _) in variants.items():
                times[k].append(window(fn, reps[k]))
        med = {}
        for k, (fn, bpe) in variants.items():
            med[k] = float(np.median(times[k]))
            gbs = n_elem * bpe / (med[k] * 1e-3) / 1e9
            emit({"kernel": "k_observe_rows", "variant": k, "B": B, "N": N, "P": P, "snrs": S, "n_bits": N_BITS,
                  "ms_median": round(med[k], 4), "ms_windows": [round(t, 4) for t in times[k]], "reps": reps[k],
                  "algorithmic_bytes_per_element": bpe, "achieved_GBs": round(gbs, 1), "peak_GBs": HBM_PEAK,
                  "frac_of_hbm_peak": round(gbs / HBM_PEAK, 4), "bound": "HBM"})
        ry = reps_for(fused_y, args.min_window_s)
        ty = [window(fused_y, ry) for _ in range(3)]
        my = float(np.median(ty))
        gbs = n_elem * 32 / (my * 1e-3) / 1e9
        emit({"kernel": "k_observe_rows", "variant": "fused_y_output", "B": B, "N": N, "P": P, "snrs": S,
              "n_bits": N_BITS, "ms_median": round(my, 4), "ms_windows": [round(t, 4) for t in ty], "reps": ry,
              "algorithmic_bytes_per_element": 32, "achieved_GBs": round(gbs, 1), "peak_GBs": HBM_PEAK,
              "frac_of_hbm_peak": round(gbs / HBM_PEAK, 4), "bound": "HBM"})
        ratio = med["composed_parent_functions"] / med["fused_features_fft"]
        emit({"summary": f"P={P}", "fused_ms": round(med["fused_features_fft"], 4),
              "composed_ms": round(med["composed_parent_functions"], 4), "composed_over_fused": round(ratio, 2),
              "fused_not_slower": bool(ratio >= 1.0)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
