"""Throughput of the VAE-parameterised Bussgang LMMSE kernel (qce_vae_estimate, csrc/qce_vae.hip) and of the
route the package offered before it, BLMMSE.estimate_genie with one dense covariance per sample.

  python tools/vae_bench.py [--N 64] [--P 1] [--B 100000] [--steps 200] [--warmup 3] [--genie-B 100000]

One process, one timed loop per line.  Kernel lines: device tensors in and out, HIP events around every call on a
non-null stream (a call ends with the 4-byte status read, which is inside the window); est/s from the mean call,
bytes/s from the bytes an estimate has to move (16 P N for y, 4 N for float32 log-variances, 16 N for h).
Genie line: numpy in, numpy out, host clock around one call (it ends when h is in host memory); it builds, uploads
and factorises a dense N x N covariance per sample, which is the cost a user paid for per-sample covariances.
Prints one JSON line.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_line(N, P, B, n_bits, snr, steps, warmup, seed):
    import torch
    from quantized_channel_estimation_amd import lmmse_from_decoder
    rng = np.random.default_rng(seed)
    x = np.exp(1j * np.linspace(0, np.pi / 2, P, endpoint=False))
    A = np.kron(x[:, None], np.eye(N))
    lv = torch.as_tensor(rng.uniform(-2.5, 2.5, (B, N)).astype(np.float32), device="cuda")
    lev = np.array([-1.5, -0.5, 0.5, 1.5]) if n_bits != 1 else np.array([-1.0, 1.0]) / np.sqrt(2)
    y = rng.choice(lev, (B, P * N)) + 1j * rng.choice(lev, (B, P * N))
    y = torch.as_tensor(y, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(max(1, warmup)):
            h = lmmse_from_decoder(y, lv, snr, A, n_bits)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        t0 = time.perf_counter()
        for a, b in ev:
            a.record(stream)
            h = lmmse_from_decoder(y, lv, snr, A, n_bits)
            b.record(stream)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    nbytes = B * (16 * P * N + 4 * N + 16 * N)
    return dict(n_bits=n_bits, N=N, P=P, B=B, steps=steps, call_ms_mean=round(float(ms.mean()), 4),
                call_ms_median=round(float(np.median(ms)), 4), call_ms_min=round(float(ms.min()), 4),
                est_per_s=round(B / (ms.mean() * 1e-3), 1), bytes_per_s=round(nbytes / (ms.mean() * 1e-3), 1),
                wall_est_per_s=round(B * steps / wall, 1), finite=bool(torch.isfinite(torch.view_as_real(h)).all()))


def genie_line(N, B, n_bits, snr, seed):
    from quantized_channel_estimation_amd import lmmse_from_decoder
    from quantized_channel_estimation_amd.baselines import BLMMSE
    rng = np.random.default_rng(seed)
    lv = rng.uniform(-2.5, 2.5, (B, N)).astype(np.float32)
    y = (rng.choice([-1.0, 1.0], (B, N)) + 1j * rng.choice([-1.0, 1.0], (B, N))) / np.sqrt(2)
    # toeplitz(t)^T = F^H diag(c) F for t = conj(IDFT(c))
    t = np.conj(np.fft.ifft(np.maximum(np.exp(-lv.astype(np.float64)), 1e-12), axis=1))
    est = BLMMSE(snr)
    est.estimate_genie(y[:512], t[:512], None, n_bits)  # warm: code objects, allocator
    t0 = time.perf_counter()
    hg = est.estimate_genie(y, t, None, n_bits)
    dt = time.perf_counter() - t0
    hk = lmmse_from_decoder(y[:512], lv[:512], snr, None, n_bits)
    return dict(n_bits=n_bits, N=N, B=B, call_s=round(dt, 4), est_per_s=round(B / dt, 1),
                rel_diff_to_kernel=float(np.linalg.norm(hg[:512] - hk) / np.linalg.norm(hk)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--P", type=int, default=1)
    ap.add_argument("--B", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--genie-B", type=int, default=100000)
    ap.add_argument("--snr", type=float, default=5.0)
    a = ap.parse_args()
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        raise SystemExit("vae_bench: no GPU visible")
    res = {"kernel": [kernel_line(a.N, a.P, a.B, nb, a.snr, a.steps, a.warmup, 1) for nb in (1, 2)]}
    if a.genie_B > 0:
        res["genie"] = genie_line(a.N, a.genie_B, 1, a.snr, 2)
        res["kernel_over_genie_1bit"] = round(res["kernel"][0]["est_per_s"] / res["genie"]["est_per_s"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
