"""The moments pass of the quantised fit (DeviceBackend.moments -> covrec.quant_moments -> qce_quant_moments) at the
training scale B = 100k, D = 64, K = 16, 3-bit uniform data: once for a zero-mean model (d = x) and once for a model
with means (d = x - mu_k), next to the FP64 MFMA roofline of the sign correlation (8 K B N^2 flops) and the bytes the
indicator pass moves (X once per block of 8 components, R once).

moments_ms: a host clock around DeviceBackend.moments(), which ends with the results on the host (synchronised).
device_ms: HIP events around covrec.quant_moments with resident inputs and outputs (the four kernels and the scratch
allocation of the call).  held_MB: torch.cuda.memory_allocated() with the backend alive (X, R and the M-step's
outputs); used_MB: the drop of the driver's free memory from before the backend was made to after the calls (adds
the runtime's own pools; the call's scratch is freed when it returns).  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_channel_estimation_amd import _em_quant, covrec, inputs  # noqa: E402

FP64_PEAK = 78.6  # TFLOP/s, MI355X FP64 matrix (spec)
HBM_PEAK = 8.0    # TB/s (spec)


def make_data(B, N, K, n_bits, snr, seed=5):
    rng = np.random.default_rng(seed)
    hp, _ = inputs.scm_generate(4096, 1, N, rng, n_path=3)
    X = hp[rng.integers(0, 4096, size=B), 0, :].astype(np.complex128)
    thr, lab = inputs.uniform_quantizer(snr, n_bits)[:2]
    X = X + 10 ** (-snr / 20) * np.sqrt(0.5) * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    X = np.asarray(inputs.quant(X, n_bits, thr, lab), dtype=np.complex128)
    R = rng.random((B, K))
    R /= R.sum(axis=1, keepdims=True)
    mu = 0.3 * np.sqrt(0.5) * (rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    return np.ascontiguousarray(X), R, mu, (np.asarray(thr), np.asarray(lab), None)


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(backend_cls=None, B=None, reps=None):
    """backend_cls: a DeviceBackend-compatible class (default: the package's)."""
    backend_cls = backend_cls or _em_quant.DeviceBackend
    N, K, n_bits, snr = 64, 16, 3, 10.0
    B = B or int(os.environ.get("COVREC_B", 100_000))
    reps = reps or int(os.environ.get("COVREC_REPS", 5))
    X, R, mu, quantizer = make_data(B, N, K, n_bits, snr)
    T = 2 ** (n_bits - 1) - 1
    flops = 8.0 * K * B * N * N
    bytes_ind = 16.0 * B * N * ((K + 7) // 8) + 8.0 * B * K
    out = {"workload": f"quantised-fit moments B={B} D={N} K={K} {n_bits}-bit uniform (T={T})",
           "corr_flops": flops, "indicator_bytes": bytes_ind, "fp64_peak_tflops": FP64_PEAK, "hbm_peak_TBps": HBM_PEAK}
    for name, zero_mean in (("zero_mean", True), ("with_means", False)):
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        be = backend_cls(X, K, 1e-6, zero_mean, n_bits, 10 ** (-snr / 10), quantizer, "uniform", 0)
        be.em.R.copy_(torch.from_numpy(R))
        torch.cuda.synchronize()
        setup_ms = (time.perf_counter() - t0) * 1e3
        held = torch.cuda.memory_allocated()
        means = None if zero_mean else mu
        low = [free0]

        def call():
            res = be.moments(None, means)
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            return res

        ms = wall(call, reps if zero_mean else max(1, reps // 2))
        rec = {"setup_ms": round(setup_ms, 1), "moments_ms": round(ms, 3), "held_MB": round(held / 1e6, 1),
               "used_MB": round((free0 - low[0]) / 1e6, 1)}
        if backend_cls is _em_quant.DeviceBackend:
            mud = None if zero_mean else torch.from_numpy(mu).cuda()
            thr = quantizer[0]
            dms = events(lambda: covrec.quant_moments(be.em.X, be.em.R, mud, thr, out="device"), reps)
            rec["device_ms"] = round(dms, 3)
            rec["corr_tflops_over_whole_call"] = round(flops / (dms * 1e-3) / 1e12, 2)
        be.close()
        del be
        torch.cuda.empty_cache()
        out[name] = rec
    return out


if __name__ == "__main__":
    print(json.dumps(run()), flush=True)
