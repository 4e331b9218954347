"""The covariance recovery of the quantised M-step on the host (NumPy, _em_quant.py) and on the device
(csrc/qce_quant_recover.hip through covrec.fit_variances / covrec.eig_clip) at the scripts' size: B = 100k, N = 64,
K = 64, 3-bit uniform data.  The two settings alternate in one process; the first round warms every path up and is
dropped; each figure is min / median / max of --reps runs.

Line "mstep": the recovery of one M-step, `_em_quant.quant_covariances` from the moments of a resident backend (the
moments pass itself is computed once and not timed), recovery="host" against recovery="device", with the parts of the
device setting alongside: the variance fits (one call for all K N), the eigenvalue clip (one call for all K), and what
stays on the host (the Bussgang gains from the prepare kernels, A Cy A^H with the quantised variances).  host_parts:
the variance fits and the clip of the host setting alone.  max_diff: the two settings' covariances compared.

Line "fit": a 10-iteration Gmm_quant.fit (tol = 0) end to end with both settings, kmeans="device" in both so that
the initialisation does not hide the M-steps, with the time spent inside the recovery (a host clock around
quant_covariances) and the rest of the fit per iteration.

beats_by_3_spreads: device median < host median - 3 (host spread + device spread), spread = max - min.
Lines go to stdout and to --out."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_channel_estimation_amd import Gmm_quant, _em_quant, covrec, inputs  # noqa: E402

SETTINGS = ("host", "device")


def make_data(B, N, n_bits, snr, seed=5):
    rng = np.random.default_rng(seed)
    hp, _ = inputs.scm_generate(4096, 1, N, rng, n_path=3)
    X = hp[rng.integers(0, 4096, size=B), 0, :].astype(np.complex128)
    thr, lab = inputs.uniform_quantizer(snr, n_bits)[:2]
    X = X + 10 ** (-snr / 20) * np.sqrt(0.5) * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    X = np.asarray(inputs.quant(X, n_bits, thr, lab), dtype=np.complex128)
    return np.ascontiguousarray(X), (np.asarray(thr), np.asarray(lab), None)


def spread(ts):
    return {"min": round(min(ts), 2), "median": round(statistics.median(ts), 2), "max": round(max(ts), 2)}


def beats(host, dev):
    noise = (max(host) - min(host)) + (max(dev) - min(dev))
    return bool(statistics.median(dev) < statistics.median(host) - 3 * noise)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_mstep(X, quantizer, K, n_bits, sigma2, reps):
    B, N = X.shape
    reg = 1e-6
    rng = np.random.default_rng(9)
    be = _em_quant.DeviceBackend(X, K, reg, True, n_bits, sigma2, quantizer, "uniform", 0)
    try:
        resp = be.kmeans_resp(X, K, np.random.RandomState(0))  # the responsibilities of a fit's first M-step
        nk, _, Q = be.mstep(resp)
        mom = be.moments(resp, None)
        thr = quantizer[0]
        x0 = np.real(np.einsum("kii->ki", Q)) + reg
        res = {s: [] for s in SETTINGS}
        parts = {"fits": [], "clip": [], "host_rest": [], "host_fits": [], "host_clip": []}
        covs, flagged, iters = {}, 0, None
        for r in range(reps + 1):
            for s in SETTINGS:
                np.random.seed(1)
                ms, (cov, _) = timed(lambda: _em_quant.quant_covariances(Q, nk, reg, n_bits, sigma2, quantizer,
                                                                         lambda: mom, be.gains, recovery=s))
                covs[s] = cov
                if r:
                    res[s].append(ms)
            ms_f, (s2, status, iters) = timed(lambda: covrec.variance_fits(mom[1], nk, thr, x0))
            ms_c, _ = timed(lambda: covrec.eig_clip(mom[0], reg, prep="sin-scaled", s2=s2, diag_pre=reg - sigma2,
                                                    diag_post=reg))
            ms_r, _ = timed(lambda: _em_quant._quantised_covariances(covs["device"], sigma2, quantizer, be.gains))
            flagged = int(status.sum())
            if r:
                parts["fits"].append(ms_f)
                parts["clip"].append(ms_c)
                parts["host_rest"].append(ms_r)
        # the host setting's two expensive pieces alone (once: they are the host figure above minus host_rest)
        thres = np.concatenate([_em_quant._positive_thresholds(thr)] * 2)
        ms_hf, _ = timed(lambda: [_em_quant.variance_fit(mom[1][k, d], nk[k], thres, x0[k, d])
                                  for k in range(K) for d in range(N)])
        ms_hc, _ = timed(lambda: [_em_quant._eig_clip(covs["host"][k], reg) for k in range(K)])
        diff = float(np.linalg.norm(covs["device"] - covs["host"]) / np.linalg.norm(covs["host"]))
    finally:
        be.close()
    return {"what": "mstep", "B": B, "N": N, "K": K, "n_bits": n_bits, "reps": reps,
            "threads": int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count()),
            "recovery_host_ms": spread(res["host"]), "recovery_device_ms": spread(res["device"]),
            "speedup": round(statistics.median(res["host"]) / statistics.median(res["device"]), 1),
            "beats_by_3_spreads": beats(res["host"], res["device"]),
            "device_parts_ms": {"variance_fits": spread(parts["fits"]), "eig_clip": spread(parts["clip"]),
                                "host_gains_and_assembly": spread(parts["host_rest"])},
            "host_parts_ms": {"variance_fits": round(ms_hf, 1), "eig_clip": round(ms_hc, 1)},
            "fits_flagged": flagged, "fit_steps": {"median": float(np.median(iters)), "max": int(iters.max())},
            "max_diff": diff}


def bench_fit(X, quantizer, K, n_bits, sigma2, reps, em_iter):
    clock = {"t": 0.0, "n": 0}
    orig = _em_quant.quant_covariances

    def wrapped(*a, **kw):
        t0 = time.perf_counter()
        out = orig(*a, **kw)
        clock["t"] += time.perf_counter() - t0
        clock["n"] += 1
        return out

    _em_quant.quant_covariances = wrapped
    res = {s: [] for s in SETTINGS}
    rec = {s: [] for s in SETTINGS}
    rest = {s: [] for s in SETTINGS}
    try:
        for r in range(reps + 1):
            for s in SETTINGS:
                clock["t"], clock["n"] = 0.0, 0
                g = Gmm_quant(n_components=K, covariance_type="full", max_iter=em_iter, tol=0.0, random_state=r,
                              kmeans="device", recovery=s)
                np.random.seed(r)
                with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
                    warnings.simplefilter("ignore")
                    ms, _ = timed(lambda: g.fit(h=X, n_bits=n_bits, sigma2=sigma2, quantizer=quantizer,
                                                quant_type="uniform", zero_mean=True))
                if r:
                    res[s].append(ms)
                    rec[s].append(clock["t"] * 1e3 / clock["n"])
                    rest[s].append((ms - clock["t"] * 1e3) / clock["n"])
    finally:
        _em_quant.quant_covariances = orig
    out = {"what": "fit", "B": X.shape[0], "N": X.shape[1], "K": K, "n_bits": n_bits, "em_max_iter": em_iter,
           "reps": reps, "kmeans": "device", "m_steps_per_fit": em_iter + 1}
    for s in SETTINGS:
        out[f"fit_{s}_ms"] = spread(res[s])
        out[f"recovery_ms_per_mstep_{s}"] = spread(rec[s])
        out[f"rest_of_fit_ms_per_mstep_{s}"] = spread(rest[s])
    out["speedup"] = round(statistics.median(res["host"]) / statistics.median(res["device"]), 1)
    out["beats_by_3_spreads"] = beats(res["host"], res["device"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--bits", type=int, default=3)
    ap.add_argument("--snr", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--em-iter", type=int, default=10)
    ap.add_argument("--no-fit", action="store_true", help="the M-step line only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_recover", "bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_quant_recover: no GPU visible")
    X, quantizer = make_data(a.B, a.N, a.bits, a.snr)
    sigma2 = 10 ** (-a.snr / 10)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        def emit(line):
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")
            fh.flush()

        emit(bench_mstep(X, quantizer, a.K, a.bits, sigma2, a.reps))
        if not a.no_fit:
            emit(bench_fit(X, quantizer, a.K, a.bits, sigma2, a.reps, a.em_iter))


if __name__ == "__main__":
    main()
