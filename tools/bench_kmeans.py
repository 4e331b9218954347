"""The K-means initialisation of the fits on the host (sklearn) and on the device (kmeans.DeviceKMeans ->
qce_kmeans_lloyd, csrc/qce_kmeans.hip) at the training scale B = 100k, N = 64 (D = 128 real columns), K in {64, 128}.

Per K, one JSON line "kmeans": sklearn's KMeans(n_init=1) on the real view (host clock, the process's thread limit),
the seeding alone (sklearn.cluster.kmeans_plusplus on the centred data), and the device Lloyd loop from the same seeds
on resident data (host clock around the synchronous C call: kernels, the per-iteration status read-back, the call's
scratch allocation), each repeated with min / median / max.  lloyd_ms_per_iter is the whole call over its iterations;
fixed_ms is a one-iteration call (allocation, two assignments, the inertia).  Shares of peak use the operations and
bytes the algorithm needs per iteration, 4 B K D flops on the FP64 MFMA and two reads of X, over that per-iteration
time -- a whole-call rate, not a kernel's.

Per K, one JSON line "seed": the k-means++ seeding alone, sklearn.cluster.kmeans_plusplus on the centred data against
kmeans.predraw + kmeans.seed_device (qce_kmeans_seed, csrc/qce_kmeans_seed.hip) on resident data, alternating, the
indices compared; step_us is the device call over its K - 1 steps (two launches each: pick + search, candidate pass),
pass_floor_us one read of X at the achievable HBM rate -- kernel times come from a kernel trace in a run of its own;
predraw_ms the pre-drawn random numbers alone, host_part_ms what DeviceKMeans._fit does on the host before the seeding
(real view, tolerance from the column variances, column mean, centring).

Per K and covariance type ('full', 'circulant'), one JSON line "fit": Gmm_nbit.fit end to end with kmeans="host",
kmeans="device" and kmeans="device-seeded", alternating, with the time spent in the EM steps (E-step + M-step, host
clock, both end synchronised) alongside.  Lines go to stdout and to --out."""
import argparse
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
from quantized_channel_estimation_amd import Gmm_nbit, _em, inputs, kmeans  # noqa: E402

FP64_PEAK = 78.6  # TFLOP/s, MI355X FP64 matrix (spec)
HBM_PEAK = 8.0    # TB/s (spec)
HBM_ACHIEVABLE = 6.3  # TB/s, a wide streaming copy
FIT_OPTIONS = ("host", "device", "device-seeded")


def make_data(B, N, seed=5):
    """Noisy draws from a pool of 3-path SCM channels (the training data of the scripts, scaled down in variety)."""
    rng = np.random.default_rng(seed)
    hp, _ = inputs.scm_generate(4096, 1, N, rng, n_path=3)
    X = hp[rng.integers(0, 4096, size=B), 0, :].astype(np.complex128)
    X += 0.1 * np.sqrt(0.5) * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return np.ascontiguousarray(X)


def spread(ts):
    return {"min": round(min(ts), 2), "median": round(statistics.median(ts), 2), "max": round(max(ts), 2)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench_kmeans(X, K, reps, max_iter):
    from sklearn.cluster import KMeans, kmeans_plusplus
    B, N = X.shape
    D = 2 * N
    Xr = np.concatenate([X.real, X.imag], axis=1)
    mean = Xr.mean(axis=0)
    tol_abs = 1e-4 * float(np.mean(np.var(Xr, axis=0)))
    Xc = Xr - mean
    host, host_it, seed_ms = [], [], []
    for r in range(reps):
        ms, km = timed(lambda: KMeans(n_clusters=K, n_init=1, max_iter=max_iter,
                                      random_state=np.random.RandomState(r)).fit(Xr))
        host.append(ms)
        host_it.append(int(km.n_iter_))
    seeds = []
    for r in range(reps):
        ms, (C0, _) = timed(lambda: kmeans_plusplus(Xc, K, random_state=np.random.RandomState(r)))
        seed_ms.append(ms)
        seeds.append(C0)
    Xd = torch.from_numpy(X).cuda()
    mean_il = kmeans.to_interleaved(mean)
    kmeans.lloyd_device(Xd, kmeans.to_interleaved(seeds[0]), tol_abs, 2, x_mean=mean_il)  # warm-up: code objects
    dev, dev_it, fixed = [], [], []
    for r in range(reps):
        C0 = kmeans.to_interleaved(seeds[r])
        ms, res = timed(lambda: kmeans.lloyd_device(Xd, C0, tol_abs, max_iter, x_mean=mean_il, want_resp=True))
        dev.append(ms)
        dev_it.append(res["n_iter"])
        fixed.append(timed(lambda: kmeans.lloyd_device(Xd, C0, tol_abs, 1, x_mean=mean_il))[0])
    per_iter = [t / n for t, n in zip(dev, dev_it)]
    t_it = statistics.median(per_iter) * 1e-3
    flops, nbytes = 4.0 * B * K * D, 2.0 * 8 * B * D
    return {"what": "kmeans", "B": B, "N": N, "K": K, "reps": reps, "threads": int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count()),
            "host_sklearn_ms": spread(host), "host_n_iter": host_it,
            "host_ms_per_iter": spread([t / n for t, n in zip(host, host_it)]),
            "seeding_ms": spread(seed_ms), "device_lloyd_ms": spread(dev), "device_n_iter": dev_it,
            "lloyd_ms_per_iter": spread(per_iter), "fixed_ms": spread(fixed),
            "iter_flops": flops, "iter_bytes": nbytes,
            "mfma_share_of_peak": round(flops / t_it / (FP64_PEAK * 1e12), 4),
            "hbm_share_of_peak": round(nbytes / t_it / (HBM_PEAK * 1e12), 4)}


def bench_seed(X, K, reps):
    """The seeding alone: host kmeans_plusplus against predraw + seed_device on resident data, alternating."""
    from sklearn.cluster import kmeans_plusplus
    B, N = X.shape
    Xr = np.concatenate([X.real, X.imag], axis=1)
    mean = Xr.mean(axis=0)
    Xc = Xr - mean
    Xd = torch.from_numpy(X).cuda()
    mean_il = kmeans.to_interleaved(mean)

    def device_seed(r):
        first, U = kmeans.predraw(np.random.RandomState(r), B, K)
        return kmeans.seed_device(Xd, K, first, U, x_mean=mean_il)[1]

    def host_part():  # what DeviceKMeans._fit does on the host before the seeding, on the host copy of X
        xr = np.concatenate([X.real, X.imag], axis=1).astype(np.float64, copy=False)
        tol = float(np.mean(np.var(xr, axis=0)) * 1e-4)
        m = xr.mean(axis=0)
        xr -= m
        return tol, kmeans.to_interleaved(m)

    device_seed(0)  # warm-up: code objects
    host, dev, pre, hp, same = [], [], [], [], True
    for r in range(reps):
        hp.append(timed(host_part)[0])
        ms, (_, idx) = timed(lambda: kmeans_plusplus(Xc, K, random_state=np.random.RandomState(r)))
        host.append(ms)
        ms, didx = timed(lambda: device_seed(r))
        dev.append(ms)
        pre.append(timed(lambda: kmeans.predraw(np.random.RandomState(r), B, K))[0])
        same = same and bool(np.array_equal(idx, didx))
    nbytes = 8.0 * B * 2 * N
    return {"what": "seed", "B": B, "N": N, "K": K, "reps": reps, "n_trials": 2 + int(np.log(K)),
            "host_seeding_ms": spread(host), "device_seeding_ms": spread(dev), "predraw_ms": spread(pre),
            "host_part_ms": spread(hp), "indices_equal": same, "launches_per_step": 2,
            "step_us": round(statistics.median(dev) * 1e3 / max(K - 1, 1), 2),
            "pass_bytes": nbytes, "pass_floor_us": round(nbytes / (HBM_ACHIEVABLE * 1e12) * 1e6, 2)}


def bench_fit(X, K, ct, reps, em_iter):
    """Gmm_nbit.fit with the three settings, alternating; EM time from a host clock around DeviceEM.estep / mstep."""
    clock = {"t": 0.0, "n": 0}
    estep, mstep = _em.DeviceEM.estep, _em.DeviceEM.mstep

    def wrap(fn, count):
        def inner(self, *a, **kw):
            t0 = time.perf_counter()
            out = fn(self, *a, **kw)
            clock["t"] += time.perf_counter() - t0
            clock["n"] += count
            return out
        return inner

    _em.DeviceEM.estep, _em.DeviceEM.mstep = wrap(estep, 1), wrap(mstep, 0)
    out = {"what": "fit", "B": X.shape[0], "N": X.shape[1], "K": K, "covariance_type": ct, "em_max_iter": em_iter,
           "reps": reps}
    try:
        res = {opt: [] for opt in FIT_OPTIONS}
        em = {opt: [] for opt in FIT_OPTIONS}
        for r in range(reps + 1):  # the first round warms every path up and is dropped
            for opt in FIT_OPTIONS:
                clock["t"], clock["n"] = 0.0, 0
                g = Gmm_nbit(n_components=K, covariance_type=ct, max_iter=em_iter, random_state=r, kmeans=opt)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ms, _ = timed(lambda: g.fit(X))
                if r:
                    res[opt].append(ms)
                    em[opt].append(clock["t"] * 1e3 / max(clock["n"], 1))
        for opt in FIT_OPTIONS:
            key = opt.replace("-", "_")
            out[f"fit_{key}_ms"] = spread(res[opt])
            out[f"em_ms_per_iter_{key}"] = spread(em[opt])
    finally:
        _em.DeviceEM.estep, _em.DeviceEM.mstep = estep, mstep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--K", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--em-iter", type=int, default=10)
    ap.add_argument("--no-fit", action="store_true", help="the K-means lines only (a kernel trace of the Lloyd loop)")
    ap.add_argument("--no-lloyd", action="store_true", help="skip the host KMeans / device Lloyd lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_seed", "bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_kmeans: no GPU visible")
    X = make_data(a.B, a.N)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        def emit(line):
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")
            fh.flush()

        for K in a.K:
            if not a.no_lloyd:
                emit(bench_kmeans(X, K, a.reps, a.max_iter))
            emit(bench_seed(X, K, a.reps))
            for ct in () if a.no_fit else ("full", "circulant"):
                emit(bench_fit(X, K, ct, a.reps, a.em_iter))


if __name__ == "__main__":
    main()
