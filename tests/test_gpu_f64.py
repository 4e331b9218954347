"""FP64 fused 'all'-mode kernel (qce_estimate_f64.hip) — the reference-precision default of
estimate_from_y (gmm_cplx_bussgang.py:220-228, every reference step complex128).

The bar here is FP64-class agreement with the FP64 oracle (1e-9 relative Frobenius: the remaining
difference is the Cholesky-vs-pinv filter of the prepare and summation order, cond(Cr) <= 1e3), far
below what an fp32 or fp16-split computation reaches (~1e-7), so a silent fall back to a narrower
kernel fails these tests.  The fp16-split fast path stays reachable with precision='fast'.
"""
import numpy as np
import pytest

from conftest import rel_fro

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9


def _gpu_or_skip():
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")


def _synthetic(K, N, B, seed, n_bits=1, snr=5.0, mean=False):
    from quantized_channel_estimation_amd import inputs
    means, covs, w = inputs.synthetic_model(K, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if mean:
        means = 0.3 * inputs.crandn(K, N, rng=rng)
    h, _ = inputs.scm_generate(B, 1, N, rng, n_path=3)
    h = h[:, 0, :].astype(complex)
    thr = lab = None
    if n_bits not in (1, np.inf):
        thr, lab, _ = inputs.uniform_quantizer(snr, n_bits)
    y = inputs.get_observation_nbit(h, snr, None, n_bits, thr, lab, rng=rng)
    return means, covs, w, h, y, (thr, lab, None)


@pytest.mark.parametrize("K,N,B,n_bits,mean", [
    (128, 64, 2048, 1, False),   # metric geometry
    (64, 64, 3000, 1, True),     # means: the -q0 / b mean blocks
    (33, 48, 1000, 2, True),     # padded N (48 -> 64), 2-bit uniform
    (16, 20, 257, np.inf, True),  # padded 20 -> 32, unquantised
    (5, 16, 100, 1, False),      # smallest padding, K < 8
    (40, 32, 700, 3, False),     # 3-bit uniform
])
def test_f64_all_mode_vs_oracle(K, N, B, n_bits, mean):
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit
    means, covs, w, h, y, qz = _synthetic(K, N, B, 300 + K, n_bits, mean=mean)
    g = Gmm_nbit.from_params(means, covs, w)
    hg = g.estimate_from_y(y, 5.0, N, None, "all", n_bits, "uniform", qz)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", n_bits, "uniform", qz)
    err = rel_fro(hg, ho)
    assert err < F64_TOL, err
    # MSE within 1e-9 (relative) of the reference computation
    mse_g = np.mean(np.abs(hg - h) ** 2)
    mse_o = np.mean(np.abs(ho - h) ** 2)
    assert abs(mse_g - mse_o) <= 1e-9 * mse_o


@pytest.mark.parametrize("wg", ["1", "3", "7", "100", "255", "5000"])
def test_f64_stream_k_cuts(wg, monkeypatch):
    """Persistent-grid schedule under different workgroup counts: whole tiles, cut tail tiles (merged
    by k_merge_f64), more workgroups than items."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit
    monkeypatch.setenv("QCE_WORKGROUPS", wg)
    K, N, B = 37, 64, 1500
    means, covs, w, h, y, qz = _synthetic(K, N, B, 41, 1, mean=True)
    g = Gmm_nbit.from_params(means, covs, w)
    hg = g.estimate_from_y(y, 5.0, N, None, "all", 1)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    assert rel_fro(hg, ho) < F64_TOL, rel_fro(hg, ho)


def test_f64_ragged_batches():
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit
    K, N = 20, 24
    means, covs, w, h, y, qz = _synthetic(K, N, 700, 33, 1)
    g = Gmm_nbit.from_params(means, covs, w)
    for B in (1, 2, 15, 16, 17, 127, 128, 129, 255, 700):
        hg = g.estimate_from_y(y[:B], 5.0, N, None, "all", 1)
        ho = O.estimate(means, covs, w, y[:B], 5.0, N, None, "all", 1)
        assert rel_fro(hg, ho) < F64_TOL, (B, rel_fro(hg, ho))


def test_f64_partials_combine():
    """FP64 K-shard partials (qce_estimate_partial_f64) combine to the full estimate at FP64 accuracy;
    the f32 entry point still returns the same partial rounded to f32."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import _lib
    from quantized_channel_estimation_amd.sharding import combine_partials_numpy
    K, N, B = 40, 64, 900
    means, covs, w, h, y, qz = _synthetic(K, N, B, 8, 1, mean=True)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    p64, p32 = [], []
    for lo, hi in [(0, 13), (13, 30), (30, 40)]:
        dm = _lib.DeviceModel(means[lo:hi], covs[lo:hi], w[lo:hi])
        dm.prepare(None, 5.0, 1.0)
        p64.append(dm.partial64(y))
        p32.append(dm.partial(y))
    assert rel_fro(combine_partials_numpy(p64, N), ho) < F64_TOL
    assert rel_fro(combine_partials_numpy(p32, N), ho) < 1e-6


def test_fast_precision_is_opt_in():
    """precision='fast' selects the fp16 two-term split kernel: still within the 1e-5 bar, but
    measurably less exact than the default FP64 kernel."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit
    K, N, B = 64, 64, 2000
    means, covs, w, h, y, qz = _synthetic(K, N, B, 12, 1)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    g = Gmm_nbit.from_params(means, covs, w)
    e64 = rel_fro(g.estimate_from_y(y, 5.0, N, None, "all", 1), ho)
    gf = Gmm_nbit.from_params(means, covs, w, precision="fast")
    efast = rel_fro(gf.estimate_from_y(y, 5.0, N, None, "all", 1), ho)
    assert e64 < F64_TOL
    assert efast < 1e-5
    assert efast > 10 * e64


def test_f64_device_io_matches_host():
    _gpu_or_skip()
    import torch
    from quantized_channel_estimation_amd import _lib
    K, N, B = 32, 64, 4096
    means, covs, w, h, y, qz = _synthetic(K, N, B, 3, 1)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, 5.0, 1.0)
    host = dm.estimate(y)
    out = dm.estimate(torch.from_numpy(y).to("cuda"))
    dm.synchronize()
    assert rel_fro(out.cpu().numpy(), host) == 0.0


@pytest.mark.parametrize("K,N,pilots,B,n_bits,mean", [
    (256, 128, 1, 512, 1, False),    # cfg4 geometry at its full K (the selective-mode limit K = 256)
    (24, 100, 1, 300, 2, True),      # padded N (100 -> 128), means
    (12, 64, 2, 400, 1, False),      # two pilots: M = 128 over N = 64
    (9, 128, 1, 200, np.inf, True),  # unquantised, means, N = 128
])
def test_f64_large_shapes_vs_oracle(K, N, pilots, B, n_bits, mean):
    """FP64 fused kernel at padded dimensions of 128 (one column tile per wave)."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit, inputs
    means, covs, w = inputs.synthetic_model(K, N, seed=K + N)
    rng = np.random.default_rng(K * N + 1)
    if mean:
        means = 0.3 * inputs.crandn(K, N, rng=rng)
    h, _ = inputs.scm_generate(B, 1, N, rng, n_path=3)
    h = h[:, 0, :].astype(complex)
    A = None if pilots == 1 else inputs.get_pilot_matrix(N, pilots, n_bits)
    qz = (None, None, None)
    if n_bits not in (1, np.inf):
        qz = inputs.uniform_quantizer(5.0, n_bits)
    y = inputs.get_observation_nbit(h, 5.0, A, n_bits, qz[0], qz[1], rng=rng)
    g = Gmm_nbit.from_params(means, covs, w)
    hg = g.estimate_from_y(y, 5.0, N, A, "all", n_bits, "uniform", qz)
    ho = O.estimate(means, covs, w, y, 5.0, N, A, "all", n_bits, "uniform", qz)
    # 1 bit with two pilots: the arcsine law's sensitivity at |rho| ~ 1 (test_gpu_parity.py) bounds the tables
    tol = 1e-7 if (pilots > 1 and n_bits == 1) else F64_TOL
    assert rel_fro(hg, ho) < tol, rel_fro(hg, ho)


@pytest.mark.parametrize("wg", ["1", "13", "300"])
def test_f64_n128_stream_k_and_partial(wg, monkeypatch):
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import _lib
    from quantized_channel_estimation_amd.sharding import combine_packed_numpy
    monkeypatch.setenv("QCE_WORKGROUPS", wg)
    K, N, B = 30, 128, 333
    means, covs, w, h, y, qz = _synthetic(K, N, B, 77, 1, mean=True)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, 5.0, 1.0)
    assert rel_fro(dm.estimate(y), ho) < F64_TOL
    parts = []
    shift = None
    models = []
    for lo, hi in [(0, 11), (11, 30)]:
        d = _lib.DeviceModel(means[lo:hi], covs[lo:hi], w[lo:hi])
        d.prepare(None, 5.0, 1.0)
        models.append(d)
    shift = max(float(np.max(d.cconst())) for d in models)
    parts = [d.partial_shifted(y, shift) for d in models]
    assert rel_fro(combine_packed_numpy(parts), ho) < F64_TOL


@pytest.mark.parametrize("K,N,pilots,B,n_bits,mean", [
    (128, 64, 1, 1024, 1, False),    # metric geometry
    (33, 48, 1, 700, 2, True),       # padded, means, 2-bit
    (64, 128, 1, 300, 1, False),     # N = 128
    (6, 64, 2, 300, 1, True),        # two pilots (M = 128)
    (5, 256, 1, 120, 1, False),      # N = 256
])
def test_f64_selective_modes_vs_oracle(K, N, pilots, B, n_bits, mean):
    """Modes 1 (argmax), top-n and cumulative-p in FP64: FP64 log-probabilities (exact labels), FP64
    selection weights and FP64 filters (k_est_sparse_f64) — the reference's complex128 arithmetic."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit, inputs
    means, covs, w = inputs.synthetic_model(K, N, seed=K + 2 * N)
    rng = np.random.default_rng(K + N + 5)
    if mean:
        means = 0.3 * inputs.crandn(K, N, rng=rng)
    h, _ = inputs.scm_generate(B, 1, N, rng, n_path=3)
    h = h[:, 0, :].astype(complex)
    A = None if pilots == 1 else inputs.get_pilot_matrix(N, pilots, n_bits)
    qz = (None, None, None)
    if n_bits not in (1, np.inf):
        qz = inputs.uniform_quantizer(5.0, n_bits)
    y = inputs.get_observation_nbit(h, 5.0, A, n_bits, qz[0], qz[1], rng=rng)
    g = Gmm_nbit.from_params(means, covs, w)
    tol = 1e-7 if (pilots > 1 and n_bits == 1) else F64_TOL
    for mode in (1, 3, 0.9, K + 5):
        hg = g.estimate_from_y(y, 5.0, N, A, mode, n_bits, "uniform", qz)
        ho = O.estimate(means, covs, w, y, 5.0, N, A, mode, n_bits, "uniform", qz)
        assert rel_fro(hg, ho) < tol, (mode, rel_fro(hg, ho))


@pytest.mark.parametrize("N,M_pilots,mean", [(64, 1, False), (64, 1, True), (48, 1, True), (32, 1, False),
                                             (16, 1, True), (20, 1, False), (32, 2, True), (16, 4, False),
                                             (128, 1, False), (128, 1, True), (100, 1, True), (72, 1, False)])
def test_f64_3m_matches_4m_and_oracle(N, M_pilots, mean, monkeypatch):
    """The 3M (Gauss) kernel k_est_all_f64g against the 4M kernel k_est_all_f64 (QCE_F64_3M=0 at prepare) and the FP64
    oracle: same FP64 computation up to rounding (1e-12 relative between the kernels, 1e-9 vs the oracle), for every
    padded shape it covers (M, N in {16, 32, 64}, square and with pilots M = 2N, 4N), with and without means, and the
    stream-K partial / K-shard packed outputs."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import _lib
    K, B = 24, 1500
    means, covs, w, h, _, _ = _synthetic(K, N, B, 500 + N, 1, mean=mean)
    rng = np.random.default_rng(N + M_pilots)
    M = N * M_pilots
    A = None if M_pilots == 1 else np.kron(np.exp(2j * np.pi * rng.random((M_pilots, 1))), np.eye(N)) / np.sqrt(M_pilots)
    y = (np.sign(rng.standard_normal((B, M))) + 1j * np.sign(rng.standard_normal((B, M)))) / np.sqrt(2)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(A, 5.0, 1.0)
    assert dm.kernel() == "f64_3m"
    h3 = dm.estimate(y)
    m3, s3, a3 = dm.partial64(y)
    monkeypatch.setenv("QCE_F64_3M", "0")
    dm.prepare(A, 5.0, 1.0)
    assert dm.kernel() == "f64_4m"
    h4 = dm.estimate(y)
    m4, s4, a4 = dm.partial64(y)
    assert rel_fro(h3, h4) < 1e-12, rel_fro(h3, h4)
    sc = np.exp(m3 - m4)  # the lazy running maxima may settle on different components
    assert rel_fro(a3 * sc[:, None], a4) < 1e-12 and rel_fro(s3 * sc, s4) < 1e-12
    Ao = np.eye(N) if A is None else A
    ho = O.estimate(means, covs, w, y, 5.0, N, Ao, "all", 1)
    tol = F64_TOL if M_pilots == 1 else 1e-6  # 1 bit with a general A: the arcsine law's documented sensitivity
    assert rel_fro(h3, ho) < tol, rel_fro(h3, ho)
    dm.close()


def test_reserved_cus_same_estimate():
    """QCE_OPT_RESERVE_CUS (the K-shard step's QCE_KSHARD_RESERVE_CUS, default 0 since round 6): the
    persistent grid shrinks, the estimate is the same FP64 computation (1e-12; the stream-K split differs)."""
    _gpu_or_skip()
    from quantized_channel_estimation_amd import _lib
    means, covs, w, h, y, qz = _synthetic(128, 64, 9000, 77, 1)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, 5.0, 1.0)
    h0 = dm.estimate(y)
    m0, s0, a0 = dm.partial64(y)
    for n in (16, 40, 250):
        dm.reserve_cus(n)
        assert rel_fro(dm.estimate(y), h0) < 1e-12
        m1, s1, a1 = dm.partial64(y)
        assert rel_fro(a1 * np.exp(m1 - m0)[:, None], a0) < 1e-12
    dm.close()


def test_snr_sweep_double_buffered_matches_serial():
    """sweep.SnrSweep (two table sets; the prepare of SNR point t+1 on its own stream beside the estimate of point t,
    Bussgang_GMM.py:284-287): every point equals the single-model prepare-then-estimate result (1e-12), over the
    reference's SNR list with one batch per point, 1 bit and 2-bit uniform."""
    _gpu_or_skip()
    import torch
    from quantized_channel_estimation_amd import _lib
    from quantized_channel_estimation_amd.sweep import SnrSweep
    for nb in (1, 2):
        means, covs, w, _, _, _ = _synthetic(32, 64, 10, 91, nb)
        pts, ys = [], []
        for i, snr in enumerate([-10, -5, 0, 5, 10, 15, 20]):
            _, _, _, _, y, _ = _synthetic(32, 64, 3000, 91 + i, nb, snr=float(snr))
            ys.append(y)
            pts.append((None, float(snr), nb, _lib.QUANT_UNIFORM, None, None, torch.from_numpy(y).cuda()))
        sw = SnrSweep(means, covs, w)
        outs = sw.run(pts)
        torch.cuda.synchronize()
        single = _lib.DeviceModel(means, covs, w)
        for (A, snr, _, _, _, _, _), y, h in zip(pts, ys, outs):
            single.prepare(None, snr, nb)
            assert rel_fro(h.cpu().numpy(), single.estimate(y)) < 1e-12, (nb, snr)
        sw.close()
        single.close()


def test_bench_sweep_line():
    """bench.py --sweep (the reference's SNR list, one batch per point, double-buffered tables) prints one JSON line
    whose points equal the serial loop and match the FP64 oracle."""
    _gpu_or_skip()
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg1", "--sweep", "--steps", "3",
                        "--warmup", "1", "--full"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["config"]["points"] == 7 and r["max_rel_dev_vs_serial"] < 1e-12
    assert r["parity"]["rel_fro"] < 1e-9 and r["ms_per_snr_point"] > 0


@pytest.mark.parametrize("mean", [False, True])
def test_f64h_whole_rounds_and_kshard_rows(mean, monkeypatch):
    """The padded-128 3M kernel k_est_all_f64h (row halves, y in LDS) with whole-tile rounds AND a stream-K tail
    (B = 40 000: 625 tiles of 64 over the persistent grid), and its shifted packed K-shard rows: equal to the 4M
    wave-pair kernel (QCE_F64_3M=0) within 1e-12, to the FP64 oracle within 1e-9 on 300 rows."""
    _gpu_or_skip()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import _lib
    K, N, B = 8, 128, 40000
    means, covs, w, h, y, _ = _synthetic(K, N, B, 913, 1, mean=mean)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, 5.0, 1.0)
    assert dm.kernel() == "f64_3m"
    h3 = dm.estimate(y)
    pk3 = dm.partial_shifted(y, dm.cconst_max())
    monkeypatch.setenv("QCE_F64_3M", "0")
    dm.prepare(None, 5.0, 1.0)
    assert dm.kernel() == "f64_4m"
    h4 = dm.estimate(y)
    pk4 = dm.partial_shifted(y, dm.cconst_max())
    assert rel_fro(h3, h4) < 1e-12, rel_fro(h3, h4)
    assert rel_fro(pk3, pk4) < 1e-12, rel_fro(pk3, pk4)
    ho = O.estimate(means, covs, w, y[:300], 5.0, N, None, "all", 1)
    assert rel_fro(h3[:300], ho) < F64_TOL
    dm.close()
