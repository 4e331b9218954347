"""Random-SNR observations and fused VAE encoder features (reference utils.py:254-318
get_observation_nbit_randSNR*, estimators/vae.py:46-53 / :89-94; csrc/qce_observe_rows.hip through
qce_observe_randsnr).

CPU: the numpy restatement tests/randsnr_ref.py against tests/golden/randsnr.npz (made by make_golden_randsnr.py from
the reference itself, its draws replayed), and the argument checks observe.py makes before it touches the library.
GPU: bit-exact y for the reference's own draws (host and device I/O, kron pilot matrices against the dense route),
the features against the reference's float32 features, the shapes at which the kernel takes another path, and the
statistics / determinism / chunk invariance of the draws made on the device."""
import os

import numpy as np
import pytest

import randsnr_ref as R
from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "randsnr.npz")
F32_ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIX, allow_pickle=False))


def _case(d, tag):
    btag, atag, ptag = str(tag).split("_")
    nb = float(d[f"n_bits__{btag}"])
    A, p = d[f"A__{atag}"], d[f"p__{ptag}"]
    return dict(A=None if A.size == 0 else A, p=None if p.size == 0 else p, n_bits=np.inf if np.isinf(nb) else int(nb),
                thr=d.get(f"thr__{btag}"), lab=d.get(f"lab__{btag}"), idx=d[f"idx__{ptag}"], w=d[f"w__{atag}"],
                y=d[f"y__{tag}"], snr_list=d[f"snr_list__{tag}"], feat=d[f"feat__{tag}"])


def _quantizer(snrs, thr, lab):
    """The dict of inputs.get_quantizer from stacked tables."""
    if thr is None:
        return None
    return {s: (thr[i], lab[i], None) for i, s in enumerate(np.asarray(snrs).tolist())}


def _feature_bound(got, ref):
    """|got - ref| <= 2^-23 |ref| + 1e-13 max|row|: one float32 rounding of a value whose FP64 error is far below it,
    and bins that cancel to near zero.  Returns the worst ratio error / bound (<= 1 passes)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = F32_ULP * np.abs(ref) + 1e-13 * np.abs(ref).max(axis=-1, keepdims=True)
    err = np.abs(got - ref)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


# ----------------------------------------------------------------------------------------- CPU
def test_fixture_holds_every_case(fx):
    assert len(fx["tags"]) == 16
    for ptag in ("pu", "pw"):
        assert np.bincount(fx[f"idx__{ptag}"], minlength=4).min() >= 12


def test_restatement_reproduces_reference(fx):
    N = fx["h"].shape[1]
    for tag in fx["tags"]:
        c = _case(fx, tag)
        y, snr_list = R.observe(fx["h"], fx["snrs"], c["idx"], c["w"], c["A"], c["n_bits"], c["thr"], c["lab"])
        assert y.shape == c["y"].shape and np.array_equal(y, c["y"]), tag
        assert np.array_equal(snr_list, c["snr_list"]), tag
        f = R.features(y, N)
        assert f.dtype == np.float32 and f.shape == c["feat"].shape and np.array_equal(f, c["feat"]), tag
        assert _feature_bound(R.features_f64(y, N), c["feat"]) <= 1.0, tag


def test_argument_checks_need_no_gpu(fx):
    from quantized_channel_estimation_amd import observe
    f = observe.get_observation_nbit_randSNR
    h = np.zeros((4, 16), complex)
    snrs = [-10, 0, 5, 20]
    q2 = _quantizer(snrs, fx["thr__b2u"], fx["lab__b2u"])
    with pytest.raises(ValueError):
        f(h, [])
    with pytest.raises(ValueError):
        f(h, list(range(65)))
    with pytest.raises(ValueError):
        f(h, snrs, snr_scaling=[.5, .5])
    with pytest.raises(ValueError):
        f(h, snrs, snr_scaling=[.5, .7, -.1, -.1])
    with pytest.raises(ValueError):
        f(h, snrs, snr_scaling=[.1, .2, .3, .3])
    with pytest.raises(ValueError):
        f(h, snrs, None, 2, {s: q2[s] for s in snrs[:3]})
    with pytest.raises(ValueError):
        f(h, snrs, None, 2, None)
    q_mixed = dict(q2)
    q_mixed[20] = (fx["thr__b3l"][0], fx["lab__b3l"][0], None)
    with pytest.raises(ValueError):
        f(h, snrs, None, 2, q_mixed)
    with pytest.raises(ValueError):
        f(h, snrs, snr_index=np.array([0, 1, 2, 4]))
    with pytest.raises(ValueError):
        f(h, snrs, snr_index=np.array([0, -1, 2, 3]))
    with pytest.raises(ValueError):
        f(h, snrs, snr_index=np.array([0, 1, 2]))
    with pytest.raises(ValueError):
        f(h, snrs, noise=np.zeros((4, 15), complex))
    with pytest.raises(ValueError):
        f(h, snrs, np.zeros((32, 15), complex))
    with pytest.raises(ValueError):
        f(h, snrs, features="dft")
    with pytest.raises(NotImplementedError):
        f(h, snrs, np.zeros((24, 16), complex), features="fft")
    with pytest.raises(NotImplementedError):
        f(np.zeros((4, 48), complex), snrs, features="raw")
    with pytest.raises(NotImplementedError):
        observe.encoder_features(np.zeros((4, 40), complex), 16)
    with pytest.raises(NotImplementedError):
        observe.encoder_features(np.zeros((4, 96), complex), 48)


def test_exported_from_the_package():
    import quantized_channel_estimation_amd as pkg
    assert pkg.get_observation_nbit_randSNR is pkg.observe.get_observation_nbit_randSNR
    assert pkg.encoder_features is pkg.observe.encoder_features


# ----------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_gpu_fixture_supplied_draws_bit_exact(fx):
    import torch
    from quantized_channel_estimation_amd import observe
    h, snrs = fx["h"], fx["snrs"].tolist()
    ht = torch.from_numpy(h).cuda()
    for tag in fx["tags"]:
        c = _case(fx, tag)
        q = _quantizer(snrs, c["thr"], c["lab"])
        y, snr_list = observe.get_observation_nbit_randSNR(h, snrs, c["A"], c["n_bits"], q, c["p"],
                                                           snr_index=c["idx"], noise=c["w"])
        assert y.shape == c["y"].shape and y.dtype == np.complex128, tag
        assert np.array_equal(y, c["y"]), (tag, np.abs(y - c["y"]).max())
        assert snr_list.dtype == np.float64 and np.array_equal(snr_list, c["snr_list"]), tag
        yt, st = observe.get_observation_nbit_randSNR(ht, snrs, c["A"], c["n_bits"], q, c["p"],
                                                      snr_index=torch.from_numpy(c["idx"]).cuda(),
                                                      noise=torch.from_numpy(c["w"]).cuda())
        assert yt.is_cuda and st.is_cuda and st.dtype == torch.float64, tag
        assert np.array_equal(yt.cpu().numpy(), c["y"]) and np.array_equal(st.cpu().numpy(), c["snr_list"]), tag
        if c["A"] is not None:
            # the kron(x, I) route keeps one term of each row sum, rounded as numpy's matmul rounds it; the dense route
            # of qce_observe (cfma) fuses one product of each part into the sum: the same quantised y, and unquantised
            # values within the roundings of the products and sums (2^-53 each, relative to |x| |h| and |y|)
            for i, s in enumerate(snrs):
                rows = c["idx"] == i
                t = (None, None) if c["thr"] is None else (c["thr"][i], c["lab"][i])
                yd = observe.get_observation_nbit(h[rows], float(s), c["A"], c["n_bits"], t[0], t[1],
                                                  noise=c["w"][rows])
                if c["n_bits"] == np.inf:
                    tol = 2.0 ** -51 * (np.abs(h[rows]) @ np.abs(c["A"]).T + np.abs(yd))
                    assert np.all(np.abs(y[rows] - yd) <= tol), (tag, s)
                else:
                    assert np.array_equal(y[rows], yd), (tag, s)


@pytest.mark.gpu
def test_gpu_fixture_features(fx):
    import torch
    from quantized_channel_estimation_amd import observe
    h, snrs = fx["h"], fx["snrs"].tolist()
    N = h.shape[1]
    worst = 0.0
    for tag in fx["tags"]:
        c = _case(fx, tag)
        q = _quantizer(snrs, c["thr"], c["lab"])
        kw = dict(snr_index=c["idx"], noise=c["w"])
        f, snr_list = observe.get_observation_nbit_randSNR(h, snrs, c["A"], c["n_bits"], q, c["p"], features="fft", **kw)
        assert f.dtype == np.float32 and f.shape == c["feat"].shape, tag
        assert np.array_equal(snr_list, c["snr_list"]), tag
        r1 = _feature_bound(f, c["feat"])
        raw, _ = observe.get_observation_nbit_randSNR(h, snrs, c["A"], c["n_bits"], q, c["p"], features="raw", **kw)
        assert np.array_equal(raw, R.features(c["y"], N, fft_pre=False)), tag
        e = observe.encoder_features(c["y"], N)
        r2 = _feature_bound(e, c["feat"])
        assert np.array_equal(observe.encoder_features(c["y"], N, fft_pre=False), R.features(c["y"], N, False)), tag
        et = observe.encoder_features(torch.from_numpy(c["y"]).cuda(), N)
        assert et.is_cuda and et.dtype == torch.float32 and np.array_equal(et.cpu().numpy(), e), tag
        print(f"{tag}: features error / bound {r1:.3f}, encoder_features {r2:.3f}")
        worst = max(worst, r1, r2)
        assert r1 <= 1.0 and r2 <= 1.0, (tag, r1, r2)
    print("worst features error / bound:", worst)


def _tables(rng, S, L):
    """S increasing threshold rows (L - 1) and label rows (L), different for every SNR."""
    thr = np.sort(rng.standard_normal((S, L - 1)) * 1.5, axis=1)
    lab = np.sort(rng.standard_normal((S, L)) * 2.0, axis=1)
    return thr, lab


def _near(v, idx, n_bits, thr):
    """Elements of the unquantised v (B, M) within 1e-10 of a decision boundary of their row's quantiser."""
    if n_bits == 1:
        return (np.abs(v.real) < 1e-10) | (np.abs(v.imag) < 1e-10)
    t = thr[idx][:, None, :]  # (B, 1, L-1)
    return (np.abs(v.real[:, :, None] - t).min(-1) < 1e-10) | (np.abs(v.imag[:, :, None] - t).min(-1) < 1e-10)


SHAPES = {
    # name: (B, N, A kind, S, n_bits / levels)
    "n16_b37_ragged": (37, 16, None, 3, 8),
    "n256_b5": (5, 256, None, 3, 4),
    "n48_dense_m96": (257, 48, "dense96", 4, 8),
    "p3_n32": (70, 32, "kron3", 5, 1),
    "s1": (33, 64, None, 1, 4),
    "b1": (1, 32, "kron2", 3, 4),
    "s40_8bit_global_tables": (61, 16, None, 40, 256),
    "s3_8bit_lds_tables": (61, 16, None, 3, 256),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_gpu_shapes_vs_restatement(name):
    from quantized_channel_estimation_amd import observe
    B, N, akind, S, L = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    h = (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))) * np.sqrt(0.5)
    snrs = (np.arange(S) * 1.5 - 10.0).tolist()
    exact = True  # A h is exact in any summation order: identity, or pilots from {1, j, -1}
    if akind is None:
        A = None
    elif akind.startswith("kron"):
        A = np.kron(np.array([1, 1j, -1][:int(akind[4:])])[:, None], np.eye(N))
    else:
        M = int(akind[5:])
        A = rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))
        exact = False
    M = N if A is None else A.shape[0]
    idx = rng.integers(0, S, B).astype(np.int32)
    idx[:min(B, S)] = np.arange(min(B, S))  # every SNR that fits occurs
    w = (rng.standard_normal((B, M)) + 1j * rng.standard_normal((B, M))) * np.sqrt(0.5)
    if L == 1:
        n_bits, thr, lab, q = 1, None, None, None
    else:
        n_bits = int(np.log2(L))
        thr, lab = _tables(rng, S, L)
        q = _quantizer(snrs, thr, lab)
    v, _ = R.observe(h, snrs, idx, w, A, np.inf)
    yr, sr = R.observe(h, snrs, idx, w, A, n_bits, thr, lab)
    y, snr_list = observe.get_observation_nbit_randSNR(h, snrs, A, n_bits, q, snr_index=idx, noise=w)
    assert y.shape == (B, M) and snr_list.shape == (B,)
    assert np.array_equal(snr_list, sr)
    if exact:
        assert np.array_equal(y, yr)
    else:
        vg, _ = observe.get_observation_nbit_randSNR(h, snrs, A, np.inf, snr_index=idx, noise=w)
        assert np.abs(vg - v).max() <= 1e-12 * np.abs(v).max()
        near = _near(v, idx, n_bits, thr)
        assert near.mean() < 0.01
        assert np.array_equal(y[~near], yr[~near])
    if N in observe.FEATURE_ANTENNAS and exact:
        P = M // N
        f, _ = observe.get_observation_nbit_randSNR(h, snrs, A, n_bits, q, snr_index=idx, noise=w, features="fft")
        assert f.shape == (B, P, 2 * N) and f.dtype == np.float32
        assert _feature_bound(f, R.features(yr, N)) <= 1.0
        raw, _ = observe.get_observation_nbit_randSNR(h, snrs, A, n_bits, q, snr_index=idx, noise=w, features="raw")
        assert raw.shape == (B, P, 2 * N) and np.array_equal(raw, R.features(yr, N, fft_pre=False))


@pytest.fixture(scope="module")
def drawn():
    """Generated draws, B = 40 000 rows of N = 16 at h = 0, unquantised: uniform and weighted indices."""
    import torch
    from quantized_channel_estimation_amd import observe
    B, N = 40_000, 16
    snrs = [-10, 0, 5, 20]
    h = torch.zeros((B, N), dtype=torch.complex128, device="cuda")
    out = dict(B=B, N=N, snrs=snrs, h=h, p=[.1, .2, .3, .4])
    out["u"] = observe.get_observation_nbit_randSNR(h, snrs, None, np.inf, seed=77)
    out["w"] = observe.get_observation_nbit_randSNR(h, snrs, None, np.inf, snr_scaling=out["p"], seed=77)
    return out


@pytest.mark.gpu
def test_gpu_generated_index_and_noise_statistics(drawn):
    from scipy.stats import chi2
    B, N, snrs = drawn["B"], drawn["N"], np.asarray(drawn["snrs"], float)
    limit = chi2.isf(1e-9, 3)
    for key, p in (("u", np.full(4, .25)), ("w", np.asarray(drawn["p"]))):
        y, snr_list = drawn[key]
        y, snr_list = y.cpu().numpy(), snr_list.cpu().numpy()
        assert y.shape == (B, N) and snr_list.shape == (B,)
        counts = np.array([(snr_list == s).sum() for s in snrs])
        assert counts.sum() == B
        stat = float(((counts - B * p) ** 2 / (B * p)).sum())
        print(f"{key}: counts {counts}, chi2 {stat:.2f} (limit {limit:.2f})")
        assert stat < limit
        for s, n in zip(snrs, counts):
            scale = 10 ** (-s / 20)
            power = float((np.abs(y[snr_list == s]) ** 2).mean() / scale ** 2)
            print(f"{key}: snr {s}: mean |y|^2 / s^2 = {power:.5f} (n = {n})")
            assert abs(power - 1.0) < 6.0 / np.sqrt(n * N)


@pytest.mark.gpu
def test_gpu_generated_determinism_chunks_and_seed(drawn):
    import torch
    from quantized_channel_estimation_amd import observe
    h, snrs, p = drawn["h"], drawn["snrs"], drawn["p"]
    y, sl = drawn["w"]
    y2, sl2 = observe.get_observation_nbit_randSNR(h, snrs, None, np.inf, snr_scaling=p, seed=77)
    assert torch.equal(y, y2) and torch.equal(sl, sl2)
    B1 = 12_345
    yc, slc = observe.get_observation_nbit_randSNR(h[B1:], snrs, None, np.inf, snr_scaling=p, seed=77, row_offset=B1)
    assert torch.equal(yc, y[B1:]) and torch.equal(slc, sl[B1:])
    _, sl3 = observe.get_observation_nbit_randSNR(h[:1000], snrs, None, np.inf, snr_scaling=p, seed=78)
    assert not torch.equal(sl3, sl[:1000])


@pytest.mark.gpu
def test_gpu_single_snr_equals_get_observation_nbit(fx):
    from quantized_channel_estimation_amd import observe
    h = fx["h"]
    M = h.shape[1]
    snr = int(fx["snrs"][0])
    thr, lab = fx["thr__b3l"][0], fx["lab__b3l"][0]
    for n_bits, q, t in ((1, None, (None, None)), (3, {snr: (thr, lab, None)}, (thr, lab))):
        for off in (0, 7):
            y, sl = observe.get_observation_nbit_randSNR(h, [snr], None, n_bits, q, seed=5, row_offset=off)
            yo = observe.get_observation_nbit(h, snr, None, n_bits, t[0], t[1], seed=5, offset=off * M)
            assert np.array_equal(y, yo), (n_bits, off)
            assert np.array_equal(sl, np.full(h.shape[0], float(snr)))


@pytest.mark.gpu
def test_gpu_generated_features_and_quantiser_consistency(fx):
    import torch
    from quantized_channel_estimation_amd import observe
    snrs = fx["snrs"].tolist()
    rng = np.random.default_rng(12)
    B, N = 300, 32
    A = np.kron(np.array([1.0, 0.6 + 0.8j])[:, None], np.eye(N))
    h = torch.from_numpy((rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))) * np.sqrt(0.5)).cuda()
    thr, lab = fx["thr__b3l"], fx["lab__b3l"]
    q = _quantizer(snrs, thr, lab)
    kw = dict(snr_scaling=[.1, .2, .3, .4], seed=31, row_offset=3)
    v, sv = observe.get_observation_nbit_randSNR(h, snrs, A, np.inf, **kw)
    for n_bits, qq in ((3, q), (1, None)):
        y, sl = observe.get_observation_nbit_randSNR(h, snrs, A, n_bits, qq, **kw)
        f, sf = observe.get_observation_nbit_randSNR(h, snrs, A, n_bits, qq, features="fft", **kw)
        assert torch.equal(sl, sv) and torch.equal(sf, sv)
        # the fused features are the feature pass over the y of the same draws
        assert f.shape == (B, 2, 2 * N) and torch.equal(f, observe.encoder_features(y, N))
        # and y is quant() of the unquantised observation, one SNR group at a time
        for i, s in enumerate(snrs):
            rows = sv == float(s)
            assert int(rows.sum()) > 0
            t = (thr[i], lab[i]) if n_bits == 3 else (None, None)
            assert torch.equal(y[rows], observe.quant(v[rows], n_bits, t[0], t[1])), (n_bits, s)
