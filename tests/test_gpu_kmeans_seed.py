"""The device k-means++ seeding (qce_kmeans_seed, csrc/qce_kmeans_seed.hip) through the C ABI against sklearn's
kmeans_plusplus and the NumPy model of tests/kmeans_seed_ref.py, DeviceKMeans(seeding="device") against sklearn's
KMeans, and the fits' kmeans="device-seeded" against kmeans="host".

The margins of the parity cases (asserted in tests/test_kmeans_seed_ref.py: > 1e-9 relative, measured >= 5.6e-9 for
the search and >= 1.6e-6 for the argmin) are many orders over FP64 rounding, so indices and candidates are compared
exactly; on the exact cases (integer data) every sum is exact."""
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kmeans_ref as R
import kmeans_seed_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def km_mod():
    from quantized_channel_estimation_amd import _lib, kmeans
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    return kmeans


def _seed_host_io(X, K, first, U, mean_il):
    """qce_kmeans_seed with host buffers (QCE_IO_HOST) -> (centers, indices, cand, pot)."""
    from quantized_channel_estimation_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.complex128)
    B, N = X.shape
    T = U.shape[1] if K > 1 else 1
    centers, indices = np.empty((K, 2 * N)), np.empty(K, np.int64)
    cand, pot = np.empty((K - 1, T), np.int64), np.empty(K)
    _lib.check(_lib.load().qce_kmeans_seed(_lib.ptr(X), B, N, K, _lib.ptr(mean_il), int(first),
                                           _lib.ptr(np.ascontiguousarray(U)) if K > 1 else None, T, _lib.ptr(indices),
                                           _lib.ptr(centers), _lib.ptr(cand), _lib.ptr(pot), 0, _lib.IO_HOST, None))
    return centers, indices, cand, pot


def _centred_rows(e, idx):
    x = np.ascontiguousarray(e["Xz"]).view(np.float64)[idx]
    return x if e["mean_il"] is None else x - e["mean_il"]


@pytest.mark.parametrize("name", S.PARITY_NAMES + S.EXACT_NAMES)
def test_seeds_equal_model_and_sklearn(km_mod, name):
    e = S.expected(name)
    m = e["model"]
    centers, indices, cand, pot = km_mod.seed_device(e["Xz"], e["K"], e["first"], e["U"], x_mean=e["mean_il"],
                                                     want_debug=True)
    rel = np.abs(pot - m["pot"]) / np.where(m["pot"] > 0, m["pot"], 1.0)
    print(name, "mismatched indices", int((indices != e["sk_indices"]).sum()), "candidates",
          int((cand != m["cand"]).sum()), "pot rel", float(rel.max()))
    assert_array_equal(indices, e["sk_indices"])
    assert_array_equal(indices, m["indices"])
    assert_array_equal(cand, m["cand"])
    if name in S.EXACT_NAMES:
        assert_array_equal(pot, m["pot"])
    else:
        assert_allclose(pot, m["pot"], rtol=1e-12, atol=0)
    assert_array_equal(centers, _centred_rows(e, indices))


def test_host_io_equals_device_io_and_resident_input(km_mod):
    import torch
    e = S.expected("parity1")
    ref = km_mod.seed_device(e["Xz"], e["K"], e["first"], e["U"], x_mean=e["mean_il"], want_debug=True)
    host = _seed_host_io(e["Xz"], e["K"], e["first"], e["U"], e["mean_il"])
    Xd = torch.from_numpy(np.ascontiguousarray(e["Xz"])).cuda()
    keep = Xd.clone()
    res = km_mod.seed_device(Xd, e["K"], e["first"], e["U"], x_mean=e["mean_il"], want_debug=True)
    assert torch.equal(Xd, keep)  # used in place, left as it was
    for a, b, c in zip(ref, host, res):
        assert_array_equal(a, b)
        assert_array_equal(a, c)
    # without the debug outputs (NULL pointers)
    c2, i2 = km_mod.seed_device(Xd, e["K"], e["first"], e["U"], x_mean=e["mean_il"])
    assert_array_equal(c2, ref[0])
    assert_array_equal(i2, ref[1])


def test_two_runs_are_bit_identical(km_mod):
    e = S.expected("parity5")
    a = km_mod.seed_device(e["Xz"], e["K"], e["first"], e["U"], x_mean=e["mean_il"], want_debug=True)
    b = km_mod.seed_device(e["Xz"], e["K"], e["first"], e["U"], x_mean=e["mean_il"], want_debug=True)
    for x, y in zip(a, b):
        assert_array_equal(x, y)


def test_refusals(km_mod):
    z = lambda B, N: np.zeros((B, N), complex)  # noqa: E731
    u = lambda K, T=2: np.full((K - 1, T), 0.5)  # noqa: E731
    with pytest.raises(NotImplementedError, match="N <= 256"):
        km_mod.seed_device(z(8, 257), 2, 0, u(2))
    with pytest.raises(NotImplementedError, match="K <= 1024"):
        km_mod.seed_device(z(1100, 2), 1025, 0, u(1025))
    with pytest.raises(NotImplementedError, match="n_trials <= 16"):
        km_mod.seed_device(z(8, 2), 2, 0, u(2, 17))
    with pytest.raises(ValueError, match="n_samples=4 should be >= n_clusters=5"):
        km_mod.seed_device(z(4, 2), 5, 0, u(5))
    with pytest.raises(ValueError, match="first=8 is outside"):
        km_mod.seed_device(z(8, 2), 2, 8, u(2))
    bad = u(3)
    bad[1, 1] = 1.0
    with pytest.raises(ValueError, match=r"u must be in \[0, 1\)"):
        km_mod.seed_device(z(8, 2), 3, 0, bad)


@pytest.mark.parametrize("name", ["case1", "case2", "case5", "nonstrict0"])
def test_fit_with_device_seeding_equals_sklearn(km_mod, name):
    e = R.expected(name)
    rs = np.random.RandomState(e["seed"])
    km = km_mod.DeviceKMeans(e["K"], random_state=rs, seeding="device", **e["kw"]).fit(e["X"])
    ref = e["km"]
    assert_array_equal(km.labels_, ref.labels_)
    assert km.n_iter_ == ref.n_iter_
    assert_allclose(km.cluster_centers_, ref.cluster_centers_, rtol=0, atol=1e-12)
    assert_allclose(km.inertia_, ref.inertia_, rtol=1e-10, atol=0)
    rs2 = np.random.RandomState()
    rs2.set_state(e["rs_state"])
    assert_array_equal(rs.rand(4), rs2.rand(4))


# ---------------------------------------------------------------------------------------------------------------------
# through the fits: the same seeds give the same labels, hence identical kernels downstream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h_fit():
    return R.case(1037, 16, 5, 1.0, 21)


def _fit_quiet(g, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return g.fit(*args, **kw)


@pytest.mark.parametrize("ct,n_init", [("full", 2), ("circulant", 1)])
def test_gmm_nbit_fit_device_seeded_equals_host(km_mod, h_fit, ct, n_init):
    from quantized_channel_estimation_amd import Gmm_nbit
    fits = {}
    for opt in ("host", "device-seeded"):
        g = Gmm_nbit(n_components=5, covariance_type=ct, max_iter=5, n_init=n_init, random_state=3, kmeans=opt)
        fits[opt] = _fit_quiet(g, h_fit).gm
    for name in ("weights_", "means_", "covariances_", "n_iter_", "lower_bound_"):
        assert_array_equal(getattr(fits["device-seeded"], name), getattr(fits["host"], name), err_msg=name)


def test_gmm_quant_fit_device_seeded_equals_host(km_mod, h_fit, capsys):
    from quantized_channel_estimation_amd import Gmm_quant
    y = (np.sign(h_fit.real) + 1j * np.sign(h_fit.imag)) / np.sqrt(2)
    fits = {}
    for opt in ("host", "device-seeded"):
        g = Gmm_quant(n_components=5, covariance_type="full", max_iter=5, random_state=3, kmeans=opt)
        fits[opt] = _fit_quiet(g, h=y, n_bits=1, sigma2=0.1, quantizer=(None, None, None), quant_type="uniform")
    capsys.readouterr()  # the fit prints its lower bound per iteration
    for name in ("weights_", "means_", "covariances_", "n_iter_", "lower_bound_"):
        assert_array_equal(getattr(fits["device-seeded"].gm, name), getattr(fits["host"].gm, name), err_msg=name)
    assert_array_equal(fits["device-seeded"].covariances_quant, fits["host"].covariances_quant)


def test_mofa_initialize_device_seeded_equals_host(km_mod, h_fit):
    from quantized_channel_estimation_amd import Mofa
    out = {}
    for opt in ("host", "device-seeded"):
        np.random.seed(7)
        out[opt] = Mofa(5, 2, kmeans=opt, verbose=False)._initialize(h_fit)
    assert_allclose(out["device-seeded"][0], out["host"][0], rtol=0, atol=1e-12)  # means: the K-means centres
    for a, b in zip(out["device-seeded"][1:], out["host"][1:]):  # lambdas, psis, amps: the stream after the seeding
        assert_array_equal(a, b)
