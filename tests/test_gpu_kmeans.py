"""The device Lloyd loop (qce_kmeans_lloyd, csrc/qce_kmeans.hip) against sklearn's KMeans and the NumPy reference of
tests/kmeans_ref.py, and the fits' kmeans="device" against kmeans="host".

The reference margins of the cases (asserted in tests/test_kmeans_ref.py: > 1e-9 relative, measured >= 2.4e-6) are
many orders over FP64 rounding, so labels and iteration counts are compared exactly."""
import ctypes
import warnings

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kmeans_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def km_mod():
    from quantized_channel_estimation_amd import _lib, kmeans
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    return kmeans


def _fit(km_mod, e, X=None, **kw):
    init = {} if e["init"] is None else {"init": e["init"]}
    km = km_mod.DeviceKMeans(e["K"], random_state=np.random.RandomState(e["seed"]), **init, **e["kw"])
    return km._fit(e["X"] if X is None else X, **kw)


@pytest.mark.parametrize("name", R.ALL_NAMES)
def test_fit_equals_sklearn(km_mod, name):
    e = R.expected(name)
    km, ref = _fit(km_mod, e), e["km"]
    print(name, "mismatched labels", int((km.labels_ != ref.labels_).sum()), "n_iter", km.n_iter_, ref.n_iter_,
          "centres", float(np.abs(km.cluster_centers_ - ref.cluster_centers_).max()),
          "inertia rel", abs(km.inertia_ - ref.inertia_) / max(ref.inertia_, 1e-300))
    assert_array_equal(km.labels_, ref.labels_)
    assert km.n_iter_ == ref.n_iter_
    assert_allclose(km.cluster_centers_, ref.cluster_centers_, rtol=0, atol=1e-12)
    assert_allclose(km.inertia_, ref.inertia_, rtol=1e-10, atol=0)


def test_exact_ties_single_step(km_mod):
    """Integer data make every summation order exact: the step pins the lowest-index rule and the f64 lane map."""
    X, C = R.tie_case()
    labels1, margins1, _ = R.assign(X, C)
    assert int((margins1 == 0).sum()) == 124 and not np.any(labels1 == 3)
    labels, Cref, inertia, n_iter, info = R.lloyd_ref(X, C, 0.0, 1)
    assert info["relocated"] == 1  # cluster 3 got no row in the step
    # the closing assignment is against centres that are no integers any more: it must not be a close call
    assert R.assign(X, Cref)[1].min() > 1e-9
    Xz = np.ascontiguousarray(X).view(np.complex128)  # columns as stored: (re0, im0, re1, ...)
    r = km_mod.lloyd_device(Xz, C, 0.0, 1)
    assert_array_equal(r["labels"], labels)
    assert_array_equal(r["centers"], Cref)
    assert (r["n_iter"], r["strict"], r["relocated"]) == (1, False, 1)
    assert_allclose(r["inertia"], inertia, rtol=1e-12, atol=0)


def test_resp_out_and_device_input(km_mod):
    import torch
    e = R.expected("case1")
    km = _fit(km_mod, e, want_resp=True)
    resp = km.resp_.cpu().numpy()
    host = np.zeros((e["X"].shape[0], e["K"]))
    host[np.arange(host.shape[0]), km.labels_] = 1
    assert_array_equal(resp, host)
    assert_array_equal(resp.argmax(axis=1), km.labels_)
    assert_array_equal(resp.sum(axis=1), np.ones(host.shape[0]))
    Xd = torch.from_numpy(e["X"]).cuda()
    kd = _fit(km_mod, e, X=Xd, want_resp=True)
    assert_array_equal(kd.labels_, km.labels_)
    assert_array_equal(kd.cluster_centers_, km.cluster_centers_)
    assert kd.inertia_ == km.inertia_ and kd.n_iter_ == km.n_iter_
    assert torch.equal(kd.resp_, km.resp_)


def test_host_io_equals_device_io(km_mod):
    """The C call with host buffers (QCE_IO_HOST) against the tensor path."""
    from quantized_channel_estimation_amd import _lib
    e = R.expected("case0")
    X, K = np.ascontiguousarray(e["X"]), e["K"]
    B, N = X.shape
    _, Xc, mean = R.centred(X)
    C0 = km_mod.to_interleaved(Xc[:K])
    mean_il = km_mod.to_interleaved(mean)
    r = km_mod.lloyd_device(X, C0, 1e-3, 300, x_mean=mean_il, want_resp=True)
    centers, labels, resp, info = np.empty((K, 2 * N)), np.empty(B, np.int64), np.empty((B, K)), np.empty(4)
    _lib.check(_lib.load().qce_kmeans_lloyd(_lib.ptr(X), B, N, K, _lib.ptr(mean_il), _lib.ptr(C0), 300, 1e-3,
                                            _lib.ptr(centers), _lib.ptr(labels), _lib.ptr(resp), _lib.ptr(info), 0,
                                            _lib.IO_HOST, None))
    assert_array_equal(labels, r["labels"])
    assert_array_equal(centers, r["centers"])
    assert_array_equal(resp, r["resp"].cpu().numpy())
    assert (int(info[0]), info[1], bool(info[2])) == (r["n_iter"], r["inertia"], r["strict"])


def test_two_runs_are_bit_identical(km_mod):
    e = R.expected("case5")
    a, b = _fit(km_mod, e), _fit(km_mod, e)
    assert_array_equal(a.cluster_centers_, b.cluster_centers_)
    assert a.inertia_ == b.inertia_
    assert_array_equal(a.labels_, b.labels_)


def test_refusals(km_mod):
    z = lambda B, N: np.zeros((B, N), complex)  # noqa: E731
    with pytest.raises(NotImplementedError, match="N <= 256"):
        km_mod.lloyd_device(z(8, 257), np.zeros((2, 514)), 0.0, 1)
    with pytest.raises(NotImplementedError, match="K <= 1024"):
        km_mod.lloyd_device(z(1100, 2), np.zeros((1025, 4)), 0.0, 1)
    with pytest.raises(ValueError, match="n_samples=4 should be >= n_clusters=5"):
        km_mod.lloyd_device(z(4, 2), np.zeros((5, 4)), 0.0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# through the fits: identical labels give an identical one-hot R, hence identical kernels downstream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h_fit():
    return R.case(1037, 16, 5, 1.0, 21)


def _fit_quiet(g, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return g.fit(*args, **kw)


@pytest.mark.parametrize("ct,n_init", [("full", 2), ("circulant", 1), ("toeplitz", 1)])
def test_gmm_nbit_fit_device_equals_host(km_mod, h_fit, ct, n_init):
    from quantized_channel_estimation_amd import Gmm_nbit
    fits = {}
    for opt in ("host", "device"):
        g = Gmm_nbit(n_components=5, covariance_type=ct, max_iter=5, n_init=n_init, random_state=3, kmeans=opt)
        fits[opt] = _fit_quiet(g, h_fit).gm
    for name in ("weights_", "means_", "covariances_", "n_iter_", "lower_bound_"):
        assert_array_equal(getattr(fits["device"], name), getattr(fits["host"], name), err_msg=name)


def test_gmm_quant_fit_device_equals_host(km_mod, h_fit, capsys):
    from quantized_channel_estimation_amd import Gmm_quant
    y = (np.sign(h_fit.real) + 1j * np.sign(h_fit.imag)) / np.sqrt(2)
    fits = {}
    for opt in ("host", "device"):
        g = Gmm_quant(n_components=5, covariance_type="full", max_iter=5, random_state=3, kmeans=opt)
        fits[opt] = _fit_quiet(g, h=y, n_bits=1, sigma2=0.1, quantizer=(None, None, None), quant_type="uniform")
    capsys.readouterr()  # the fit prints its lower bound per iteration
    for name in ("weights_", "means_", "covariances_", "n_iter_", "lower_bound_"):
        assert_array_equal(getattr(fits["device"].gm, name), getattr(fits["host"].gm, name), err_msg=name)
    assert_array_equal(fits["device"].covariances_quant, fits["host"].covariances_quant)


def test_mofa_initialize_device_equals_host(km_mod, h_fit):
    from quantized_channel_estimation_amd import Mofa
    out = {}
    for opt in ("host", "device"):
        np.random.seed(7)
        out[opt] = Mofa(5, 2, kmeans=opt, verbose=False)._initialize(h_fit)
    assert_allclose(out["device"][0], out["host"][0], rtol=0, atol=1e-12)  # means: the K-means centres
    for a, b in zip(out["device"][1:], out["host"][1:]):  # lambdas, psis, amps: the stream after the seeding
        assert_array_equal(a, b)
