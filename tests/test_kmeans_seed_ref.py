"""The pre-drawn random numbers and the NumPy model of the device k-means++ seeding (tests/kmeans_seed_ref.py) against
sklearn's kmeans_plusplus, and the host plumbing of ``seeding="device"`` / ``kmeans="device-seeded"`` with the model
standing in for the device.  No GPU."""
import copy
import pickle

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kmeans_ref as R
import kmeans_seed_ref as S


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", S.PARITY_NAMES + S.EXACT_NAMES)
def test_predraw_leaves_the_stream_where_sklearn_does(name):
    e = S.expected(name)
    assert _same_state(e["pre_state"], e["rs_state"])
    K = e["K"]
    assert 0 <= e["first"] < e["Xz"].shape[0]
    assert e["U"].shape == (K - 1, 2 + int(np.log(K)))
    assert np.all((e["U"] >= 0) & (e["U"] < 1))


def test_predraw_over_three_restarts():
    from sklearn.cluster import kmeans_plusplus
    from quantized_channel_estimation_amd import kmeans
    d = S.data("parity1")
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    for _ in range(3):
        kmeans_plusplus(d["Xs"], d["K"], random_state=a)
        kmeans.predraw(b, d["Xz"].shape[0], d["K"])
        assert _same_state(a.get_state(), b.get_state())


def test_predraw_takes_the_number_of_trials():
    from sklearn.cluster import kmeans_plusplus
    from quantized_channel_estimation_amd import kmeans
    d = S.data("parity0")
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    kmeans_plusplus(d["Xs"], d["K"], random_state=a, n_local_trials=7)
    _, U = kmeans.predraw(b, d["Xz"].shape[0], d["K"], n_local_trials=7)
    assert U.shape == (d["K"] - 1, 7) and _same_state(a.get_state(), b.get_state())


@pytest.mark.parametrize("name", S.PARITY_NAMES)
def test_model_equals_sklearn_with_margins(name):
    """The margins are a condition on the inputs (the tests/test_gpu_kmeans.py convention), not a tolerance: a case
    that misses them gets another seed."""
    e = S.expected(name)
    m = e["model"]
    print(name, "search margin", m["search_margin"], "argmin margin", m["argmin_margin"])
    assert_array_equal(m["indices"], e["sk_indices"])
    assert m["search_margin"] > 1e-9 and m["argmin_margin"] > 1e-9


@pytest.mark.parametrize("name", S.EXACT_NAMES)
def test_model_equals_sklearn_on_exact_data(name):
    e = S.expected(name)
    assert_array_equal(e["model"]["indices"], e["sk_indices"])
    assert np.all(e["model"]["pot"] == np.round(e["model"]["pot"]))  # integer data: every sum is exact


def test_exact_cases_hold_what_they_are_for():
    tie = S.data("tie6")["Xs"]
    assert np.unique(tie, axis=0).shape[0] < tie.shape[0]  # duplicate rows
    z = S.expected("zero_pot")["model"]
    assert z["pot"][2] == 0 and list(z["indices"][3:]) == [0, 0]  # a zero potential selects row 0
    for name in ("int64", "int257"):  # K = B: every distinct row is taken before the potential is zero
        e = S.expected(name)
        assert e["K"] == e["Xz"].shape[0]
    assert S.expected("int1024")["U"].shape[1] == 8


@pytest.mark.parametrize("chunked", [64, 256, 1024])
def test_search_is_searchsorted_on_exact_data(chunked):
    """On integer data the level-by-level search is np.searchsorted on the cumulative sum, whatever the chunk size."""
    rng = np.random.default_rng(chunked)
    closest = rng.integers(0, 5, 3000).astype(np.float64)
    closest[rng.integers(0, 3000, 400)] = 0
    C = -(-closest.shape[0] // chunked)
    part = S.chunk_sums(closest[None, :], chunked, C)[0]
    cum = np.cumsum(closest)
    assert part.sum() == cum[-1]
    for r in list(rng.uniform(0, cum[-1], 50)) + [0.0, 1.0, cum[-1], cum[1500]]:
        want = min(int(np.searchsorted(cum, r, side="left")), closest.shape[0] - 1)
        assert S.search(closest, part, r, chunked, C)[0] == want


@pytest.mark.parametrize("name", ["case1", "case3", "nonstrict0"])
def test_fit_with_device_seeding_equals_sklearn(name):
    from quantized_channel_estimation_amd import DeviceKMeans
    e = R.expected(name)
    rs = np.random.RandomState(e["seed"])
    km = DeviceKMeans(e["K"], random_state=rs, seeding="device", _seed=S.seed_for_kmeans, _lloyd=R.lloyd_ref,
                      **e["kw"]).fit(e["X"])
    ref = e["km"]
    assert_array_equal(km.labels_, ref.labels_)
    assert km.n_iter_ == ref.n_iter_
    assert_allclose(km.cluster_centers_, ref.cluster_centers_, rtol=0, atol=1e-12)
    assert_allclose(km.inertia_, ref.inertia_, rtol=1e-10, atol=0)
    rs2 = np.random.RandomState()
    rs2.set_state(e["rs_state"])
    assert_array_equal(rs.rand(4), rs2.rand(4))


def test_seeding_is_ignored_for_other_inits():
    from quantized_channel_estimation_amd import DeviceKMeans
    e = R.expected("empty")

    def never(*a):
        raise AssertionError("the seeding stand-in was called")
    km = DeviceKMeans(e["K"], init=e["init"], seeding="device", _seed=never, _lloyd=R.lloyd_ref).fit(e["X"])
    assert_array_equal(km.labels_, e["km"].labels_)


def _classes():
    from quantized_channel_estimation_amd import GaussianMixtureCplx, Gmm_nbit, Gmm_quant, Mofa
    gm = dict(n_components=3, covariance_type="full")
    return [(Gmm_nbit, (), gm), (Gmm_quant, (), gm), (GaussianMixtureCplx, (), gm), (Mofa, (3, 2), {})]


@pytest.mark.parametrize("i", range(4))
def test_option_is_accepted_and_kept(i):
    cls, args, kw = _classes()[i]
    obj = cls(*args, kmeans="device-seeded", **kw)
    assert obj.kmeans == "device-seeded"
    assert pickle.loads(pickle.dumps(obj)).kmeans == "device-seeded"
    assert copy.deepcopy(obj).kmeans == "device-seeded"
    with pytest.raises(ValueError, match="kmeans"):
        cls(*args, kmeans="bogus", **kw)


def test_option_survives_from_reference():
    from quantized_channel_estimation_amd import Gmm_nbit, Mofa, inputs
    means, covs, w = inputs.synthetic_model(2, 4, seed=1)
    g = Gmm_nbit.from_params(means, covs, w)
    g.kmeans = "device-seeded"
    assert Gmm_nbit.from_reference(g).kmeans == "device-seeded"
    assert Gmm_nbit.from_reference(g, kmeans="device-seeded").kmeans == "device-seeded"
    m = Mofa.from_params(None, np.ones((2, 4, 1), complex), np.ones((2, 4)), np.array([0.5, 0.5]))
    m.kmeans = "device-seeded"
    assert Mofa.from_reference(m).kmeans == "device-seeded"


def test_seeding_keyword_is_validated():
    from quantized_channel_estimation_amd import DeviceKMeans, kmeans
    with pytest.raises(ValueError, match="seeding"):
        DeviceKMeans(3, seeding="bogus")
    assert DeviceKMeans(3).seeding == "host"
    assert kmeans.seeding_of("device-seeded") == "device" and kmeans.seeding_of("device") == "host"
    with pytest.raises(ValueError, match="kmeans"):
        kmeans.check_kmeans_option("bogus")
