"""The NumPy reference of the device Lloyd loop (tests/kmeans_ref.py) against sklearn's KMeans: the reference the GPU
tests and the CPU plumbing tests stand on.  No GPU."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kmeans_ref as R

MARGIN_MIN = 1e-9  # a fixture whose closest call drifts near a tie fails here instead of flaking on a device


def _run_ref(e, max_iter=300, tol=1e-4):
    """lloyd_ref as KMeans.fit would drive it: (result, RandomState after seeding, mean)."""
    from sklearn.cluster import kmeans_plusplus
    Xr, Xc, mean = R.centred(e["X"])
    tol_abs = tol * np.mean(np.var(Xr, axis=0))
    rs = np.random.RandomState(e["seed"])
    if e["init"] is None:
        C0, _ = kmeans_plusplus(Xc, e["K"], random_state=rs)
    else:
        C0 = e["init"] - mean
    return R.lloyd_ref(Xc, C0, tol_abs, max_iter), rs, mean


def _check(e, res, mean):
    labels, C, inertia, n_iter, info = res
    km = e["km"]
    if e["K"] > 1:
        assert info["margin"] > MARGIN_MIN, f"reference margin {info['margin']:.3e}: the fixture is near a tie"
    assert_array_equal(labels, km.labels_)
    assert n_iter == km.n_iter_
    assert_allclose(C + mean, km.cluster_centers_, rtol=0, atol=1e-12)
    assert_allclose(inertia, km.inertia_, rtol=1e-10, atol=0)
    return info


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_reference_equals_sklearn(i):
    e = R.expected(f"case{i}")
    res, rs, mean = _run_ref(e)
    info = _check(e, res, mean)
    # every case stops on unchanged labels, except K = B: each row is its own centre, so the first shift is zero
    assert info["strict"] == (e["K"] < e["X"].shape[0]) and info["relocated"] == 0
    rs2 = np.random.RandomState()
    rs2.set_state(e["rs_state"])
    assert_array_equal(rs.rand(4), rs2.rand(4))  # the public kmeans_plusplus leaves the stream where KMeans.fit does


@pytest.mark.parametrize("i", range(len(R.NONSTRICT)))
def test_reference_nonstrict_stops(i):
    """max_iter and tol stops: the final re-assignment against the last centres."""
    e = R.expected(f"nonstrict{i}")
    res, _, mean = _run_ref(e, **e["kw"])
    info = _check(e, res, mean)
    # the K = 130 case reaches unchanged labels before its shift falls under tol = 0.05; the other three stop early
    assert info["strict"] == (i == 3)


def test_reference_empty_cluster():
    """A centre far from every row is empty after the first assignment and takes the farthest row."""
    e = R.expected("empty")
    assert_array_equal(np.bincount(e["km"].labels_, minlength=4), [1, 156, 311, 132])
    assert e["km"].n_iter_ == 3
    res, _, mean = _run_ref(e)
    info = _check(e, res, mean)
    assert info["relocated"] >= 1


def test_reference_exact_ties_take_the_lowest_index():
    X, C = R.tie_case()
    labels, margins, S = R.assign(X, C)
    assert int((margins == 0).sum()) == 124
    assert not np.any(labels == 3)  # centre 3 copies centre 1
    best = S.min(axis=1)
    for b in np.flatnonzero(margins == 0):
        assert labels[b] == np.flatnonzero(S[b] == best[b])[0]


def test_relocation_order():
    d = np.array([1.0, 5.0, 3.0, 5.0, 0.0])
    assert_array_equal(R.relocation_rows(d, 3), [1, 3, 2])
