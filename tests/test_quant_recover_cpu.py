"""Covariance recovery on the device, the parts that need no GPU: the ``recovery=`` / ``solver=`` options, the NumPy
restatement of the two kernels (quant_recover_ref.py) against the host recovery code it replaces
(``_em_quant.variance_fit`` / ``cov_from_quant`` / ``_eig_clip``), and the routing of ``recovery="device"`` through
``_em_quant`` with that restatement standing in for the library.

Tolerance: 1e-9, the tolerance quant_fit.npz and quant_fit_struct.npz pin the host path to the reference with."""
import pickle

import numpy as np
import pytest

import quant_recover_ref as R
from conftest import rel_fro

TOL = 1e-9


def test_recovery_option_is_validated_and_kept():
    from quantized_channel_estimation_amd import Gmm_quant
    kw = dict(n_components=3, covariance_type="full")
    with pytest.raises(ValueError, match="recovery"):
        Gmm_quant(recovery="bogus", **kw)
    assert Gmm_quant(**kw).recovery == "host"
    g = Gmm_quant(recovery="device", **kw)
    assert g.recovery == "device"
    assert pickle.loads(pickle.dumps(g)).recovery == "device"
    assert Gmm_quant.from_reference(g).recovery == "device"


def test_pickle_without_the_option_loads_as_host():
    from quantized_channel_estimation_amd import Gmm_quant, _em_quant
    g = Gmm_quant(n_components=2, covariance_type="full")
    del g.__dict__["recovery"]  # an object pickled before the option existed
    old = pickle.loads(pickle.dumps(g))
    assert "recovery" not in old.__dict__
    old.n_bits, old.sigma2, old.quantizer = 1, 0.1, (None, None, None)

    class Backend:
        gains = moments = None  # the 1-bit branch calls neither

        def mstep(self, resp):
            Q = np.stack([np.eye(4, dtype=complex) * 0.5] * 2)
            return np.array([3.0, 5.0]), np.zeros((2, 4), complex), Q

    seen = {}
    orig = _em_quant.quant_covariances

    def spy(*a, **kw):
        seen.update(kw)
        return orig(*a, **kw)

    _em_quant.quant_covariances = spy
    try:
        _em_quant.estimate_parameters(old, Backend(), resp=None)
    finally:
        _em_quant.quant_covariances = orig
    assert seen["recovery"] == "host"
    old.recovery = "bogus"  # a bad value set later stops the M-step
    with pytest.raises(ValueError, match="recovery"):
        _em_quant.estimate_parameters(old, Backend(), resp=None)


def test_solver_option_is_validated():
    from quantized_channel_estimation_amd import covrec
    X = np.ones((4, 2), complex)
    thr = R.symmetric([0.5])
    with pytest.raises(ValueError, match="solver"):
        covrec.recover_covariances(X, np.ones((4, 1)), thr, solver="bogus")
    with pytest.raises(ValueError, match="solver"):
        covrec.est_cov_from_quant(X, 2, thr, np.ones(4), 4.0, solver="bogus")
    with pytest.raises(ValueError, match="solver"):
        covrec.cov_from_moments(np.ones((1, 2, 2), complex), np.ones((1, 2, 1, 2)), np.ones(1), thr, solver="bogus")
    with pytest.raises(ValueError, match="prep"):
        covrec.eig_clip(np.eye(2), 1e-6, prep="bogus")


# ---- the restatement of the variance-fit kernel against the host solver -------------------------------------------
def host_fits(probs, nk, pos, x0):
    """(s2, steps, drew) of the host solver per entry; drew: the entry consumed NumPy's global generator."""
    from quantized_channel_estimation_amd import _em_quant
    K, D = probs.shape[:2]
    thres = np.concatenate([pos, pos])
    s2, steps, drew = np.empty((K, D)), np.zeros((K, D), int), np.zeros((K, D), bool)
    for k in range(K):
        for d in range(D):
            before = np.random.get_state()
            s2[k, d], steps[k, d] = _em_quant.variance_fit(probs[k, d], nk[k], thres, x0[k, d])
            after = np.random.get_state()
            drew[k, d] = not (np.array_equal(before[1], after[1]) and before[2:] == after[2:])
    return s2, steps, drew


@pytest.mark.parametrize("T", [1, 3, 63])
def test_variance_fit_ref_matches_host(T):
    probs, nk, pos, x0 = R.fit_case(T)
    s2, status, iters = R.variance_fits_ref(probs, nk, pos, x0)
    np.random.seed(7)
    h_s2, h_steps, drew = host_fits(probs, nk, pos, x0)
    assert not drew.any() and not status.any()
    assert np.array_equal(iters, h_steps)
    assert np.max(np.abs(s2 - h_s2) / h_s2) <= TOL


def test_variance_fit_ref_flags_what_the_host_restarts():
    probs, nk, pos, x0 = R.fit_case(3, far=(5, 11))
    s2, status, iters = R.variance_fits_ref(probs, nk, pos, x0)
    np.random.seed(7)
    h_s2, h_steps, drew = host_fits(probs, nk, pos, x0)
    assert np.array_equal(status != 0, drew)
    want = np.zeros_like(drew)
    want[:, [5, 11]] = True
    assert np.array_equal(drew, want)
    ok = ~drew
    assert np.array_equal(iters[ok], h_steps[ok])
    assert np.max(np.abs(s2[ok] - h_s2[ok]) / h_s2[ok]) <= TOL


def test_variance_fit_ref_flags_non_finite_values():
    probs, nk, pos, x0 = R.fit_case(3)
    probs[0, 2, 1, 0] = np.nan
    x0[1, 3] = np.inf
    _, status, _ = R.variance_fits_ref(probs, nk, pos, x0)
    want = np.zeros_like(status)
    want[0, 2] = want[1, 3] = 1
    assert np.array_equal(status, want)


def test_cov_from_fits_matches_cov_from_quant():
    """The device solver's assembly (arcsine law, r corr r) from the restated fits is cov_from_quant."""
    from quantized_channel_estimation_amd import _em_quant, covrec
    probs, nk, pos, x0 = R.fit_case(3)
    corr = R.corr_case()
    s2, _, _ = R.variance_fits_ref(probs, nk, pos, x0)
    got = covrec._cov_from_fits(corr, s2)
    thr = R.symmetric(pos)
    for k in range(corr.shape[0]):
        assert rel_fro(got[k], _em_quant.cov_from_quant(corr[k], probs[k], nk[k], thr, x0[k])) <= TOL


# ---- the restatement of the clip kernel against eigh ---------------------------------------------------------------
def test_tournament_meets_every_pair_once():
    for n in (2, 8, 64):
        seen = set()
        for r in range(n - 1):
            step = R.pairs_of_step(n, r)
            assert sorted(i for pq in step for i in pq) == list(range(n))  # disjoint: one rotation per index
            seen.update(step)
        assert len(seen) == n * (n - 1) // 2


@pytest.mark.parametrize("name,C", R.clip_cases(), ids=[n for n, _ in R.clip_cases()])
def test_eig_clip_ref_matches_eigh(name, C):
    from quantized_channel_estimation_amd import _em_quant
    out, status, sweeps = R.eig_clip_ref(C, 1e-6)
    assert status == 0 and sweeps <= 12
    assert rel_fro(out, _em_quant._eig_clip(C, 1e-6)) <= TOL
    assert np.max(np.abs(out - out.conj().T)) <= 1e-13


def test_eig_clip_ref_identity_takes_no_sweep():
    out, status, sweeps = R.eig_clip_ref(np.eye(8), 1e-6)
    assert (status, sweeps) == (0, 0)
    assert np.array_equal(out, np.eye(8))


# ---- recovery="device" through _em_quant, the restatement standing in for the library ------------------------------
@pytest.fixture
def ref_library(monkeypatch):
    """covrec.variance_fits / eig_clip served by quant_recover_ref (no library call)."""
    from quantized_channel_estimation_amd import _em_quant, covrec
    calls = {"fits": 0, "clip": 0, "flagged": 0}

    def variance_fits(probs, nk, thresholds, x0, device=0):
        calls["fits"] += 1
        K, N = probs.shape[:2]
        out = R.variance_fits_ref(probs, nk, _em_quant._positive_thresholds(thresholds),
                                  np.broadcast_to(np.real(x0), (K, N)))
        calls["flagged"] += int(out[1].sum())
        return out

    def eig_clip(covs, floor, device=0, prep="plain", s2=None, diag_pre=0.0, diag_post=0.0, return_info=False):
        calls["clip"] += 1
        out = np.empty_like(covs)
        for k in range(covs.shape[0]):
            a = covrec._prepared(covs[k], prep, None if s2 is None else s2[k], diag_pre)
            out[k], status, _ = R.eig_clip_ref(a, floor)
            assert status == 0
            out[k] += diag_post * np.eye(a.shape[0])
        return out

    monkeypatch.setattr(covrec, "variance_fits", variance_fits)
    monkeypatch.setattr(covrec, "eig_clip", eig_clip)
    return calls


@pytest.mark.parametrize("tag", ["b1_zm", "b2u_zm", "inf_mean", "t_b1_zm", "t_b2u_zm"])
def test_device_recovery_routing_matches_host(ref_library, tag):
    """quant_covariances / quant_covariances_inv with recovery="device" against recovery="host" on the first M-step's
    moments of a fixture fit (all three n_bits branches, and the inverse-EM ones)."""
    import os
    from conftest import GOLDEN
    from quantized_channel_estimation_amd import _em_quant
    from test_quant_fit import NumpyBackend, _case
    struct = tag.startswith("t_")
    fx = dict(np.load(os.path.join(GOLDEN, "quant_fit_struct.npz" if struct else "quant_fit.npz"), allow_pickle=False))
    y, n_bits, qt, quantizer, zm, K, _, sigma2 = _case(fx, tag)
    y = np.asarray(y, complex)
    B, N = y.shape
    be = NumpyBackend(y, K, zm, n_bits, sigma2, quantizer, qt)
    rng = np.random.default_rng(3)
    resp = rng.random((B, K))
    resp /= resp.sum(axis=1, keepdims=True)
    nk, means, Q = be.mstep(resp)
    moments = lambda: be.moments(resp, None if zm else means)  # noqa: E731
    reg = 1e-6
    out = {}
    for recovery in ("host", "device"):
        np.random.seed(11)
        if struct:
            F2 = np.fft.fft(np.eye(2 * N))[:, :N] / np.sqrt(2 * N)
            prev = np.stack([np.eye(N, dtype=complex)] * K)
            Sigma = np.ones((K, 2 * N))
            out[recovery] = _em_quant.quant_covariances_inv(Q, nk, reg, n_bits, sigma2, quantizer, moments, be.gains,
                                                            F2, Sigma, prev, recovery=recovery) + (Sigma,)
        else:
            out[recovery] = _em_quant.quant_covariances(Q, nk, reg, n_bits, sigma2, quantizer, moments, be.gains,
                                                        recovery=recovery)
        out[recovery + "_state"] = np.random.get_state()
    assert ref_library["clip"] == 1
    assert ref_library["fits"] == (0 if n_bits in (1, np.inf) else 1)
    assert ref_library["flagged"] == 0
    for a, b in zip(out["host"], out["device"]):
        assert rel_fro(b, a) <= TOL
    assert all(np.array_equal(a, b) for a, b in zip(out["host_state"], out["device_state"]))
