"""covrec on the device: the fused moments pass (qce_quant_moments, csrc/qce_quant_moments.hip) against its NumPy
restatement, its exact decisions (sign(0) = 0, strict indicator), placement and determinism, and the recovery
against the reference's est_cov_from_quant (tests/golden/covrec.npz, make_golden_covrec.py).

Bound of the moments: the entries are sums of B terms of size <= r_bk normalised by their own total, each side's
summation error is at most (B - 1) eps, so the two differ by less than 4 B eps per element."""
import numpy as np
import pytest

from conftest import rel_fro
from test_covrec import TAGS, case, case_moments, positive

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def covrec():
    from quantized_channel_estimation_amd import _lib, covrec
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    return covrec


_dev = {}


def device_moments(covrec, tag):
    """quant_moments of a fixture case from host arrays, computed once per session."""
    if tag not in _dev:
        c = case(tag)
        _dev[tag] = covrec.quant_moments(c["X"], c["resp"], c["means"], c["thr"])
    return _dev[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_gpu_quant_moments_match_numpy(covrec, tag):
    c = case(tag)
    nk0, corr0, probs0 = case_moments(tag)
    nk, corr, probs = device_moments(covrec, tag)
    B = c["X"].shape[0]
    bound = 4 * B * EPS
    e_nk = float(np.max(np.abs(nk - nk0) / nk0))
    e_corr = float(np.max(np.abs(corr - corr0)))
    e_probs = float(np.max(np.abs(probs - probs0)))
    print(f"{tag}: bound {bound:.3e} nk {e_nk:.3e} corr {e_corr:.3e} probs {e_probs:.3e}")
    assert corr.shape == corr0.shape and probs.shape == probs0.shape and nk.shape == nk0.shape
    assert e_nk <= bound
    assert e_corr <= bound
    assert e_probs <= bound


def test_gpu_quant_moments_exact_decisions(covrec):
    """Unweighted, K = 1, N = 20, B = 517, data on the labels of a 3-bit uniform quantiser of step 1/2 (dyadic values:
    every difference below is exact).  The means put entries of d exactly on 0 (sign 0, as np.sign) and exactly on
    a threshold (strict <: not counted)."""
    N, B = 20, 517
    thr = np.arange(-3, 4) * 0.5
    lab = np.arange(-4, 4) * 0.5 + 0.25
    rng = np.random.default_rng(42)
    z = 0.8 * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    X = lab[np.digitize(z.real, thr)] + 1j * lab[np.digitize(z.imag, thr)]
    mu = np.full(N, 0.1 + 0.05j)
    mu[0] = 0.25 + 0.05j    # Re d = 0 where Re x = 0.25
    mu[1] = 0.1 - 0.75j     # Im d = 0 where Im x = -0.75, |Im d| = 1.0 where Im x = 0.25 or -1.75
    mu[2] = -0.25 + 0.05j   # |Re d| = 0.5 where Re x = 0.25 or -0.75, |Re d| = 1.5 where Re x = 1.25 or -1.75
    mu[3] = 0.75 + 0.25j    # zeros in both parts, and both parts on thresholds
    d = X - mu[None, :]
    pos = positive(thr)
    zeros = (d.real == 0) | (d.imag == 0)
    ties = (np.abs(d.real)[..., None] == pos).any(-1) | (np.abs(d.imag)[..., None] == pos).any(-1)
    for f in (0, 1, 3):
        assert zeros[:, f].sum() > 10
    for f in (1, 2, 3):
        assert ties[:, f].sum() > 10
    assert not zeros[:, 4:].any() and not ties[:, 4:].any()
    S = np.sign(d.real) + 1j * np.sign(d.imag)
    gram = S.T @ S.conj()  # small integers: exact
    counts = np.stack([np.stack([(np.abs(d.real) < t).sum(0), (np.abs(d.imag) < t).sum(0)], -1) for t in pos], 1)
    nk, corr, probs = covrec.quant_moments(X, None, mu[None, :], thr)
    assert nk.shape == (1,) and corr.shape == (1, N, N) and probs.shape == (1, N, 3, 2)
    assert nk[0] == B + 10 * EPS
    g = 2 * nk[0] * corr[0]
    assert np.array_equal(np.rint(g.real), gram.real) and np.array_equal(np.rint(g.imag), gram.imag)
    assert np.max(np.abs(g - gram)) <= 1e-9
    assert np.array_equal(np.rint(nk[0] * probs[0]), counts)
    assert np.max(np.abs(nk[0] * probs[0] - counts)) <= 1e-9


def test_gpu_quant_moments_placement_and_determinism(covrec):
    import torch
    c = case("n20_mean")
    host = device_moments(covrec, "n20_mean")
    again = covrec.quant_moments(c["X"], c["resp"], c["means"], c["thr"])
    Xd = torch.from_numpy(c["X"]).cuda()
    Rd = torch.from_numpy(c["resp"]).cuda()
    dev = covrec.quant_moments(Xd, Rd, c["means"], c["thr"])
    res = covrec.quant_moments(Xd, Rd, torch.from_numpy(c["means"]).cuda(), c["thr"], out="device")
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in res)
    for a, b, d, e in zip(host, again, dev, res):
        assert np.array_equal(a, b)
        assert np.array_equal(a, d)
        assert np.array_equal(a, e.cpu().numpy())


def test_gpu_quant_moments_without_thresholds(covrec):
    c = case("n20_zm")
    nk0, corr0, _ = device_moments(covrec, "n20_zm")
    nk, corr, probs = covrec.quant_moments(c["X"], c["resp"], c["means"], None)
    assert np.array_equal(corr, corr0) and np.array_equal(nk, nk0)
    assert probs.shape == (3, 20, 0, 2)


@pytest.mark.parametrize("tag", TAGS)
def test_gpu_covrec_matches_reference(covrec, tag):
    c = case(tag)
    K = c["resp"].shape[1]
    nk = c["resp"].sum(axis=0) + 10 * EPS
    for k in range(K):
        d = c["X"] if c["means"] is None else c["X"] - c["means"][k]
        np.random.seed(c["seed"])
        got = covrec.est_cov_from_quant(d, c["n_bits"], c["thr"], c["resp"][:, k], nk[k])
        assert rel_fro(got, c["covs"][k]) < 1e-7, (tag, k)
    np.random.seed(c["seed"])
    allk = covrec.recover_covariances(c["X"], c["resp"], c["thr"], means=c["means"])
    assert allk.shape == c["covs"].shape
    assert rel_fro(allk, c["covs"]) < 1e-7, tag
