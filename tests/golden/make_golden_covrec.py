"""Generate tests/golden/covrec.npz (and covrec_n256.npz, the N = 256 case): the reference's covariance recovery
from quantised samples (modules/cov_est_quant.py:31-88 est_cov_from_quant), called per component on d = x - mu_k
as the reference's M-step does (gmm_cplx_quant.py:817).

Runs ONLY in the build container (reference imported read-only, no bytecode written, the shims of make_golden.py).
Data per case: K SCM-Toeplitz covariances (2 paths, path_sigma 2.0), samples x = C_k^1/2 w (+ a mean of size
about 0.4 in the cases with means) + noise at the case's SNR, quantised with the reference's own get_quantizer /
quant; responsibilities are random, favour the true component and are normalised per row; nk = sum_b r + 10 eps
(the M-step's).  NumPy's global RNG is seeded (SEED) before each call of the reference.

Conditions on the inputs, asserted per case and recorded in the file (they are what lets FP64 code other than the
reference decide every sign and indicator alike, and reproduce the variance fits):
  * no entry of d is exactly 0;
  * the smallest distance | |d| - t | over all entries and positive thresholds t is >= 1e-9;
  * the call leaves the global RNG's state unchanged: no Gauss-Newton restart (utils.py:651-700).
The last cannot hold for a single sample (case n16_b1): with nk = 1 + 10 eps the clip bounds 1 / nk and (nk - 1) / nk
cross, every probability becomes 10 eps / nk, and the variance fit walks past 10 into the restart branch.  That case
is asserted to restart; its covariance is the one the seeded generator gives.
The recovered covariances are Hermitian up to rounding (asserted: asymmetry below 1e-14 relative) and are stored as
their packed upper triangles (covs_triu, np.triu_indices order).

Usage:  python -B tests/golden/make_golden_covrec.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SEED = 123
CASES = [  # tag, N, B, K, n_bits, quantizer type, means, snr
    ("n20_zm", 20, 517, 3, 3, "uniform", False, 5.0),
    ("n20_mean", 20, 517, 3, 3, "uniform", True, 5.0),
    ("n16_b2", 16, 130, 2, 2, "uniform", False, 5.0),
    ("n48_k9", 48, 1029, 9, 3, "lloyd", True, 10.0),
    ("n64_b4", 64, 2051, 3, 4, "uniform", False, 10.0),
    ("n256", 256, 70, 1, 2, "uniform", True, 5.0),
    ("n20_b3", 20, 3, 2, 2, "uniform", True, 5.0),
    ("n16_b1", 16, 1, 1, 2, "uniform", False, 5.0),
]
RESTARTS = {"n16_b1"}


def _sqrt_psd(C):
    import numpy as np
    w, Q = np.linalg.eigh(C)
    return Q * np.sqrt(np.clip(w, 0, None))


def main():
    import warnings
    import numpy as np
    from scipy.linalg import toeplitz
    from make_golden import _import_reference
    R = _import_reference()
    ut = R["ut"]
    from modules.cov_est_quant import est_cov_from_quant
    warnings.simplefilter("ignore")
    scm = R["SCMMulti"](path_sigma=2.0, n_path=2)
    small, big, tags = {}, {}, []  # the N = 256 case goes to a file of its own (size limit per committed file)
    for ci, (tag, N, B, K, nb, qt, with_means, snr) in enumerate(CASES):
        rng = np.random.default_rng(100 + ci)
        _, t = scm.generate_channel(K, 1, N, rng)
        comp = rng.integers(0, K, size=B)
        X = np.empty((B, N), complex)
        mu_true = np.zeros((K, N), complex)
        if with_means:
            mu_true = 0.4 * np.sqrt(0.5) * (rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
        for k in range(K):
            L = _sqrt_psd(toeplitz(t[k].astype(complex)).T)  # C = toeplitz(t)^T, as the genie estimator has it
            idx = np.nonzero(comp == k)[0]
            w = np.sqrt(0.5) * (rng.standard_normal((idx.size, N)) + 1j * rng.standard_normal((idx.size, N)))
            X[idx] = w @ L.T + mu_true[k]
        noise = np.sqrt(0.5) * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
        X = X + 10 ** (-snr / 20) * noise
        thr, lab, _ = ut.get_quantizer([snr], nb, qt)[snr]
        thr, lab = np.asarray(thr, float), np.asarray(lab, float)
        X = np.ascontiguousarray(ut.quant(X, nb, thr, lab), dtype=complex)
        resp = rng.random((B, K))
        resp[np.arange(B), comp] += 2.0
        resp /= resp.sum(axis=1)[:, None]
        nk = resp.sum(axis=0) + 10 * np.finfo(float).eps
        # the means the recovery is centred on: a perturbed copy of the true ones (as fitted means would be)
        means = mu_true + (0.02 * (rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))) if with_means else 0)
        pos = thr[(thr.shape[0] - 1) // 2 + 1:]
        covs = np.empty((K, N, N), complex)
        restarted = False
        margin = np.inf
        for k in range(K):
            d = X - means[k]
            parts = np.stack([d.real, d.imag])
            assert np.all(parts != 0.0), (tag, k, "an entry of d is exactly 0")
            margin = min(margin, float(np.min(np.abs(np.abs(parts)[..., None] - pos))))
            np.random.seed(SEED)
            before = np.random.get_state()
            covs[k] = est_cov_from_quant(d, nb, thr, resp[:, k], nk[k])
            after = np.random.get_state()
            restarted |= not (np.array_equal(before[1], after[1]) and before[2:] == after[2:])
        assert margin >= 1e-9, (tag, margin)
        assert restarted == (tag in RESTARTS), (tag, "Gauss-Newton restart", restarted)
        assert np.isfinite(covs).all(), tag
        # Hermitian up to rounding (diag(r) sin-law(corr) diag(r)): stored as the packed upper triangle
        asym = float(np.linalg.norm(covs - covs.conj().transpose(0, 2, 1)) / np.linalg.norm(covs))
        assert asym < 1e-14, (tag, asym)
        out = big if N > 128 else small
        p = tag + "__"
        out[p + "X"], out[p + "resp"], out[p + "means"] = X, resp, means
        out[p + "with_means"] = np.bool_(with_means)
        out[p + "thr"], out[p + "lab"], out[p + "n_bits"] = thr, lab, np.int64(nb)
        out[p + "qtype"] = np.array(qt)
        out[p + "covs_triu"] = covs[:, np.triu_indices(N)[0], np.triu_indices(N)[1]]
        out[p + "tie_margin"] = np.float64(margin)
        out[p + "no_zero_d"] = np.bool_(True)
        out[p + "rng_unchanged"] = np.bool_(not restarted)
        tags.append(tag)
        print(f"{tag}: tie margin {margin:.3e}, restart {restarted}")
    small["tags"] = np.array(tags)
    small["seed"] = np.int64(SEED)
    np.savez_compressed(os.path.join(HERE, "covrec.npz"), **small)
    np.savez_compressed(os.path.join(HERE, "covrec_n256.npz"), **big)
    print("wrote covrec.npz, covrec_n256.npz:", tags)


if __name__ == "__main__":
    main()
