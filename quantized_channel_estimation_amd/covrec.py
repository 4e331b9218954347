"""Covariance recovery from quantised samples (reference cov_est_quant.py:31-88 ``est_cov_from_quant``; the loop
body of Covariance_recovery.py is built on it).

The B-sized part -- the responsibility-weighted 1-bit sign correlation and the per-dimension threshold
probabilities of d = x - mu_k, for all K components -- is one device pass over X (``qce_quant_moments``,
csrc/qce_quant_moments.hip).  The per-component algebra that follows (arcsine law, the scalar Gauss-Newton variance
fits) is ``_em_quant.cov_from_quant`` on the host: the solver draws its restarts from NumPy's global generator, as
the reference does.
"""
import numpy as np

from . import _em_quant, _lib

MAX_FEATURES = 256
MAX_THRESHOLDS = 15


def _is_tensor(a):
    return a is not None and not isinstance(a, np.ndarray) and type(a).__module__.split(".")[0] == "torch"


def _shape_checks(X, resp, means, thresholds):
    """Argument errors, before the library is touched.  Returns (B, N, K, positive thresholds)."""
    if X.ndim != 2:
        raise ValueError("X must be (n_samples, n_features)")
    B, N = int(X.shape[0]), int(X.shape[1])
    if B < 1 or N < 1:
        raise ValueError("X must hold at least one sample and one feature")
    if N > MAX_FEATURES:
        raise NotImplementedError(f"quant_moments supports n_features <= {MAX_FEATURES}, not {N}")
    thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(_em_quant._positive_thresholds(thresholds))
    if thr.shape[0] > MAX_THRESHOLDS:
        raise NotImplementedError(f"quant_moments supports at most {MAX_THRESHOLDS} positive thresholds "
                                  f"(5 bits), not {thr.shape[0]}")
    if thr.shape[0] and (not thr[0] > 0 or np.any(np.diff(thr) <= 0)):
        raise ValueError("the positive thresholds must be ascending")
    if resp is not None and (resp.ndim != 2 or resp.shape[0] != B):
        raise ValueError("resp must be (n_samples, n_components)")
    K = 1 if resp is None else int(resp.shape[1])
    if means is not None:
        if means.ndim != 2 or means.shape[1] != N:
            raise ValueError("means must be (n_components, n_features)")
        if resp is None and means.shape[0] > 1:
            raise ValueError("resp=None is one component of unit weights: means must have one row")
        if means.shape[0] != K:
            raise ValueError(f"means has {means.shape[0]} rows for {K} components")
    if K < 1:
        raise ValueError("resp must have at least one column")
    return B, N, K, thr


def quant_moments(X, resp=None, means=None, thresholds=None, device=0, out="host"):
    """(nk (K,), corr (K, N, N), probs (K, N, T, 2)) of d = x - means[k] weighted by resp[:, k]:
    nk = sum_b r + 10 eps, corr = sum_b r s s^H / nk with s = (sign Re d + j sign Im d) / sqrt 2, and
    probs[k, i, t] = sum_b r 1(|Re d_i| < thr_t) / nk, sum_b r 1(|Im d_i| < thr_t) / nk.

    X (B, N) complex128 and resp (B, K) float64 are NumPy arrays or tensors on ``device`` (used in place);
    resp None: unit weights, K = 1; means (K, N) or None (zero).  thresholds: the quantiser's full symmetric
    threshold vector (its positive half is used); None: corr only, probs is (K, N, 0, 2).  out: "host" (NumPy) or
    "device" (tensors)."""
    if out not in ("host", "device"):
        raise ValueError("out must be 'host' or 'device'")
    if not _is_tensor(X):
        X = np.ascontiguousarray(X, dtype=np.complex128)
    if resp is not None and not _is_tensor(resp):
        resp = np.ascontiguousarray(resp, dtype=np.float64)
    if means is not None and not _is_tensor(means):
        means = np.ascontiguousarray(means, dtype=np.complex128)
        if means.ndim == 1:
            means = means[None, :]
    B, N, K, thr = _shape_checks(X, resp, means, thresholds)
    T = int(thr.shape[0])
    lib = _lib.load()
    on_device = out == "device" or any(_is_tensor(a) for a in (X, resp, means))
    if not on_device:
        nk = np.empty(K)
        corr = np.empty((K, N, N), dtype=np.complex128)
        probs = np.empty((K, N, T, 2))
        _lib.check(lib.qce_quant_moments(_lib.ptr(X), B, N, K, _lib.ptr(resp), _lib.ptr(means), _lib.ptr(thr), T,
                                         _lib.ptr(nk), _lib.ptr(corr), _lib.ptr(probs) if T else None, int(device),
                                         _lib.IO_HOST, None))
        return nk, corr, probs
    import torch
    dev = torch.device("cuda", int(device))

    def resident(a, dtype, what):
        if a is None:
            return None
        if not _is_tensor(a):
            return torch.from_numpy(a).to(dev)
        if a.device != dev or a.dtype != dtype:
            raise ValueError(f"{what} must be a {dtype} tensor on {dev}")
        return a.contiguous()  # a contiguous tensor is used in place

    X = resident(X, torch.complex128, "X")
    resp = resident(resp, torch.float64, "resp")
    means = resident(means, torch.complex128, "means")
    nk = torch.empty(K, dtype=torch.float64, device=dev)
    corr = torch.empty((K, N, N), dtype=torch.complex128, device=dev)
    probs = torch.empty((K, N, T, 2), dtype=torch.float64, device=dev)
    _lib.check(lib.qce_quant_moments(_lib.ptr(X), B, N, K, _lib.ptr(resp), _lib.ptr(means), _lib.ptr(thr), T,
                                     _lib.ptr(nk), _lib.ptr(corr), _lib.ptr(probs) if T else None, int(device),
                                     _lib.IO_DEVICE, torch.cuda.current_stream(dev).cuda_stream))
    if out == "device":
        return nk, corr, probs
    return nk.cpu().numpy(), corr.cpu().numpy(), probs.cpu().numpy()


def est_cov_from_quant(x, n_bits, thresholds, resp, nk, x0_vec=None, device=0):
    """Drop-in for the reference's est_cov_from_quant (cov_est_quant.py:31-88): the unquantised covariance (N, N) of
    one component from its quantised samples x (B, N), their weights resp (B,) and the caller's nk; x0_vec (N,)
    starts the variance fits (None: 1.0 in every dimension)."""
    thr = _em_quant._positive_thresholds(thresholds)
    if thr.shape[0] != int(2 ** (n_bits - 1) - 1):
        raise ValueError(f"{n_bits}-bit data has {int(2 ** (n_bits - 1) - 1)} positive thresholds, not {thr.shape[0]}")
    r = resp.reshape(-1, 1) if _is_tensor(resp) else np.asarray(resp, dtype=np.float64).reshape(-1, 1)
    nk_dev, corr, probs = quant_moments(x, r, None, thresholds, device=device)
    scale = nk_dev[0] / float(nk)  # the reference normalises by the nk it is given
    x0 = np.ones(corr.shape[1]) if x0_vec is None else np.asarray(x0_vec)
    return _em_quant.cov_from_quant(corr[0] * scale, probs[0] * scale, float(nk), thresholds, x0)


def recover_covariances(X, resp, thresholds, means=None, x0=None, device=0):
    """The recovered covariances (K, N, N) of all components: one quant_moments call, then est_cov_from_quant's
    host algebra per component with the moments' own nk.  x0 (K, N) or (N,) starts the variance fits (None: 1.0)."""
    nk, corr, probs = quant_moments(X, resp, means, thresholds, device=device)
    K, N = corr.shape[0], corr.shape[1]
    x0 = np.ones((K, N)) if x0 is None else np.broadcast_to(np.asarray(x0), (K, N))
    return np.stack([_em_quant.cov_from_quant(corr[k], probs[k], nk[k], thresholds, x0[k]) for k in range(K)])
