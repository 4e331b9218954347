"""Covariance recovery from quantised samples (reference cov_est_quant.py:31-88 ``est_cov_from_quant``; the loop
body of Covariance_recovery.py is built on it).

The B-sized part -- the responsibility-weighted 1-bit sign correlation and the per-dimension threshold
probabilities of d = x - mu_k, for all K components -- is one device pass over X (``qce_quant_moments``,
csrc/qce_quant_moments.hip).  The per-component algebra that follows (arcsine law, the scalar Gauss-Newton variance
fits) is ``_em_quant.cov_from_quant`` on the host: the solver draws its restarts from NumPy's global generator, as
the reference does.

Opt-in (``solver="device"``, ``Gmm_quant(recovery="device")``), csrc/qce_quant_recover.hip runs that algebra on the
device: ``variance_fits`` (all K N scalar fits in one call; a fit that would restart is flagged and redone here on
the host, so the generator is consumed as before) and ``eig_clip`` (the batched Hermitian eigenvalue clip of the
M-step, N <= 64).
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


SOLVERS = ("host", "device")
CLIP_MAX_FEATURES = 64  # qce_herm_eig_clip keeps A and V of one component in LDS
_PREPS = {"plain": _lib.CLIP_PLAIN, "sin": _lib.CLIP_SIN, "sin-scaled": _lib.CLIP_SIN_SCALED}


def check_solver(value, what="solver"):
    """'host' (the NumPy algebra of _em_quant, the default) or 'device' (csrc/qce_quant_recover.hip)."""
    if value not in SOLVERS:
        raise ValueError(f"{what} must be one of {SOLVERS}, not {value!r}")
    return value


def variance_fits(probs, nk, thresholds, x0, device=0):
    """The scalar Gauss-Newton variance fits of all (component, dimension) pairs on the device
    (``qce_quant_variance_fit``): probs (K, N, T, 2) and nk (K,) as quant_moments returns them, thresholds the
    quantiser's full symmetric threshold vector (its positive half is used, T >= 1), x0 (K, N) the start values.
    Returns (s2 (K, N), status (K, N) int32, iters (K, N) int32).  status 1: the fit reached a restart branch of the
    reference's solver (|s| < 0.1 or > 10, drawn from NumPy's global generator) or a non-finite value; its s2 is not
    a result and the entry is the caller's to redo on the host (``fit_variances`` does)."""
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    if probs.ndim != 4 or probs.shape[3] != 2:
        raise ValueError("probs must be (n_components, n_features, T, 2)")
    K, N, T = (int(v) for v in probs.shape[:3])
    thr = np.ascontiguousarray(_em_quant._positive_thresholds(thresholds))
    if thr.shape[0] != T or T < 1:
        raise ValueError(f"probs holds {T} thresholds per dimension, the quantiser has {thr.shape[0]} positive ones")
    nk = np.ascontiguousarray(nk, dtype=np.float64).reshape(-1)
    if nk.shape[0] != K:
        raise ValueError(f"nk must have {K} entries")
    x0 = np.ascontiguousarray(np.broadcast_to(np.real(np.asarray(x0)), (K, N)), dtype=np.float64)
    s2 = np.empty((K, N))
    status = np.empty((K, N), dtype=np.int32)
    iters = np.empty((K, N), dtype=np.int32)
    _lib.check(_lib.load().qce_quant_variance_fit(_lib.ptr(probs), _lib.ptr(nk), _lib.ptr(thr), T, _lib.ptr(x0), K, N,
                                                  _lib.ptr(s2), _lib.ptr(status), _lib.ptr(iters), int(device),
                                                  _lib.IO_HOST, None))
    return s2, status, iters


def fit_variances(probs, nk, thresholds, x0, device=0):
    """s2 (K, N) of ``variance_fits`` with the flagged entries redone by the host solver
    (``_em_quant.variance_fit``) in ascending (component, dimension) order: NumPy's global generator is consumed as
    the host path consumes it.  Returns (s2, status)."""
    s2, status, _ = variance_fits(probs, nk, thresholds, x0, device=device)
    flagged = np.argwhere(status != 0)  # row-major: ascending (k, d)
    if flagged.shape[0]:
        K, N = s2.shape
        x0 = np.broadcast_to(np.asarray(x0), (K, N))
        thr = _em_quant._positive_thresholds(thresholds)
        thr = np.concatenate((thr, thr), axis=0)
        for k, d in flagged:
            s2[k, d] = _em_quant.variance_fit(probs[k, d], nk[k], thr, x0[k, d])[0]
    return s2, status


def _prepared(c, prep, s2, diag_pre):
    """The clip's input of one component as the device forms it (host fall-back of eig_clip)."""
    c = np.array(c, dtype=np.complex128)
    if prep != "plain":
        c = np.sin(np.pi / 2 * c.real) + 1j * np.sin(np.pi / 2 * c.imag)
    if prep == "sin-scaled":
        r = np.sqrt(s2)
        c = r[:, None] * c * r[None, :]
    idx = np.arange(c.shape[0])
    c[idx, idx] += diag_pre
    return c


def eig_clip(covs, floor, device=0, prep="plain", s2=None, diag_pre=0.0, diag_post=0.0, return_info=False):
    """V max(L, floor) V^H + diag_post I of the Hermitian matrices A_k = V L V^H, all K at once on the device
    (``qce_herm_eig_clip``: parallel cyclic Jacobi, one workgroup per matrix).  A_k is covs[k] (K, N, N) -- or one
    (N, N) matrix -- after the element-wise preparation ``prep``: "plain"; "sin" = sin(pi/2 Re) + j sin(pi/2 Im);
    "sin-scaled" = the same times sqrt(s2[k][i] s2[k][j]); then + diag_pre I.  The lower triangles are read, as eigh
    reads them.  N > 64, and a matrix the iteration flags (30 sweeps without reaching 1e-14 ||A||_F off the diagonal),
    are clipped on the host with eigh.  return_info: also (status (K,), sweeps (K,)) as the device reported them
    (None for N > 64)."""
    if prep not in _PREPS:
        raise ValueError(f"prep must be one of {tuple(_PREPS)}, not {prep!r}")
    covs = np.ascontiguousarray(covs, dtype=np.complex128)
    single = covs.ndim == 2
    if single:
        covs = covs[None]
    if covs.ndim != 3 or covs.shape[1] != covs.shape[2] or covs.shape[1] < 1 or covs.shape[0] < 1:
        raise ValueError("covs must be (n_components, n_features, n_features)")
    K, N = int(covs.shape[0]), int(covs.shape[1])
    if prep == "sin-scaled":
        s2 = np.ascontiguousarray(s2, dtype=np.float64).reshape(K, N)
    else:
        s2 = None
    idx = np.arange(N)

    def on_host(k):
        c = _em_quant._eig_clip(_prepared(covs[k], prep, None if s2 is None else s2[k], diag_pre), floor)
        c[idx, idx] += diag_post
        return c

    status = sweeps = None
    if N > CLIP_MAX_FEATURES:
        out = np.stack([on_host(k) for k in range(K)])
    else:
        out = np.empty_like(covs)
        status = np.empty(K, dtype=np.int32)
        sweeps = np.empty(K, dtype=np.int32)
        _lib.check(_lib.load().qce_herm_eig_clip(_lib.ptr(covs), K, N, float(floor), _PREPS[prep], _lib.ptr(s2),
                                                 float(diag_pre), float(diag_post), _lib.ptr(out), _lib.ptr(status),
                                                 _lib.ptr(sweeps), int(device), _lib.IO_HOST, None))
        for k in np.flatnonzero(status):
            out[k] = on_host(k)
    if single:
        out = out[0]
    return (out, status, sweeps) if return_info else out


def _cov_from_fits(corr, s2):
    """est_cov_from_quant's last lines (cov_est_quant.py:49-50, :85-88): the arcsine law and the r corr r scaling."""
    corr = np.sin(np.pi / 2 * np.real(corr)) + 1j * np.sin(np.pi / 2 * np.imag(corr))
    r = np.sqrt(s2)
    return r[..., :, None] * corr * r[..., None, :]


def cov_from_moments(corr, probs, nk, thresholds, x0=None, device=0, solver="host"):
    """est_cov_from_quant's algebra for all components from the moments quant_moments returns: corr (K, N, N),
    probs (K, N, T, 2), nk (K,) -> the recovered covariances (K, N, N).  x0 (K, N) or (N,) starts the variance fits
    (None: 1.0).  solver "host": ``_em_quant.cov_from_quant``, one component after the other; "device": all K N
    variance fits in one ``variance_fits`` call, restarted fits redone on the host in the host's order."""
    check_solver(solver)
    K, N = corr.shape[0], corr.shape[1]
    x0 = np.ones((K, N)) if x0 is None else np.broadcast_to(np.asarray(x0), (K, N))
    if solver == "device":
        s2, _ = fit_variances(probs, nk, thresholds, x0, device=device)
        return _cov_from_fits(corr, s2)
    return np.stack([_em_quant.cov_from_quant(corr[k], probs[k], nk[k], thresholds, x0[k]) for k in range(K)])


def est_cov_from_quant(x, n_bits, thresholds, resp, nk, x0_vec=None, device=0, solver="host"):
    """Drop-in for the reference's est_cov_from_quant (cov_est_quant.py:31-88): the unquantised covariance (N, N) of
    one component from its quantised samples x (B, N), their weights resp (B,) and the caller's nk; x0_vec (N,)
    starts the variance fits (None: 1.0 in every dimension).  solver: "host" (the NumPy solver) or "device" (the
    variance fits on the device, restarted fits redone on the host)."""
    check_solver(solver)
    thr = _em_quant._positive_thresholds(thresholds)
    if thr.shape[0] != int(2 ** (n_bits - 1) - 1):
        raise ValueError(f"{n_bits}-bit data has {int(2 ** (n_bits - 1) - 1)} positive thresholds, not {thr.shape[0]}")
    r = resp.reshape(-1, 1) if _is_tensor(resp) else np.asarray(resp, dtype=np.float64).reshape(-1, 1)
    nk_dev, corr, probs = quant_moments(x, r, None, thresholds, device=device)
    scale = nk_dev[0] / float(nk)  # the reference normalises by the nk it is given
    x0 = None if x0_vec is None else np.asarray(x0_vec)
    return cov_from_moments(corr * scale, probs * scale, np.array([float(nk)]), thresholds, x0, device=device,
                            solver=solver)[0]


def recover_covariances(X, resp, thresholds, means=None, x0=None, device=0, solver="host"):
    """The recovered covariances (K, N, N) of all components: one quant_moments call, then est_cov_from_quant's
    algebra per component with the moments' own nk.  x0 (K, N) or (N,) starts the variance fits (None: 1.0).
    solver: "host" (NumPy, one component after the other) or "device" (all K N variance fits in one
    ``variance_fits`` call, restarted fits redone on the host)."""
    check_solver(solver)
    nk, corr, probs = quant_moments(X, resp, means, thresholds, device=device)
    return cov_from_moments(corr, probs, nk, thresholds, x0, device=device, solver=solver)
