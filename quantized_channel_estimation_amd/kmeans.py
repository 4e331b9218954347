"""K-means for the EM initialisation with the Lloyd loop on the device (``qce_kmeans_lloyd``,
csrc/qce_kmeans.hip).

``DeviceKMeans`` is sklearn's ``KMeans`` (dense data, unit weights, ``algorithm="lloyd"``) for the real view of
complex rows.  The host part is sklearn's own: the data are centred with their column mean, ``tol`` is scaled
by the mean column variance, and the seeds come from the public ``sklearn.cluster.kmeans_plusplus`` with the
caller's ``RandomState`` -- the same seeds, and the same stream afterwards, as ``KMeans(n_init=1,
random_state=rs).fit``.  With ``seeding="device"`` the same seeds are chosen on the device instead
(``qce_kmeans_seed``, csrc/qce_kmeans_seed.hip) from random numbers drawn in advance in sklearn's order
(``predraw``).  Otherwise only the Lloyd iterations move: they run on the resident complex128 rows in their stored
interleaved order (distances do not depend on the column order); centres are converted to and from sklearn's
``[Re | Im]`` column order here.
"""
import numpy as np

from . import _lib

KMEANS_OPTIONS = ("host", "device", "device-seeded")
DEVICE_OPTIONS = ("device", "device-seeded")  # the settings that cluster the resident data


def check_kmeans_option(value):
    """The ``kmeans=`` keyword of the fits: "host" (sklearn's KMeans, the default), "device" (host seeds, the Lloyd
    loop on the device) or "device-seeded" (the k-means++ seeds chosen on the device as well)."""
    if value not in KMEANS_OPTIONS:
        raise ValueError(f"kmeans must be 'host', 'device' or 'device-seeded', not {value!r}")
    return value


def seeding_of(option):
    """The ``seeding=`` of DeviceKMeans that a fit's ``kmeans=`` option stands for."""
    return "device" if option == "device-seeded" else "host"


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


def to_interleaved(C):
    """(K, 2N) columns [Re | Im] -> (re0, im0, re1, ...)."""
    C = np.asarray(C, dtype=np.float64)
    N = C.shape[-1] // 2
    out = np.empty_like(C)
    out[..., 0::2] = C[..., :N]
    out[..., 1::2] = C[..., N:]
    return out


def from_interleaved(C):
    """(K, 2N) columns (re0, im0, re1, ...) -> [Re | Im]."""
    C = np.asarray(C, dtype=np.float64)
    return np.concatenate([C[..., 0::2], C[..., 1::2]], axis=-1)


def lloyd_device(X, centers_init, tol_abs, max_iter, x_mean=None, want_resp=False, device=0):
    """One Lloyd run on the device (``qce_kmeans_lloyd``).

    X: (B, N) complex128 NumPy array (uploaded) or tensor on ``device`` (used in place).  centers_init (K, 2N)
    and x_mean (2N,) or None are in the interleaved column order and centers_init is centred.  Returns a dict:
    labels (B,) int64, centers (K, 2N) centred and interleaved, inertia, n_iter, strict, relocated, and resp -- the
    one-hot (B, K) float64 responsibilities as a device tensor when want_resp."""
    import torch
    dev = torch.device("cuda", int(device))
    if not _is_tensor(X):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.complex128)).to(dev)
    elif X.device != dev or X.dtype != torch.complex128:
        raise ValueError(f"X must be a complex128 tensor on {dev}")
    X = X.contiguous()
    if X.dim() != 2:
        raise ValueError("X must be (n_samples, n_features)")
    B, N = X.shape
    C0 = np.ascontiguousarray(centers_init, dtype=np.float64)
    if C0.ndim != 2 or C0.shape[1] != 2 * N:
        raise ValueError(f"centers_init must be (n_clusters, {2 * N})")
    K = C0.shape[0]
    mean = None if x_mean is None else np.ascontiguousarray(x_mean, dtype=np.float64).reshape(2 * N)
    centers = np.empty((K, 2 * N))
    info = np.empty(4)
    labels = torch.empty(B, dtype=torch.int64, device=dev)
    resp = torch.empty((B, K), dtype=torch.float64, device=dev) if want_resp else None
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.load().qce_kmeans_lloyd(_lib.ptr(X), B, N, K, _lib.ptr(mean), _lib.ptr(C0), int(max_iter),
                                            float(tol_abs), _lib.ptr(centers), _lib.ptr(labels), _lib.ptr(resp),
                                            _lib.ptr(info), int(device), _lib.IO_DEVICE, stream.cuda_stream))
    return dict(labels=labels.cpu().numpy(), centers=centers, inertia=float(info[1]), n_iter=int(info[0]),
                strict=bool(info[2]), relocated=int(info[3]), resp=resp)


def predraw(random_state, B, K, n_local_trials=None):
    """Every random number ``sklearn.cluster.kmeans_plusplus(X (B rows), K, random_state=...)`` draws, in its order:
    ``(first, U)`` with ``first`` the row of the first centre and ``U`` (K - 1, T) the uniforms of the further
    centres, T = 2 + int(log K) unless given.  None of the draws depends on the data, so ``random_state`` is left in
    the state ``kmeans_plusplus`` leaves it in.

    Pinned to ``_kmeans_plusplus`` of the installed scikit-learn 1.7.2: one ``choice(B, p=ones / B)``, then
    ``uniform(size=T)`` once per further centre (tests/test_kmeans_seed_ref.py compares the states)."""
    B, K = int(B), int(K)
    T = 2 + int(np.log(K)) if n_local_trials is None else int(n_local_trials)
    first = int(random_state.choice(B, p=np.full(B, 1.0 / B)))
    U = np.empty((K - 1, T))
    for c in range(K - 1):
        U[c] = random_state.uniform(size=T)
    return first, U


def seed_device(X, K, first, U, x_mean=None, device=0, want_debug=False):
    """k-means++ seeds chosen on the device from pre-drawn uniforms (``qce_kmeans_seed``).

    X: (B, N) complex128 NumPy array (uploaded) or tensor on ``device`` (used in place); ``first`` and ``U`` (K - 1, T)
    from ``predraw``; x_mean (2N,) interleaved or None.  Returns (centers (K, 2N) centred and interleaved, indices (K,)
    int64), and with want_debug also (candidates (K - 1, T) int64, potentials (K,))."""
    import torch
    dev = torch.device("cuda", int(device))
    if not _is_tensor(X):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.complex128)).to(dev)
    elif X.device != dev or X.dtype != torch.complex128:
        raise ValueError(f"X must be a complex128 tensor on {dev}")
    X = X.contiguous()
    if X.dim() != 2:
        raise ValueError("X must be (n_samples, n_features)")
    B, N = X.shape
    K = int(K)
    U = np.ascontiguousarray(U, dtype=np.float64)
    if U.ndim != 2 or U.shape[0] != max(K - 1, 0) or U.shape[1] < 1:
        raise ValueError(f"U must be ({K - 1}, n_trials)")
    T = U.shape[1]
    mean = None if x_mean is None else np.ascontiguousarray(x_mean, dtype=np.float64).reshape(2 * N)
    centers = np.empty((max(K, 0), 2 * N))
    indices = np.empty(max(K, 0), dtype=np.int64)
    cand = np.empty((max(K - 1, 0), T), dtype=np.int64) if want_debug else None
    pot = np.empty(max(K, 0)) if want_debug else None
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.load().qce_kmeans_seed(_lib.ptr(X), B, N, K, _lib.ptr(mean), int(first),
                                           _lib.ptr(U) if K > 1 else None, T, _lib.ptr(indices), _lib.ptr(centers),
                                           _lib.ptr(cand), _lib.ptr(pot), int(device), _lib.IO_DEVICE,
                                           stream.cuda_stream))
    return (centers, indices, cand, pot) if want_debug else (centers, indices)


def _same_clustering(a, b, K):
    """sklearn's _is_same_clustering: equal up to a permutation of the labels."""
    mapping = np.full(K, -1, dtype=np.int64)
    for x, y in zip(a, b):
        if mapping[x] == -1:
            mapping[x] = y
        elif mapping[x] != y:
            return False
    return True


class DeviceKMeans:
    """``sklearn.cluster.KMeans`` for complex rows with the Lloyd loop on the device.

    fit(X): X (B, N) complex NumPy array, or a complex128 tensor already resident on ``device`` (not uploaded
    again).  Sets ``labels_``, ``cluster_centers_`` ((K, 2N) in sklearn's ``[Re | Im]`` order, mean added back),
    ``inertia_`` and ``n_iter_``.  init: "k-means++", "random" or a (K, 2N) array in sklearn's column order.
    seeding: "host" (``sklearn.cluster.kmeans_plusplus``, the default) or "device": with init="k-means++" the random
    numbers are drawn in advance (``predraw``) and the seeds are chosen on the device (``seed_device``), once per
    ``n_init`` run; any other init ignores it.
    ``_lloyd``: a callable (X_centred (B, 2N), centers_init (K, 2N), tol_abs, max_iter) -> (labels, centers, inertia,
    n_iter, ...) in sklearn's column order that stands in for the device loop (CPU tests).  ``_seed``: a callable
    (X_centred (B, 2N), K, first, U) -> (indices, ...) that stands in for the device seeding (CPU tests)."""

    def __init__(self, n_clusters, init="k-means++", n_init=1, max_iter=300, tol=1e-4, random_state=None, device=0,
                 seeding="host", _lloyd=None, _seed=None):
        if seeding not in ("host", "device"):
            raise ValueError(f"seeding must be 'host' or 'device', not {seeding!r}")
        self.seeding = seeding
        self._seed = _seed
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.random_state = random_state
        self.device = device
        self._lloyd = _lloyd
        self.resp_ = None

    def fit(self, X):
        return self._fit(X)

    def _fit(self, X, host=None, want_resp=False):
        """host: the NumPy copy of a device-resident X, when the caller still has it (saves the download the seeding
        would need); want_resp: keep the best run's one-hot responsibilities on the device (``resp_``)."""
        from sklearn.utils import check_random_state
        K = self.n_clusters
        Xd = X if _is_tensor(X) else None
        Xh = np.asarray(X if Xd is None else (Xd.cpu().numpy() if host is None else host))
        if Xh.ndim != 2:
            raise ValueError("X must be (n_samples, n_features)")
        B, N = Xh.shape
        if B < K:
            raise ValueError(f"n_samples={B} should be >= n_clusters={K}.")
        if K < 1 or self.n_init < 1 or self.max_iter < 1:
            raise ValueError("n_clusters, n_init and max_iter must be positive")
        # the host part of KMeans.fit: the real view, the tolerance from the uncentred columns, the centred data
        Xc = np.concatenate([Xh.real, Xh.imag], axis=1).astype(np.float64, copy=False)  # ut.cplx2real(X, axis=1)
        tol_abs = float(np.mean(np.var(Xc, axis=0)) * self.tol)
        rs = check_random_state(self.random_state)
        init = self.init
        init_is_array = not isinstance(init, str)
        if init_is_array:
            init = np.array(init, dtype=np.float64, copy=True, order="C")
            if init.shape != (K, 2 * N):
                raise ValueError(f"The shape of the initial centers {init.shape} does not match the number of "
                                 f"clusters {K} and features {2 * N}.")
        elif init not in ("k-means++", "random"):
            raise ValueError(f"init must be 'k-means++', 'random' or an array, not {init!r}")
        mean = Xc.mean(axis=0)
        Xc -= mean
        if init_is_array:
            init -= mean
        seed_on_device = self.seeding == "device" and not init_is_array and init == "k-means++"
        if self._lloyd is None or (seed_on_device and self._seed is None):
            if Xd is None:
                import torch
                Xd = torch.from_numpy(np.ascontiguousarray(Xh, dtype=np.complex128)).to(
                    torch.device("cuda", int(self.device)))
            mean_il = to_interleaved(mean)
        best = None
        for _ in range(self.n_init):
            if init_is_array:
                C0 = init
            elif seed_on_device:
                first, U = predraw(rs, B, K)  # the stream moves on as kmeans_plusplus would move it
                if self._seed is not None:
                    C0 = Xc[np.asarray(self._seed(Xc, K, first, U)[0])]
                else:
                    C0 = from_interleaved(seed_device(Xd, K, first, U, x_mean=mean_il, device=self.device)[0])
            elif init == "k-means++":
                from sklearn.cluster import kmeans_plusplus
                C0, _idx = kmeans_plusplus(Xc, K, random_state=rs)
            else:
                C0 = Xc[rs.choice(B, size=K, replace=False, p=np.full(B, 1.0 / B))]
            if self._lloyd is not None:
                labels, centers, inertia, n_iter = self._lloyd(Xc, np.array(C0, copy=True), tol_abs, self.max_iter)[:4]
                resp = None
            else:
                r = lloyd_device(Xd, to_interleaved(C0), tol_abs, self.max_iter, x_mean=mean_il, want_resp=want_resp,
                                 device=self.device)
                labels, centers, inertia, n_iter = r["labels"], from_interleaved(r["centers"]), r["inertia"], \
                    r["n_iter"]
                resp = r["resp"]
            if best is None or (inertia < best[2] and not _same_clustering(labels, best[0], K)):
                best = (labels, centers, inertia, n_iter, resp)
        labels, centers, inertia, n_iter, resp = best
        if len(set(labels.tolist())) < K:
            import warnings
            from sklearn.exceptions import ConvergenceWarning
            warnings.warn("Number of distinct clusters ({}) found smaller than n_clusters ({}). Possibly due to "
                          "duplicate points in X.".format(len(set(labels.tolist())), K), ConvergenceWarning,
                          stacklevel=2)
        self.labels_ = np.asarray(labels)
        self.cluster_centers_ = np.asarray(centers) + mean
        self.inertia_ = float(inertia)
        self.n_iter_ = int(n_iter)
        self.resp_ = resp
        return self
