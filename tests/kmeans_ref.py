"""Test data and a NumPy reference of the Lloyd loop of csrc/qce_kmeans.hip (sklearn's _kmeans_single_lloyd on dense
data with unit weights), shared by the k-means tests.

Columns here are in sklearn's [Re | Im] order; Euclidean distances do not depend on the column order.
"""
import functools

import numpy as np

# (B, N, K, spread, seed): B off every tile size; K below, across and far beyond a 16-cluster block; D = 32 ... 512;
# K = 1 and K = B.  The last two reach the remaining kernel paths: D = 400 (two-tile workgroups, which D > 256 takes)
# with enough clusters for the waves to split the cluster blocks, and D = 18, no multiple of 16
CASES = [(1000, 16, 5, 1.0, 11), (1037, 16, 17, 0.7, 12), (2051, 32, 130, 0.6, 13), (777, 64, 33, 0.4, 14),
         (531, 256, 9, 0.2, 15), (4099, 16, 128, 0.7, 16), (300, 16, 1, 1.0, 17), (64, 16, 64, 1.0, 18),
         (300, 200, 40, 0.3, 19), (500, 9, 20, 1.0, 20)]
# the cases run again with a stop that is not strict: (index into CASES, KMeans keywords)
NONSTRICT = [(1, dict(max_iter=2)), (2, dict(max_iter=2)), (1, dict(tol=0.05)), (2, dict(tol=0.05))]
EMPTY_CASE = (600, 16, 4, 2.0, 3)


def case(B, N, K, spread, seed):
    """(B, N) complex rows around K complex centres."""
    rng = np.random.default_rng(seed)
    centres = spread * (rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    pick = rng.integers(0, K, B)
    return centres[pick] + (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))) / np.sqrt(2)


def real_view(X):
    return np.concatenate([X.real, X.imag], axis=1)


def centred(X):
    """(X_real, X_centred, mean) as KMeans.fit forms them."""
    Xr = real_view(X)
    mean = Xr.mean(axis=0)
    return Xr, Xr - mean, mean


def empty_case_init(X):
    """The init of the empty-cluster case, uncentred: the first three real-view rows, and a row that is all 50s
    after centring."""
    Xr, _, mean = centred(X)
    return np.concatenate([Xr[:3], (50.0 + mean)[None, :]], axis=0)


def tie_case():
    """Uncentred integer data with exact ties: 600 rows of integers in [-3, 3] (500 drawn, the first 100 repeated) and
    six centres taken from the rows (the first six), centre 3 a copy of centre 1: 124 rows have two equal best
    scores."""
    rng = np.random.default_rng(0)
    X = rng.integers(-3, 4, (500, 32)).astype(np.float64)
    X = np.concatenate([X, X[:100]], axis=0)
    C = X[:6].copy()
    C[3] = C[1]
    return X, C


def assign(Xc, C):
    """One assignment step: (labels, relative margins (second-best - best score) / (|x|^2 + |c|^2), scores).  Scores
    are the expanded form |c|^2 - 2 x.c; argmin takes the lowest index among equal scores."""
    cn = np.einsum("kd,kd->k", C, C)
    S = cn[None, :] - 2.0 * (Xc @ C.T)
    labels = np.argmin(S, axis=1)
    if C.shape[0] == 1:
        return labels, np.full(Xc.shape[0], np.inf), S
    part = np.partition(S, 1, axis=1)
    xn = np.einsum("bd,bd->b", Xc, Xc)
    margins = (part[:, 1] - part[:, 0]) / (xn + cn[labels])
    return labels, margins, S


def relocation_rows(dist, n_empty):
    """The n_empty rows farthest from their centres, in descending distance (equal distances: the lower row first)."""
    order = np.lexsort((np.arange(dist.shape[0]), -dist))
    return order[:n_empty]


def lloyd_ref(Xc, C0, tol_abs, max_iter):
    """-> (labels, centres, inertia, n_iter, info); info: margin (the smallest relative margin over all assignments),
    strict, relocated."""
    B, _ = Xc.shape
    K = C0.shape[0]
    C = np.array(C0, dtype=np.float64, copy=True)
    labels_old = np.full(B, -1)
    labels = labels_old
    margin, strict, relocated, n_iter = np.inf, False, 0, 0
    for it in range(max_iter):
        labels, m, _ = assign(Xc, C)
        margin = min(margin, float(m.min()))
        sums = np.zeros_like(C)
        np.add.at(sums, labels, Xc)
        counts = np.bincount(labels, minlength=K).astype(np.float64)
        empty = np.flatnonzero(counts == 0)
        if empty.size:  # _relocate_empty_clusters_dense
            dist = ((Xc - C[labels]) ** 2).sum(axis=1)
            for k_new, far in zip(empty, relocation_rows(dist, empty.size)):
                k_old = labels[far]
                sums[k_old] -= Xc[far]
                sums[k_new] = Xc[far]
                counts[k_new] = 1.0
                counts[k_old] -= 1.0
            relocated += int(empty.size)
        C_new = np.where(counts[:, None] > 0, sums / np.where(counts > 0, counts, 1.0)[:, None], sums)
        shift = float(((C_new - C) ** 2).sum())
        C = C_new
        n_iter = it + 1
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol_abs:
            break
        labels_old = labels
    if not strict:
        labels, m, _ = assign(Xc, C)
        margin = min(margin, float(m.min()))
    inertia = float(((Xc - C[labels]) ** 2).sum())
    return labels, C, inertia, n_iter, dict(margin=margin, strict=strict, relocated=relocated)


ALL_NAMES = [f"case{i}" for i in range(len(CASES))] + [f"nonstrict{i}" for i in range(len(NONSTRICT))] + ["empty"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """sklearn's result for one named case, computed once per session and shared: a dict with X, K, seed, init (an
    uncentred array or None), kw (KMeans keywords), km (the fitted KMeans) and rs_state (the state its RandomState was
    left in)."""
    init, kw = None, {}
    if name == "empty":
        B, N, K, spread, seed = EMPTY_CASE
        X = case(B, N, K, spread, seed)
        init = empty_case_init(X)
    else:
        if name.startswith("nonstrict"):
            i, kw = NONSTRICT[int(name[len("nonstrict"):])]
        else:
            i = int(name[len("case"):])
        B, N, K, spread, seed = CASES[i]
        X = case(B, N, K, spread, seed)
    km, rs = sklearn_fit(X, K, seed, init, **kw)
    return dict(X=X, K=K, seed=seed, init=init, kw=kw, km=km, rs_state=rs.get_state())


def sklearn_fit(X, K, seed=None, init=None, **kw):
    """KMeans on the real view; init: an uncentred (K, 2N) array, else k-means++ from RandomState(seed).  Returns
    (km, random state)."""
    from sklearn.cluster import KMeans
    rs = np.random.RandomState(seed)
    km = KMeans(n_clusters=K, n_init=1, random_state=rs, **({} if init is None else {"init": init}), **kw)
    km.fit(real_view(X))
    return km, rs
