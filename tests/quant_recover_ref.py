"""A NumPy restatement of the two kernels of csrc/qce_quant_recover.hip and the inputs of their tests.

``variance_fit_ref``: the scalar Gauss-Newton variance fit of one (component, dimension) as the kernel runs it
(``_em_quant.cov_from_quant`` / ``gauss_newt_solve`` with the one-column least squares written out; a restart branch
or a non-finite value stops the fit with status 1).  ``eig_clip_ref``: the parallel cyclic two-sided Jacobi iteration
of the Hermitian eigenvalue clip, step by step in the kernel's order (round-robin pairs, rotations from the current
2 x 2 blocks, columns of A and V, rows of A; the off-diagonal norm summed from the entries themselves).
"""
import math

import numpy as np
from scipy.special import erf

TOL, MAXITS = 1e-5, 100
OFF_TOL, MAX_SWEEPS = 1e-14, 30


def symmetric(pos):
    """The quantiser's full threshold vector (-t_T ... 0 ... t_T) of the positive thresholds `pos`."""
    pos = np.asarray(pos, dtype=float)
    return np.concatenate([-pos[::-1], [0.0], pos])


# ---- variance fits -------------------------------------------------------------------------------------------
def variance_fit_ref(p, nk, pos, x0):
    """p (T, 2), the T positive thresholds, the start value -> (s2, status, iters)."""
    lo, hi = 1 / nk, (nk - 1) / nk
    p = np.where(p < lo, lo, p)
    p = np.where(p > hi, hi, p)
    p = np.concatenate([p[:, 0], p[:, 1]])
    t = np.concatenate([pos, pos])
    dx, s, i = 1.0, float(x0), 0
    while i < MAXITS and abs(dx) > TOL:
        if abs(s) < 0.1 or abs(s) > 10.0:
            return 1.0, 1, i
        f = erf(t / (math.sqrt(2) * s)) - p
        J = -math.sqrt(2 / math.pi) * t * np.exp(-t ** 2 / (2 * s)) / s ** 2
        jj, jf = 0.0, 0.0
        for a, b in zip(J, f):
            jj += a * a
            jf += a * b
        dx = 0.0 if jj == 0.0 else -jf / jj
        s += dx
        i += 1
        if not (math.isfinite(dx) and math.isfinite(s)):
            return 1.0, 1, i
    v = s * s
    return max(2 * v, 0.0), 0, i


def variance_fits_ref(probs, nk, pos, x0):
    K, D = probs.shape[:2]
    s2, st, it = np.empty((K, D)), np.zeros((K, D), np.int32), np.zeros((K, D), np.int32)
    for k in range(K):
        for d in range(D):
            s2[k, d], st[k, d], it[k, d] = variance_fit_ref(probs[k, d], nk[k], pos, x0[k, d])
    return s2, st, it


def fit_case(T, seed=0, K=3, D=16, nk=2000.0, far=()):
    """The variance-fit inputs of the tests: probabilities erf(t / (sqrt 2 sigma)) with sigma drawn from [0.4, 1.3]
    per part plus N(0, 0.01) noise; sigma = 40 in the dimensions `far` (the fit leaves |s| <= 10 there).
    Returns (probs (K, D, T, 2), nk (K,), positive thresholds, x0 (K, D))."""
    rng = np.random.default_rng(100 + seed + T)
    pos = {1: np.array([0.8]), 3: np.array([0.5, 1.0, 1.5])}.get(T)
    if pos is None:
        pos = 0.05 * np.arange(1, T + 1)
    sig = rng.uniform(0.4, 1.3, (K, D, 1, 2))
    for d in far:
        sig[:, d] = 40.0
    probs = erf(pos[None, None, :, None] / (math.sqrt(2) * sig)) + 0.01 * rng.standard_normal((K, D, T, 2))
    return probs, np.full(K, float(nk)), pos, np.ones((K, D))


def corr_case(K=3, D=16, seed=5):
    """Sign correlations (K, D, D) of a plausible size: Hermitian, unit diagonal, |entries| < 1."""
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((K, D, 2 * D)) + 1j * rng.standard_normal((K, D, 2 * D))
    C = L @ L.conj().transpose(0, 2, 1)
    d = np.sqrt(np.real(np.einsum("kii->ki", C)))
    C = C / d[:, :, None] / d[:, None, :]
    return 2 / np.pi * (np.arcsin(np.clip(C.real, -1, 1)) + 1j * np.arcsin(np.clip(C.imag, -1, 1)))


# ---- eigenvalue clip -----------------------------------------------------------------------------------------
def pairs_of_step(n, r):
    """The n / 2 index pairs of step r of the round-robin tournament over n (even) players."""
    out = []
    for i in range(n // 2):
        a, b = (n - 1, r) if i == 0 else ((r + i) % (n - 1), (r - i + n - 1) % (n - 1))
        out.append((min(a, b), max(a, b)))
    return out


def _off2(A):
    """Squared off-diagonal Frobenius norm, summed from the off-diagonal entries themselves."""
    return float(np.sum(np.abs(A - np.diag(np.diag(A))) ** 2))


def eig_clip_ref(C, floor):
    """(V max(L, floor) V^H, status, sweeps) of the Hermitian C (its lower triangle is used, as eigh does)."""
    C = np.asarray(C, dtype=complex)
    D = C.shape[0]
    A = np.tril(C) + np.tril(C, -1).conj().T
    A[np.arange(D), np.arange(D)] = np.real(np.diag(A))
    V = np.eye(D, dtype=complex)
    n = D + (D & 1)
    norm2 = float(np.sum(np.abs(A) ** 2))
    sweeps, status = 0, 0
    while not _off2(A) <= OFF_TOL ** 2 * norm2:
        if sweeps == MAX_SWEEPS:
            status = 1
            break
        for r in range(n - 1):
            rot = []
            for p, q in pairs_of_step(n, r):
                if q >= D:
                    continue
                a, b, c = A[p, p].real, A[q, q].real, A[p, q]
                g = math.hypot(c.real, c.imag)
                if g == 0.0:
                    continue
                tau = (b - a) / (2 * g)
                t = math.copysign(1.0, tau) / (abs(tau) + math.sqrt(1 + tau * tau))
                cs = 1 / math.sqrt(1 + t * t)
                sw = (t * cs) * (c / g)
                rot.append((p, q, cs, sw, a - t * g, b + t * g))
            for p, q, cs, sw, _, _ in rot:  # columns of A and V: X <- X J, J = [[cs, sw], [-conj(sw), cs]]
                for X in (A, V):
                    xp, xq = X[:, p].copy(), X[:, q].copy()
                    X[:, p] = xp * cs - xq * np.conj(sw)
                    X[:, q] = xp * sw + xq * cs
            for p, q, cs, sw, app, aqq in rot:  # rows of A: A <- J^H A
                xp, xq = A[p, :].copy(), A[q, :].copy()
                A[p, :] = cs * xp - sw * xq
                A[q, :] = np.conj(sw) * xp + cs * xq
                A[p, p], A[q, q], A[p, q], A[q, p] = app, aqq, 0.0, 0.0
        sweeps += 1
    w = np.maximum(np.real(np.diag(A)), floor)
    out = (V * w) @ V.conj().T
    out = np.triu(out) + np.triu(out, 1).conj().T
    return out, status, sweeps


def clip_case(D, rank, seed=0):
    """L L^H / rank - 0.1 I with L (D, rank): indefinite, with a degenerate cluster at -0.1 when rank < D."""
    rng = np.random.default_rng(1000 * D + 10 * rank + seed)
    L = rng.standard_normal((D, rank)) + 1j * rng.standard_normal((D, rank))
    return L @ L.conj().T / rank - 0.1 * np.eye(D)


CLIP_SIZES = [1, 7, 8, 63, 64]
CLIP_RANKS = ["full", 5, 3]


def clip_cases():
    """(name, matrix) of every clip input of the tests."""
    out = []
    for D in CLIP_SIZES:
        for r in CLIP_RANKS:
            out.append((f"D{D}_r{r}", clip_case(D, D if r == "full" else min(r, D))))
    return out
