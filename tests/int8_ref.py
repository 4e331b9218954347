"""NumPy restatement of the int8-slice ('int8' precision) estimate: the contract k_pack_i8 / k_est_all_i8 implement.

Per component k, with the real embeddings of tests/fast_ref.py (``embed_matrix`` / ``embed_vec``), tables padded to
(2 MP, 2 MP) and (2 NP, 2 MP):

1. digits: for every row r of E(Linv_k) and E(W_k), e_r = frexp exponent of the row's largest magnitude (0 for a zero
   row), q = rint(T[r, :] 2^(7S-1-e_r)) (half to even), q in balanced base 128, digits in [-64, 63], least significant
   first, the final carry folded into the top digit (<= 64).
2. observations: t = y y_scale, ti = rint(t); a sample is on the grid when every |t - ti| <= 2^-20 and |ti| <= 127.
3. products: acc_s = D_s ti in integers (int64 here, int32 on the device), raw = sum_s 128^s acc_s in float64,
   u = raw_L 2^(e_r-7S+1) / y_scale - q0,  z = raw_W 2^(e_r-7S+1) / y_scale + b.
4. lp_k = c_k - sum u^2, softmax over k, h = sum_k p_k z_k / sum_k p_k, all float64.  Off-grid rows are NaN.

``model`` takes the tables from the FP64 oracle (``tables=None``) or as arrays (``tables=dict(P=, means_y=, W=, b=
[, cconst=])``, e.g. ``DeviceModel.tables()``).  ``drop_plane`` is the mutation switch: the least significant digit
plane is dropped.
"""
import numpy as np

from fast_ref import embed_matrix, embed_vec, errors, inputs, oracle, padded_shape, y_scale_of
from oracle import qce_oracle as O

GRID_TOL = 2.0 ** -20


def digit_planes(T, S):
    """(D (S, rows, cols) int64, least significant plane first; e (rows,) int) of a real table T."""
    T = np.asarray(T, np.float64)
    mx = np.max(np.abs(T), axis=1)
    e = np.where(mx > 0, np.frexp(mx)[1], 0).astype(np.int64)
    q = np.rint(np.ldexp(T, (7 * S - 1 - e)[:, None].astype(np.int32))).astype(np.int64)
    D = np.empty((S,) + T.shape, np.int64)
    for s in range(S):
        d = ((q + 64) & 127) - 64
        q = (q - d) >> 7
        if s == S - 1:
            d = d + 128 * q
        D[s] = d
    return D, e


def _pad(E, rows, cols):
    T = np.zeros((rows, cols))
    T[:E.shape[0], :E.shape[1]] = E
    return T


def raw_products(T, ti, S, drop_plane=False):
    """raw (B, rows) float64 = sum_s 128^s (D_s ti), the row exponents, max |digit| and max |acc|."""
    D, e = digit_planes(T, S)
    if drop_plane:
        D[0] = 0
    raw = np.zeros((ti.shape[0], T.shape[0]))
    max_acc = 0
    for s in range(S - 1, -1, -1):
        acc = ti @ D[s].T  # int64, exact
        max_acc = max(max_acc, int(np.max(np.abs(acc))))
        raw += acc.astype(np.float64) * 128.0 ** s
    return raw, e, int(np.max(np.abs(D))), max_acc


def grid(c, y):
    """(ti (B, 2 MP) int64, on_grid (B,) bool) of the observations of case c."""
    MP, _ = padded_shape(c.M, c.N)
    t = np.zeros((y.shape[0], 2 * MP))
    t[:, :2 * c.M] = embed_vec(y) * y_scale_of(c)
    ti = np.rint(t)
    ok = np.all((np.abs(t - ti) <= GRID_TOL) & (np.abs(ti) <= 127), axis=1)
    return np.where(ok[:, None], ti, 0).astype(np.int64), ok


def model(c, S, tables=None, drop_plane=False, y=None, with_oracle=True):
    """h (B, N) complex128 of the contract at S planes, the per-component raw sums and exponents, the largest digit
    and int accumulator met, and (with_oracle) the oracle's h with the model's errors against it."""
    d = inputs(c)
    y = d["y"] if y is None else y
    ho = None
    if tables is None or with_oracle:
        ho, t_or = oracle(c)
    t = t_or if tables is None else tables
    K, M, N = c.K, c.M, c.N
    MP, NP = padded_shape(M, N)
    ys = y_scale_of(c)
    Linv = np.conj(np.transpose(t["P"], (0, 2, 1)))
    q0 = np.einsum("kij,kj->ki", Linv, t["means_y"])
    cconst = t.get("cconst")
    if cconst is None:
        cconst = -M * np.log(np.pi) + 2 * np.real(O.log_det_cholesky(t["P"])) + np.log(d["w"])
    ti, ok = grid(c, y)
    B = y.shape[0]
    lp = np.empty((B, K))
    z = np.empty((K, B, 2 * NP))
    rawL, rawW, exps = [], [], []
    max_digit = max_acc = 0
    for k in range(K):
        rl, el, dl, al = raw_products(_pad(embed_matrix(Linv[k]), 2 * MP, 2 * MP), ti, S, drop_plane)
        rw, ew, dw, aw = raw_products(_pad(embed_matrix(t["W"][k]), 2 * NP, 2 * MP), ti, S, drop_plane)
        max_digit, max_acc = max(max_digit, dl, dw), max(max_acc, al, aw)
        u = rl * np.ldexp(1.0, (el - 7 * S + 1).astype(np.int32))[None, :] / ys - _pad(embed_vec(q0[k])[None, :], 1, 2 * MP)
        z[k] = rw * np.ldexp(1.0, (ew - 7 * S + 1).astype(np.int32))[None, :] / ys + _pad(embed_vec(t["b"][k])[None, :], 1, 2 * NP)
        lp[:, k] = cconst[k] - np.sum(u * u, axis=1)
        rawL.append(rl)
        rawW.append(rw)
        exps.append(np.concatenate([el, ew]))
    p = np.exp(lp - np.max(lp, axis=1, keepdims=True))
    out = np.einsum("bk,kbr->br", p, z) / np.sum(p, axis=1)[:, None]
    h = out[:, 0:2 * N:2] + 1j * out[:, 1:2 * N:2]
    h[~ok] = np.nan
    res = dict(h=h, on_grid=ok, raw_L=np.array(rawL), raw_W=np.array(rawW), exps=np.array(exps), max_digit=max_digit,
               max_acc=max_acc, oracle=ho)
    if ho is not None and np.all(ok):
        res.update(errors(h, ho, "e"))
    return res
