"""Float64 NumPy restatement of the VAE training loss (reference estimators/vae.py:312-365 ``vae_loss`` with
zeromean=True) and of its gradients: the oracle of tests/test_vae_train.py.

It works on whole (B, N) arrays with np.sum / np.mean and a Python loop over the quantiser's levels, so it shares no
code and no summation order with the kernel (csrc/qce_vae_train.hip).  The one thing that follows the reference to the
bit rather than the textbook is the float32 constant delta / sqrt(pi) of ``get_Bussgang_matrix_diag_fast``
(uniform_quantizer.py:110), the ``k2`` of tests/vae_ref.py.

``enc`` (B, 2L) = [mu | s], ``dec`` (B, N) = log_var_dec, ``t`` (T, 2N) = [re | im]; row b uses target row and SNR entry
``index[b]`` (or b).  The loss is ``-mean_b rows``.
"""
import numpy as np

from vae_ref import MAX_UNIFORM_STEP, k2_of


def _gather(enc, dec, t, snr_db, index):
    enc = np.asarray(enc, dtype=np.float64)
    dec = np.asarray(dec, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    if index is not None:
        ix = np.asarray(index).astype(np.int64)
        t = t[ix]
        snr_db = None if snr_db is None else np.asarray(snr_db, dtype=np.float64)[ix]
    else:
        t = t[:enc.shape[0]]
        snr_db = None if snr_db is None else np.asarray(snr_db, dtype=np.float64)[:enc.shape[0]]
    N = dec.shape[1]
    return enc, dec, t[:, :N] ** 2 + t[:, N:] ** 2, snr_db


def _real_terms(dec, a, snr_db, n_bits):
    """(row term, d row term / d dec) of the 'real' mode."""
    N = dec.shape[1]
    s2 = 10 ** (-snr_db / 10)
    ev = np.exp(-dec)
    c = ev + s2[:, None]
    cbar = np.mean(c, axis=1)
    if np.isinf(n_bits):
        beta, dbeta = np.ones_like(cbar), np.zeros_like(cbar)
        cp = c
    else:
        nb = int(n_bits)
        delta = np.sqrt((1 + s2) / 2) * MAX_UNIFORM_STEP[nb]
        k2 = np.array([k2_of(d) for d in delta])
        S, S2 = np.zeros_like(cbar), np.zeros_like(cbar)
        for i in range(1, 2 ** nb):
            w = delta ** 2 * (i - 2 ** (nb - 1)) ** 2 / cbar
            S += np.exp(-w)
            S2 += np.exp(-w) * w / cbar
        g = k2 / np.sqrt(cbar) * S
        dg = -g / (2 * cbar) + k2 / np.sqrt(cbar) * S2
        beta = np.clip(g ** 2, 0, 1)
        dbeta = np.where(g ** 2 <= 1, 2 * g * dg, 0.0)
        cp = beta[:, None] * c + (1 - beta)[:, None] * cbar[:, None]
    term = np.sum(-np.log(cp) - a / cp, axis=1)
    q = -1 / cp + a / cp ** 2
    dc = beta[:, None] * q + ((1 - beta) * np.sum(q, axis=1) + dbeta * np.sum(q * (c - cbar[:, None]), axis=1))[:, None] / N
    return term, -dc * ev


def elbo_rows(enc, dec, t, mode, n_bits=1, snr_db=None, index=None):
    """Row ELBOs (B,) float64."""
    enc, dec, a, snr_db = _gather(enc, dec, t, snr_db, index)
    L = enc.shape[1] // 2
    mu, s = enc[:, :L], enc[:, L:]
    kl = np.sum(s, axis=1) - 0.5 * np.sum(mu ** 2, axis=1) - 0.5 * np.sum(np.exp(2 * s), axis=1)
    if mode == "real":
        return _real_terms(dec, a, snr_db, n_bits)[0] + kl
    return np.sum(dec, axis=1) - np.sum(np.exp(dec) * a, axis=1) + kl


def loss(enc, dec, t, mode, n_bits=1, snr_db=None, index=None):
    return -float(np.mean(elbo_rows(enc, dec, t, mode, n_bits, snr_db, index)))


def loss_grads(enc, dec, t, mode, n_bits=1, snr_db=None, index=None):
    """(d loss / d enc (B, 2L) -- the KL part only, dec held fixed --, d loss / d dec (B, N)), float64."""
    enc, dec, a, snr_db = _gather(enc, dec, t, snr_db, index)
    B, L = enc.shape[0], enc.shape[1] // 2
    mu, s = enc[:, :L], enc[:, L:]
    g_enc = np.concatenate([mu, -(1 - np.exp(2 * s))], axis=1) / B
    if mode == "real":
        g_dec = -_real_terms(dec, a, snr_db, n_bits)[1] / B
    else:
        g_dec = -(1 - np.exp(dec) * a) / B
    return g_enc, g_dec


def reparameterize(enc, eps):
    """(z, d z / d enc applied to g_z as a function) in float64: z = mu + exp(s) eps."""
    enc = np.asarray(enc, dtype=np.float64)
    L = enc.shape[1] // 2
    return enc[:, :L] + np.exp(enc[:, L:]) * np.asarray(eps, dtype=np.float64)


def reparameterize_bwd(enc, eps, g_z):
    enc = np.asarray(enc, dtype=np.float64)
    L = enc.shape[1] // 2
    g_z = np.asarray(g_z, dtype=np.float64)
    return np.concatenate([g_z, g_z * np.exp(enc[:, L:]) * np.asarray(eps, dtype=np.float64)], axis=1)
