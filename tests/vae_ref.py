"""Dense NumPy restatement of the VAE-parameterised Bussgang LMMSE (reference estimators/vae.py:376-431
``convert_dec_outputs`` with zeromean=True, and :368-369 ``lmmse``): the oracle of tests/test_vae.py.

It builds Ch, Cy and Cr as matrices and inverts Cr with np.linalg.inv, so it shares no arithmetic with the
spectral kernel (csrc/qce_vae.hip).  Two things follow the reference to the bit rather than the textbook:

  * the constants sqrt(2/pi), 2/pi and delta/sqrt(pi) are float32 values (the reference builds them from
    ``torch.tensor(np.pi)``, a float32 tensor);
  * the 1-bit diagonal of Cr is k3 * asin(1) exactly.  The reference computes asin of a product that rounds to 1
    or to 1 - ulp, which puts ~9.5e-9 of noise on single diagonal entries; that noise is the reference's own and
    is what the 1-bit tolerance of the tests is built around.
"""
import numpy as np

K1 = float(np.sqrt(np.float32(2) / np.float32(np.pi), dtype=np.float32))
K3 = float(np.float32(2) / np.float32(np.pi))
MAX_UNIFORM_STEP = {1: 1.596, 2: 0.9957, 3: 0.5860, 4: 0.3352, 5: 0.1881, 6: 0.1041, 7: 0.0569, 8: 0.0308}


def uniform_step(snr_db, n_bits):
    base = MAX_UNIFORM_STEP[n_bits] if n_bits <= 8 else 4 * np.sqrt(n_bits) * 2.0 ** (-n_bits)
    return np.sqrt((1 + 10 ** (-snr_db / 10)) / 2) * base


def k2_of(delta):
    return float(np.float32(delta) / np.sqrt(np.float32(np.pi), dtype=np.float32))


def bussgang_gain(d, snr_db, n_bits):
    """Diagonal Bussgang gain for the diagonal d of Cy (uniform_quantizer.py:75-87, float32 constants)."""
    d = np.asarray(d, dtype=np.float64)
    if np.isinf(n_bits):
        return np.ones_like(d)
    if n_bits == 1:
        return K1 / np.sqrt(d)
    delta = uniform_step(snr_db, int(n_bits))
    s = np.zeros_like(d)
    for i in range(1, 2 ** int(n_bits)):
        s += np.exp(-delta ** 2 * (i - 2 ** int(n_bits) / 2) ** 2 / d)
    return k2_of(delta) / np.sqrt(d) * s


def matrices(log_var_row, snr_db, A, n_bits):
    """(Ch, Cy, Cr, A_eff) of one sample."""
    lv = np.asarray(log_var_row, dtype=np.float64)
    N = lv.size
    F = np.fft.fft(np.eye(N)) / np.sqrt(N)
    c = np.maximum(np.exp(-lv), 1e-12)
    Ch = F.conj().T @ np.diag(c).astype(complex) @ F
    A = np.eye(N, dtype=complex) if A is None else np.asarray(A, dtype=complex)
    M = A.shape[0]
    Cy = A @ Ch @ A.conj().T + 10 ** (-snr_db / 10) * np.eye(M)
    d = np.real(np.diag(Cy))
    g = bussgang_gain(d, snr_db, n_bits)
    A_eff = g[:, None] * A
    if np.isinf(n_bits):
        Cr = Cy
    elif n_bits == 1:
        psi = 1 / np.sqrt(d)
        re = np.clip(psi[:, None] * Cy.real * psi[None, :], -1, 1)
        im = np.clip(psi[:, None] * Cy.imag * psi[None, :], -1, 1)
        Cr = K3 * (np.arcsin(re) + 1j * np.arcsin(im))
        Cr[np.arange(M), np.arange(M)] = K3 * np.arcsin(1.0)
    else:
        beta = np.clip(np.mean(g), 0, 1)
        Cr = beta ** 2 * Cy + (1 - beta ** 2) * np.diag(np.diag(Cy))
    return Ch, Cy, Cr, A_eff


def lmmse_from_decoder(y, log_var, snr_db, A=None, n_bits=1, return_lam_min=False):
    """h_b = Ch_b A_eff_b^H Cr_b^-1 y_b for y (B, M) complex and log_var (B, N)."""
    y = np.asarray(y, dtype=complex)
    B, N = np.asarray(log_var).shape
    out = np.empty((B, N), dtype=complex)
    lam = np.inf
    for b in range(B):
        Ch, _, Cr, A_eff = matrices(log_var[b], snr_db, A, n_bits)
        out[b] = Ch @ A_eff.conj().T @ (np.linalg.inv(Cr) @ y[b])
        if return_lam_min:
            lam = min(lam, float(np.linalg.eigvalsh((Cr + Cr.conj().T) / 2)[0]))
    return (out, lam) if return_lam_min else out
