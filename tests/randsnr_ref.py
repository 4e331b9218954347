"""Plain numpy restatement of the reference's random-SNR observations with the draws supplied
(utils.py:254-268: y_b = Q_snr(A h_b + 10^(-snr/20) w_b), snr = snrs[snr_index[b]]) and of the VAE encoder features
made from them (estimators/vae.py:48-52).  Vectorised over rows; test_randsnr.py pins it to tests/golden/randsnr.npz
bit for bit and uses it at the shapes the fixture does not hold."""
import numpy as np


def observe(h, snrs, snr_index, w, A=None, n_bits=1, thr=None, lab=None):
    """(y (B, M) complex128, snr_list (B,) float64).  thr (S, L-1) / lab (S, L): one table per SNR."""
    h = np.asarray(h, dtype=np.complex128)
    sn = np.asarray(snrs)
    idx = np.asarray(snr_index)
    N = h.shape[1]
    Amat = np.eye(N) if A is None else np.asarray(A)
    y = np.matmul(Amat, h[:, :, None])[:, :, 0]
    s = np.array([10 ** (-v / 20) for v in sn], dtype=np.float64)[idx]
    y = y + s[:, None] * np.asarray(w, dtype=np.complex128)
    snr_list = sn.astype(np.float64)[idx]
    if n_bits == np.inf or n_bits == "inf":
        return y, snr_list
    if n_bits == 1:
        return 1 / np.sqrt(2) * (np.sign(y.real) + 1j * np.sign(y.imag)), snr_list
    q = np.empty_like(y)
    for i in range(sn.size):  # per-row tables, one SNR group at a time
        rows = idx == i
        v = y[rows]
        q[rows] = lab[i][np.digitize(v.real, thr[i])] + 1j * lab[i][np.digitize(v.imag, thr[i])]
    return q, snr_list


def features(y, n_antennas, fft_pre=True):
    """float32 (B, P, 2N): rows [Re f | Im f], f = y_b[pN:(p+1)N] or its unitary DFT (numpy fft, as vae.py:48-52)."""
    N = int(n_antennas)
    r = np.reshape(np.asarray(y), (-1, N, y.shape[1] // N), "F")
    r = np.transpose(r, [0, 2, 1])
    if fft_pre:
        r = np.fft.fft(r, axis=-1) / np.sqrt(r.shape[-1])
    return np.concatenate([r.real, r.imag], axis=-1).astype(np.float32)


def features_f64(y, n_antennas, fft_pre=True):
    """The same before the float32 rounding (the reference value of the tests' error bound)."""
    N = int(n_antennas)
    r = np.asarray(y).reshape(y.shape[0], y.shape[1] // N, N)
    if fft_pre:
        r = np.fft.fft(r, axis=-1) / np.sqrt(N)
    return np.concatenate([r.real, r.imag], axis=-1)
