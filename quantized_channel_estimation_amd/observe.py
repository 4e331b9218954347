"""Observations on the device: the scripts' ``get_observation_nbit`` / ``quant`` (reference
modules/utils.py:241-251, :189-203) and the MSE reduction of the estimate loop
(Bussgang_GMM.py:289), computed by libqce.so (``qce_observe`` / ``qce_sq_error``, csrc/qce_observe.hip).

Same names, argument order and output shapes as the reference helpers.  Extra keyword arguments:

* ``noise`` — the CN(0, 1) draw to add (numpy array or CUDA tensor of y's shape).  With it, and
  A = None or a pilot matrix kron(x, I), y is bit-identical to the reference's for the same draw.
* ``seed`` / ``offset`` — without ``noise``, the draw is made on the device by a counter-based
  generator (Philox4x32-10, Box-Muller): complex element e of the batch uses counter offset + e, so
  chunked generation reproduces one-shot generation.  The reference's generator (numpy PCG64,
  unseeded, utils.py:13) cannot be reproduced; its statistics are what the tests check.
* ``device`` — the GPU (default 0).

Host numpy inputs return numpy; ``torch.complex128`` CUDA tensors stay on the device (async on the
current torch stream).

``get_observation_nbit_randSNR`` (utils.py:254-318: one SNR per row, per-SNR quantiser tables) and
``encoder_features`` (the VAE's float32 network input, vae.py:46-53) are ``qce_observe_randsnr``
(csrc/qce_observe_rows.hip); see their docstrings.
"""
import numpy as np

from . import _lib

_NOISE_NONE, _NOISE_GIVEN, _NOISE_GEN = 0, 1, 2


def _is_tensor(x):
    return not isinstance(x, np.ndarray) and hasattr(x, "data_ptr")


def _nbits(n_bits):
    if n_bits == "inf" or n_bits == np.inf:
        return np.inf
    return float(n_bits)


def _tables(nb, thresholds, quant_labels):
    if nb == 1.0 or np.isinf(nb):
        return None, None, 0
    if thresholds is None or quant_labels is None:
        raise ValueError("multi-bit quantisation needs thresholds and quant_labels")
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    lab = np.ascontiguousarray(quant_labels, dtype=np.float64).reshape(-1)
    if lab.size != thr.size + 1:
        raise ValueError(f"{thr.size} thresholds need {thr.size + 1} labels, got {lab.size}")
    return thr, lab, lab.size


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _observe(h2, M, A, scale, noise_kind, w2, seed, offset, nb, thr, lab, nlev, device):
    """h2: (B, N) complex; returns (B, M)."""
    B, N = h2.shape
    a = None if A is None else np.ascontiguousarray(A, dtype=np.complex128)
    if _is_tensor(h2):
        import torch
        if h2.dtype != torch.complex128:
            h2 = h2.to(torch.complex128)
        h2 = h2.contiguous()
        y = torch.empty((B, M), dtype=torch.complex128, device=h2.device)
        if w2 is not None:
            w2 = torch.as_tensor(w2, dtype=torch.complex128, device=h2.device).reshape(B, M).contiguous()
        dev = h2.device.index if h2.device.index is not None else 0
        _lib.check(_lib.load().qce_observe(_lib.ptr(h2), B, N, _lib.ptr(a), M, scale, noise_kind, _lib.ptr(w2),
                                           seed, offset, nb, _lib.ptr(thr), _lib.ptr(lab), nlev, _lib.ptr(y),
                                           dev, _lib.IO_DEVICE, _stream(h2)))
        return y
    h2 = np.ascontiguousarray(h2, dtype=np.complex128)
    if w2 is not None:
        w2 = np.ascontiguousarray(np.asarray(w2, dtype=np.complex128).reshape(B, M))
    y = np.empty((B, M), dtype=np.complex128)
    _lib.check(_lib.load().qce_observe(_lib.ptr(h2), B, N, _lib.ptr(a), M, scale, noise_kind, _lib.ptr(w2), seed,
                                       offset, nb, _lib.ptr(thr), _lib.ptr(lab), nlev, _lib.ptr(y), int(device),
                                       _lib.IO_HOST, None))
    return y


def _squeeze_like_reference(y_full, h_shape):
    """np.squeeze(matmul(A, h[..., None])) then re-insert axis 1 when h.shape[1] == 1 (utils.py:244-246)."""
    if _is_tensor(y_full):
        y = y_full.squeeze()
        if len(h_shape) > 1 and h_shape[1] == 1:
            y = y.unsqueeze(1)
        return y
    y = np.squeeze(y_full)
    if len(h_shape) > 1 and h_shape[1] == 1:
        y = np.expand_dims(y, 1)
    return y


def get_observation_nbit(h, snr, A=None, n_bits=1, thresholds=None, cluster=None, agc=False, *, noise=None,
                         seed=0, offset=0, device=0):
    """y = Q(A h + 10^(-snr/20) n), n ~ CN(0, I) (utils.py:241-251).  ``agc`` is accepted and unused,
    as in the reference."""
    del agc
    nb = _nbits(n_bits)
    thr, lab, nlev = _tables(nb, thresholds, cluster)
    shape = tuple(h.shape)
    N = shape[-1]
    if A is not None and np.asarray(A).shape[1] != N:
        raise ValueError(f"A must have {N} columns")
    M = N if A is None else np.asarray(A).shape[0]
    h2 = h.reshape(-1, N)
    scale = 10 ** (-snr / 20)
    kind = _NOISE_GEN if noise is None else _NOISE_GIVEN
    y = _observe(h2, M, A, scale, kind, noise, int(seed), int(offset), nb, thr, lab, nlev, device)
    return _squeeze_like_reference(y.reshape(*shape[:-1], M), shape)


def quant(inp, n_bits=1, thresholds=None, quant_labels=None, *, device=0):
    """Per-component quantiser (utils.py:189-203) on the device; output has inp's shape."""
    nb = _nbits(n_bits)
    thr, lab, nlev = _tables(nb, thresholds, quant_labels)
    shape = tuple(inp.shape)
    flat = inp.reshape(1, -1) if len(shape) != 2 else inp
    y = _observe(flat, flat.shape[1], None, 0.0, _NOISE_NONE, None, 0, 0, nb, thr, lab, nlev, device)
    return y.reshape(shape)


def sq_error(h_est, h, *, device=0):
    """sum |h_est - h|^2 on the device (deterministic order)."""
    if _is_tensor(h_est):
        import torch
        a = h_est.to(torch.complex128).contiguous()
        b = h.to(torch.complex128).contiguous()
        out = torch.empty(1, dtype=torch.float64, device=a.device)
        dev = a.device.index if a.device.index is not None else 0
        _lib.check(_lib.load().qce_sq_error(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(out), dev, _lib.IO_DEVICE,
                                            _stream(a)))
        return out
    a = np.ascontiguousarray(h_est, dtype=np.complex128)
    b = np.ascontiguousarray(h, dtype=np.complex128)
    if a.shape != b.shape:
        raise ValueError("shape mismatch")
    out = np.zeros(1)
    _lib.check(_lib.load().qce_sq_error(_lib.ptr(a), _lib.ptr(b), a.size, _lib.ptr(out), int(device), _lib.IO_HOST,
                                        None))
    return float(out[0])


def mse(h_est, h, *, device=0):
    """The scripts' MSE: sum |h_est - h|^2 / h.size (Bussgang_GMM.py:289)."""
    s = sq_error(h_est, h, device=device)
    n = h.numel() if _is_tensor(h) else np.asarray(h).size
    return s / n


# ------------------------------------------------------------------ random-SNR observations, encoder features
MAX_SNRS = 64
FEATURE_ANTENNAS = (16, 32, 64, 128, 256)
_FEATURES = {None: _lib.OUT_Y, "raw": _lib.OUT_FEATURES_RAW, "fft": _lib.OUT_FEATURES_DFT}


def _randsnr_tables(nb, snrs, quantizer):
    """Per-SNR tables stacked as (S, L-1) thresholds and (S, L) labels, from the dict of inputs.get_quantizer."""
    if nb == 1.0 or np.isinf(nb):
        return None, None, 0
    if quantizer is None:
        raise ValueError("multi-bit quantisation needs quantizer = {snr: (thresholds, labels, ...)}")
    thr, lab = [], []
    for s in snrs:
        if s not in quantizer:
            raise ValueError(f"quantizer has no entry for snr {s}")
        t = np.asarray(quantizer[s][0], dtype=np.float64).reshape(-1)
        v = np.asarray(quantizer[s][1], dtype=np.float64).reshape(-1)
        if v.size != t.size + 1:
            raise ValueError(f"snr {s}: {t.size} thresholds need {t.size + 1} labels, got {v.size}")
        thr.append(t)
        lab.append(v)
    if any(t.size != thr[0].size for t in thr):
        raise ValueError("quantizer tables differ in length between SNRs")
    return np.ascontiguousarray(np.stack(thr)), np.ascontiguousarray(np.stack(lab)), lab[0].size


def _randsnr_cdf(snr_scaling, S):
    """FP64 cumulative probabilities of snr_scaling under np.random.choice's own checks (None: uniform)."""
    if snr_scaling is None:
        return None
    p = np.asarray(snr_scaling, dtype=np.float64).reshape(-1)
    if p.size != S:
        raise ValueError(f"snr_scaling must have {S} entries, got {p.size}")
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        raise ValueError("snr_scaling must hold non-negative probabilities")
    if abs(float(np.sum(p)) - 1.0) > np.sqrt(np.finfo(np.float64).eps):
        raise ValueError("snr_scaling does not sum to 1")
    return np.ascontiguousarray(np.cumsum(p))


def _feature_shape(M, N, features):
    if features not in _FEATURES:
        raise ValueError(f"features must be None, 'raw' or 'fft', got {features!r}")
    if features is None:
        return
    if N not in FEATURE_ANTENNAS:
        raise NotImplementedError(f"features need n_antennas in {FEATURE_ANTENNAS}, got {N}")
    if M % N:
        raise NotImplementedError(f"features need M a multiple of n_antennas, got M = {M}, N = {N}")


def _observe_rows(h2, M, a, scales, cdf, idx, noise_kind, w2, seed, row_offset, nb, thr, lab, nlev, out_kind, device):
    """h2 (B, N) -> (y (B, M) complex128 or features (B, M / N, 2N) float32, snr_index (B,) int32)."""
    B, N = h2.shape
    S = scales.size
    oshape = (B, M) if out_kind == _lib.OUT_Y else (B, M // N, 2 * N)
    if _is_tensor(h2):
        import torch
        dev = h2.device
        h2 = h2.to(torch.complex128).contiguous()
        out = torch.empty(oshape, dtype=torch.complex128 if out_kind == _lib.OUT_Y else torch.float32, device=dev)
        iout = torch.empty(B, dtype=torch.int32, device=dev)
        if w2 is not None:
            w2 = torch.as_tensor(w2, dtype=torch.complex128, device=dev).reshape(B, M).contiguous()
        if idx is not None:
            idx = torch.as_tensor(idx, device=dev).to(torch.int32).contiguous()
        _lib.check(_lib.load().qce_observe_randsnr(
            _lib.ptr(h2), B, N, _lib.ptr(a), M, S, _lib.ptr(scales), _lib.ptr(cdf), _lib.ptr(idx), _lib.ptr(iout),
            noise_kind, _lib.ptr(w2), seed, row_offset, nb, _lib.ptr(thr), _lib.ptr(lab), nlev, out_kind,
            _lib.ptr(out), dev.index if dev.index is not None else 0, _lib.IO_DEVICE, _stream(h2)))
        return out, iout
    h2 = np.ascontiguousarray(h2, dtype=np.complex128)
    if w2 is not None:
        w2 = np.ascontiguousarray(np.asarray(w2, dtype=np.complex128).reshape(B, M))
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.int32)
    out = np.empty(oshape, dtype=np.complex128 if out_kind == _lib.OUT_Y else np.float32)
    iout = np.empty(B, dtype=np.int32)
    _lib.check(_lib.load().qce_observe_randsnr(
        _lib.ptr(h2), B, N, _lib.ptr(a), M, S, _lib.ptr(scales), _lib.ptr(cdf), _lib.ptr(idx), _lib.ptr(iout),
        noise_kind, _lib.ptr(w2), seed, row_offset, nb, _lib.ptr(thr), _lib.ptr(lab), nlev, out_kind, _lib.ptr(out),
        int(device), _lib.IO_HOST, None))
    return out, iout


def get_observation_nbit_randSNR(h, snrs, A=None, n_bits=1, quantizer=None, snr_scaling=None, *, snr_index=None,
                                 noise=None, seed=0, row_offset=0, device=0, features=None):
    """Row b observed at its own SNR: y_b = Q_snr(A h_b + 10^(-snr/20) n_b) with snr = snrs[i_b], i_b drawn with
    probabilities ``snr_scaling`` (uniform when None) — utils.py:254-268 and its torch variants (:271-318), in one
    launch of csrc/qce_observe_rows.hip.  Returns ``(y, snr_list)``: y (B, M) complex128 and snr_list (B,) float64.

    ``quantizer`` is the dict of ``inputs.get_quantizer``: snr -> (thresholds, labels, ...).  Keyword arguments:

    * ``snr_index`` (B,) / ``noise`` (B, M) — the reference's own draws; with both, and A = None or kron(x, I), y is
      bit-identical to the reference's.
    * ``seed`` / ``row_offset`` — draws made on the device (Philox4x32-10): row b's index uses counter row_offset + b,
      its noise the counters (row_offset + b) M + m of ``get_observation_nbit``'s stream, so rows [B1, B) generated
      with ``row_offset=B1`` equal the one-shot rows.
    * ``features`` — ``"fft"`` / ``"raw"``: instead of y, the VAE encoder's float32 input (B, P, 2N), M = P N
      (vae.py:48-53, :90-94): row (b, p) = [Re f | Im f], f the unitary DFT of y_b[pN:(p+1)N] (``"raw"``: f = that
      slice).  The complex128 y is then never written to memory.

    numpy in, numpy out; a CUDA complex128 tensor in gives tensors on its device, async on the current torch stream."""
    sn = np.asarray(snrs).reshape(-1)
    S = sn.size
    if S < 1 or S > MAX_SNRS:
        raise ValueError(f"snrs must hold 1 to {MAX_SNRS} values, got {S}")
    nb = _nbits(n_bits)
    thr, lab, nlev = _randsnr_tables(nb, sn, quantizer)  # numpy scalars hash and compare like the dict's Python keys
    cdf = _randsnr_cdf(snr_scaling, S)
    shape = tuple(h.shape)
    if len(shape) != 2:
        raise ValueError(f"h must be (B, N), got {shape}")
    B, N = shape
    a = None if A is None else np.ascontiguousarray(np.asarray(A.cpu() if _is_tensor(A) else A), dtype=np.complex128)
    if a is not None and (a.ndim != 2 or a.shape[1] != N):
        raise ValueError(f"A must have {N} columns")
    M = N if a is None else a.shape[0]
    _feature_shape(M, N, features)
    if snr_index is not None:
        if tuple(snr_index.shape) != (B,):
            raise ValueError(f"snr_index must be ({B},), got {tuple(snr_index.shape)}")
        if B and (int(snr_index.min()) < 0 or int(snr_index.max()) >= S):
            raise ValueError(f"snr_index must lie in [0, {S})")
    if noise is not None and tuple(noise.shape) != (B, M):
        raise ValueError(f"noise must be ({B}, {M}), got {tuple(noise.shape)}")
    scales = np.array([10 ** (-s / 20) for s in sn], dtype=np.float64)  # numpy scalars, as the reference computes it
    kind = _NOISE_GEN if noise is None else _NOISE_GIVEN
    out, idx = _observe_rows(h, M, a, scales, cdf, snr_index, kind, noise, int(seed), int(row_offset), nb, thr, lab,
                             nlev, _FEATURES[features], device)
    if _is_tensor(idx):
        import torch
        snr_list = torch.as_tensor(sn.astype(np.float64), device=idx.device).index_select(0, idx)
    else:
        snr_list = sn.astype(np.float64)[idx]
    return out, snr_list


def encoder_features(y, n_antennas, fft_pre=True, *, device=0):
    """float32 (B, P, 2N) encoder input of observations y (B, P N) that already exist (the validation sets of
    Bussgang_VAE.py:160; vae.py:48-53): the feature pass of ``get_observation_nbit_randSNR`` with no noise, no
    quantiser and A = I over y's (B P, N) rows."""
    N = int(n_antennas)
    if len(y.shape) != 2:
        raise ValueError(f"y must be (B, P N), got {tuple(y.shape)}")
    B, M = y.shape
    _feature_shape(M, N, "fft")
    rows = y.reshape(B * (M // N), N)
    out, _ = _observe_rows(rows, N, None, np.ones(1), None, None, _NOISE_NONE, None, 0, 0, np.inf, None, None, 0,
                           _lib.OUT_FEATURES_DFT if fft_pre else _lib.OUT_FEATURES_RAW, device)
    return out.reshape(B, M // N, 2 * N)
