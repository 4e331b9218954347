"""VAE-parameterised Bussgang estimator, evaluation side (reference estimators/vae.py, driven by Bussgang_VAE.py).

``lmmse_from_decoder`` is the hot path: the reference's ``convert_dec_outputs`` (:376-431, zeromean=True) followed
by ``lmmse`` (:368-369), computed by libqce.so in the Fourier domain (``qce_vae_estimate``, csrc/qce_vae.hip).
``VAE_nbit`` wraps it with the reference's input preparation (:161-172) and the encoder / decoder forward of
``DNN_VAE.forward_nosamp`` (:294-309), written as torch.nn.functional calls in float32 on the device (the
reference's precision; this part is plumbing).  Training (``VAE_nbit.train``, ``vae_loss``) is not part of the
package: the class consumes trained weights, under the reference's state-dict names.

The reference's behaviour is kept where it is observable, including its failures:

* ``zeromean=False`` raises the reference's ValueError (real2cplx_torch splits into chunks of 2, :634);
* ``quantizer_type='lloyd'`` with 1 < n_bits < inf raises its TypeError (:424);
* ``eval`` on a batch count with ``B % 50 == 1`` raises its IndexError (torch.squeeze in forward_nosamp drops
  the batch axis of the last batch of one row, :297); ``estimate_from_y`` takes any B >= 1;
* ``eval`` with ``eval_rate`` false raises its AttributeError (:226 calls .cpu() on the float 0.0);
* ``apply_batchnorm=True`` is refused: the reference never puts the module into eval mode, so its outputs depend
  on how the evaluation set falls into batches of 50.

Not emulated: ``pinv(hermitian=True)``'s eigenvalue cut-off.  The kernel solves with a Cholesky factorisation per
DFT bin and raises ValueError when a bin is not positive definite.
"""
import numpy as np

from . import _lib, observe, rate as _rate

ZEROMEAN_MESSAGE = "too many values to unpack (expected 2)"
LLOYD_MESSAGE = "can't assign a numpy.ndarray to a torch.ComplexDoubleTensor"
BATCH1_MESSAGE = "too many indices for tensor of dimension 1"
NORATE_MESSAGE = "'float' object has no attribute 'cpu'"
MAX_PILOTS = 4
EVAL_BATCH = 50  # the reference's DataLoader batch size in eval (:177)

# the reference's float32 constants (torch.tensor(np.pi) is a float32 tensor; uniform_quantizer.py:79, :86)
_K1 = float(np.sqrt(np.float32(2) / np.float32(np.pi), dtype=np.float32))


def _is_tensor(x):
    return not isinstance(x, np.ndarray) and hasattr(x, "data_ptr")


def _nbits(n_bits):
    if n_bits == "inf" or n_bits == np.inf:
        return np.inf
    return float(n_bits)


def pilot_vector(A, N):
    """x (P,) with A = kron(x, I_N) to 1e-12 (the scripts' pilot matrices, utils.py:337-367); A = None: x = [1].
    Any other A, P > 4, or an N that is not a power of two in [16, 256] -> NotImplementedError."""
    N = int(N)
    if N < 16 or N > 256 or N & (N - 1):
        raise NotImplementedError(f"n_antennas must be a power of two in [16, 256], got {N}")
    if A is None:
        return np.ones(1, dtype=np.complex128)
    A = np.asarray(A.cpu() if _is_tensor(A) else A, dtype=np.complex128)
    if A.ndim != 2 or A.shape[1] != N or A.shape[0] % N:
        raise NotImplementedError(f"A must be kron(x, I_{N}), got shape {A.shape}")
    P = A.shape[0] // N
    if P > MAX_PILOTS:
        raise NotImplementedError(f"at most {MAX_PILOTS} pilots, got {P}")
    x = np.ascontiguousarray(A[::N, 0])
    if np.max(np.abs(A - np.kron(x[:, None], np.eye(N)))) > 1e-12:
        raise NotImplementedError("A is not kron(x, I_N): only the scripts' pilot matrices are covered")
    return x


def lmmse_from_decoder(y, log_var, snr, A=None, n_bits=1, quantizer_type="uniform", zeromean=True, device=0):
    """h (B, N) from observations y (B, P N) complex and decoder log-variances log_var (B, N), float32 or float64.

    numpy in, numpy out; CUDA tensors in (y complex128, log_var float32 / float64), tensor out on the same device
    (the call synchronises the current stream to read the kernel's status)."""
    if not zeromean:
        raise ValueError(ZEROMEAN_MESSAGE)
    nb = _nbits(n_bits)
    if nb != 1.0 and not np.isinf(nb) and quantizer_type == "lloyd":
        raise TypeError(LLOYD_MESSAGE)
    if log_var.ndim != 2:
        raise ValueError("log_var must be (B, N)")
    B, N = (int(v) for v in log_var.shape)
    x = pilot_vector(A, N)
    P = x.size
    if tuple(y.shape) != (B, P * N):
        raise ValueError(f"y must be ({B}, {P * N}), got {tuple(y.shape)}")
    other = nb != 1.0 and not np.isinf(nb) and quantizer_type != "uniform"  # the gain stays 0 (:421-426): h = 0
    if _is_tensor(y) or _is_tensor(log_var):
        import torch
        dev = y.device if _is_tensor(y) else log_var.device
        y = torch.as_tensor(y, device=dev).to(torch.complex128).contiguous()
        lv = torch.as_tensor(log_var, device=dev)
        if lv.dtype not in (torch.float32, torch.float64):
            lv = lv.to(torch.float64)
        lv = lv.contiguous()
        h = torch.zeros((B, N), dtype=torch.complex128, device=dev)
        if not other and B:
            _lib.check(_lib.load().qce_vae_estimate(N, P, _lib.ptr(x), float(snr), nb, _lib.ptr(lv),
                                                    int(lv.dtype == torch.float32), _lib.ptr(y), B, _lib.ptr(h),
                                                    _lib.IO_DEVICE, dev.index or 0,
                                                    torch.cuda.current_stream(dev).cuda_stream))
        return h
    y = np.ascontiguousarray(y, dtype=np.complex128)
    lv = np.asarray(log_var)
    lv = np.ascontiguousarray(lv, dtype=np.float32 if lv.dtype == np.float32 else np.float64)
    h = np.zeros((B, N), dtype=np.complex128)
    if not other and B:
        _lib.check(_lib.load().qce_vae_estimate(N, P, _lib.ptr(x), float(snr), nb, _lib.ptr(lv),
                                                int(lv.dtype == np.float32), _lib.ptr(y), B, _lib.ptr(h),
                                                _lib.IO_HOST, int(device), None))
    return h


def layer_shapes(params):
    """{state-dict name: shape} of the reference's DNN_VAE (:237-267) for these params."""
    N, P, L, nl = (int(params[k]) for k in ("n_antennas", "n_pilots", "latent_dim", "n_layers"))
    npc = int(params.get("n_pilot_convs", 0))
    shapes = {}
    convs = np.linspace(P, 1, npc + 1, dtype=int)
    for i in range(npc):
        shapes[f"pre_pilot.conv{i}.weight"] = (int(convs[i + 1]), int(convs[i]), 1)
        shapes[f"pre_pilot.conv{i}.bias"] = (int(convs[i + 1]),)
    enc = np.linspace(2 * N, 2 * L, nl + 1, dtype=int)
    dec = np.linspace(L, N, nl + 1, dtype=int)
    for name, n in (("enc", enc), ("dec", dec)):
        for i in range(nl):
            shapes[f"{name}.linear{i}.weight"] = (int(n[i + 1]), int(n[i]))
            shapes[f"{name}.linear{i}.bias"] = (int(n[i + 1]),)
    return shapes


class VAE_nbit:
    """Evaluation side of the reference's ``VAE_nbit`` (estimators/vae.py:11-228) with the same ``params`` keys:
    n_antennas, n_pilots, latent_dim, n_layers, n_pilot_convs, vae_mode ('genie' / 'noisy' / 'real'), fft_pre,
    zeromean, apply_batchnorm, n_bits, quantizer_type, quantizer ({snr: (thresholds, labels, rho)}), A, eval_rate.
    ``device`` (optional) is the GPU index or a torch device."""

    def __init__(self, params):
        self.params = params
        if params.get("apply_batchnorm", False):
            raise NotImplementedError("apply_batchnorm=True: the reference evaluates its BatchNorm layers in training "
                                      "mode, so its estimates depend on the batches of 50 they fall into")
        if params["vae_mode"] not in ("genie", "noisy", "real"):
            raise NotImplementedError("Choose a valid VAE-option.")
        if params["vae_mode"] != "genie" and int(params["n_pilots"]) > 1 and not int(params.get("n_pilot_convs", 0)):
            raise NotImplementedError("several pilots need n_pilot_convs >= 1 (the reference's encoder takes one row)")
        self._w = None

    # ------------------------------------------------------------------ weights
    def _device(self):
        import torch
        d = self.params.get("device", 0)
        if isinstance(d, torch.device) and d.type == "cuda":
            return d
        return torch.device("cuda", d if isinstance(d, int) else 0)

    def load_state_dict(self, mapping):
        """Weights under the reference's names (pre_pilot.conv{i}.*, enc.linear{i}.*, dec.linear{i}.*), numpy
        arrays or tensors; stored as float32 on the device."""
        import torch
        if not self.params.get("zeromean", True):
            raise ValueError(ZEROMEAN_MESSAGE)
        dev = self._device()
        w = {}
        for name, shape in layer_shapes(self.params).items():
            if name not in mapping:
                raise KeyError(f"state dict lacks {name}")
            t = mapping[name]
            t = t.detach() if _is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
            t = t.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
            w[name] = t
        self._w = w
        return self

    @classmethod
    def from_checkpoint(cls, path, params=None):
        """The reference's checkpoint file {'model': state_dict, 'params': params} (:148-153).  With ``params`` given,
        the checkpoint's hyper-parameters are assigned into it as ``assign_params`` does (:495-502)."""
        import torch
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if params is None:
            params = dict(ck["params"])
        else:
            for k in ("n_layers", "lr", "batch_size", "apply_batchnorm", "latent_dim"):
                if k in ck["params"]:
                    params[k] = ck["params"][k]
        return cls(params).load_state_dict(ck["model"])

    # ------------------------------------------------------------------ forward
    def _inputs(self, y, h, B):
        """Encoder input (float32, on the device) as eval prepares it (:161-172)."""
        import torch
        p = self.params
        N, P = int(p["n_antennas"]), int(p["n_pilots"])
        dev = self._device()
        if p["vae_mode"] == "genie":
            if h is None:
                raise ValueError("vae_mode 'genie' encodes the true channel: pass h")
            v = torch.as_tensor(h, device=dev).to(torch.complex128).reshape(B, N)
            v = torch.fft.fft(v, dim=1) / np.sqrt(N)
            return torch.cat([v.real, v.imag], dim=1).float()
        # reshape (-1, N, P) in Fortran order, then transpose: row p of sample b is y[b, p N : (p + 1) N]
        v = y.reshape(B, P, N)
        if p.get("fft_pre", True):
            v = torch.fft.fft(v, dim=-1) / np.sqrt(N)
        return torch.cat([v.real, v.imag], dim=-1).float()

    def forward_nosamp(self, x):
        """Decoder log-variances (B, N) float32 for encoder inputs x: (B, P, 2N), or (B, 2N) in 'genie' mode."""
        import torch.nn.functional as Fn
        if self._w is None:
            raise RuntimeError("no weights: call load_state_dict or from_checkpoint first")
        p, w = self.params, self._w
        nl = int(p["n_layers"])
        if p["vae_mode"] != "genie":
            for i in range(int(p.get("n_pilot_convs", 0))):
                x = Fn.relu(Fn.conv1d(x, w[f"pre_pilot.conv{i}.weight"], w[f"pre_pilot.conv{i}.bias"]))
            x = x.squeeze(1)
        for i in range(nl):
            x = Fn.linear(x, w[f"enc.linear{i}.weight"], w[f"enc.linear{i}.bias"])
            if i < nl - 1:
                x = Fn.relu(x)
        x = x[:, :x.shape[-1] // 2]
        for i in range(nl):
            x = Fn.linear(x, w[f"dec.linear{i}.weight"], w[f"dec.linear{i}.bias"])
            if i < nl - 1:
                x = Fn.relu(x)
        return x

    def _estimate(self, y, snr, h):
        import torch
        p = self.params
        if not p.get("zeromean", True):
            raise ValueError(ZEROMEAN_MESSAGE)
        N, P = int(p["n_antennas"]), int(p["n_pilots"])
        pilot_vector(p.get("A"), N)  # refuse before anything is uploaded
        dev = self._device()
        y_t = torch.as_tensor(y, device=dev).to(torch.complex128)
        B = y_t.numel() // (P * N)
        y_t = y_t.reshape(B, P * N).contiguous()
        with torch.no_grad():
            lv = self.forward_nosamp(self._inputs(y_t, h, B))
        return lmmse_from_decoder(y_t, lv, snr, p.get("A"), p["n_bits"], p.get("quantizer_type", "uniform"), True)

    def estimate_from_y(self, y, snr, h=None):
        """Channel estimates (B, N) for observations y (B, P N); any B >= 1.  ``h``: the true channels, needed by
        vae_mode 'genie' only.  numpy in, numpy out; CUDA tensor in, tensor out."""
        hh = self._estimate(y, snr, h)
        return hh if _is_tensor(y) else hh.cpu().numpy()

    # ------------------------------------------------------------------ eval
    def _bussgang_global(self, cov, snr):
        """(gain (N,), Cq) as eval builds them (:187-195): get_Bussgang_matrix_torch with its float32 constants,
        get_Cr_torch (float64 2/pi; multi-bit: mean(gain)^2 Cy with the quantised variance on the diagonal)."""
        p = self.params
        nb = _nbits(p["n_bits"])
        N = cov.shape[0]
        Cy = cov + 10 ** (-snr / 10) * np.eye(N)
        d = np.real(np.diag(Cy))
        if np.isinf(nb):
            g, Cr = np.ones(N), Cy
        elif nb == 1.0:
            g = _K1 * (1 / np.sqrt(d))
            psi = 1 / np.sqrt(d)
            re = np.clip(psi[:, None] * Cy.real * psi[None, :], -1, 1)
            im = np.clip(psi[:, None] * Cy.imag * psi[None, :], -1, 1)
            Cr = 2 / np.pi * (np.arcsin(re) + 1j * np.arcsin(im))
        else:
            from .inputs import uniform_step
            delta = uniform_step(snr, int(nb))
            s = np.zeros(N)
            for i in range(1, 2 ** int(nb)):
                s += np.exp(-delta ** 2 * (i - 2 ** int(nb) / 2) ** 2 * (1 / d))
            g = s * (float(np.float32(delta) / np.sqrt(np.float32(np.pi), dtype=np.float32)) / np.sqrt(d))
            q = p["quantizer"][snr]
            Cr = np.mean(g) ** 2 * Cy
            np.fill_diagonal(Cr, _rate.quantized_variance(d, q[0], q[1]))
        return g, Cr - (g[:, None] * cov) * g[None, :]

    def eval(self, h_eval, y_eval, snr, h_train):
        """(mse, rate, params) as the reference's eval (:157-228): MSE = sum |h_hat - h|^2 / h.size on the device,
        rate = the statistical lower bound with the global Bussgang pair of the training channels' sample covariance
        (g = h_hat / ||h_hat||^2; torch.var's n - 1 normalisation of the inner products)."""
        p = self.params
        h_eval = np.asarray(h_eval)
        B = h_eval.shape[0]
        if p["vae_mode"] != "genie" and B % EVAL_BATCH == 1:
            raise IndexError(BATCH1_MESSAGE)
        hh = self._estimate(y_eval, snr, h_eval)
        import torch
        h_t = torch.as_tensor(h_eval, device=hh.device).to(torch.complex128)
        mse = float(observe.sq_error(hh, h_t)) / h_eval.size
        if not p.get("eval_rate", False):
            raise AttributeError(NORATE_MESSAGE)
        h_train = np.asarray(h_train, dtype=np.complex128)
        cov = (h_train.T @ h_train.conj()) / h_train.shape[0]
        g, Cq = self._bussgang_global(cov, snr)
        _, t = _rate.statistical_rate_bound(hh, h_t, g, Cq, return_terms=True)
        den1 = t["den1"] * B / (B - 1) if B > 1 else float("nan")  # torch.var is unbiased (:222)
        return mse, float(np.log2(1 + t["num"] / (den1 + t["den2"]))), self.params
