"""VAE-parameterised Bussgang estimator (reference estimators/vae.py, driven by Bussgang_VAE.py).

Evaluation.  ``lmmse_from_decoder`` is the hot path: the reference's ``convert_dec_outputs`` (:376-431,
zeromean=True) followed by ``lmmse`` (:368-369), computed by libqce.so in the Fourier domain (``qce_vae_estimate``,
csrc/qce_vae.hip).  ``VAE_nbit`` wraps it with the reference's input preparation (:161-172) and the encoder / decoder
forward of ``DNN_VAE.forward_nosamp`` (:294-309), written as torch.nn.functional calls in float32 on the device (the
reference's precision; this part is plumbing).  ``fused=True`` (``estimate_from_y``, ``eval``) and ``forward_fused``
run the same network inside libqce.so instead (``qce_vae_net_forward``, csrc/qce_vae_net.hip): features, pilot
convolutions, encoder and decoder in one kernel, then the LMMSE kernel on the same stream, two launches per chunk and
no torch op.  The default stays the torch path.

Training.  ``VAE_nbit.train`` is the reference's loop (:15-154) on the device.  The layers stay torch.nn.functional
calls under autograd; what lies between and around them is libqce.so (csrc/qce_vae_train.hip): ``reparameterize``
(z = mu + exp(s) eps, eps drawn by the kernel) and ``elbo_loss`` (``vae_loss``, :312-365: the per-row ELBO in FP64 and
its analytic gradient in the same pass, all three modes).  The per-epoch observations come from
``observe.get_observation_nbit_randSNR(features=...)``.  Training is equivalent to the reference's, not bit-equal:
torch's RNG streams for the initialisation, the shuffling and eps cannot be reproduced on another device, so the
weights start from other draws of the same distributions (nn.Linear's / nn.Conv1d's uniform bounds), every step takes
``batch_size`` distinct uniformly drawn rows as the reference's ``next(iter(dataloader))`` does, and eps is Philox
noise.  Checkpoints carry the reference's keys and state-dict names.  In 'real' mode both the training and the
validation observations are DFT features whatever ``fft_pre`` says; the reference transforms its training set always
and its validation set only with ``fft_pre`` (:64-65, :100), so with ``fft_pre=False`` its validation loss is of another
kind than its training loss, and than the validation loss here.  ``train(..., fused=True)`` runs the same loop with
every training step inside libqce.so (csrc/qce_vae_step.hip, ``qce_vae_trainer_*``): gather, layers, loss, backward and
Adam in two kernels on weights and optimiser state the library holds, one host read per epoch; ``step_gradients``
returns that step's loss and parameter gradients without an update.  The default stays the torch path.

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
import os

import numpy as np

from . import _lib, observe, rate as _rate

ZEROMEAN_MESSAGE = "too many values to unpack (expected 2)"
LLOYD_MESSAGE = "can't assign a numpy.ndarray to a torch.ComplexDoubleTensor"
BATCH1_MESSAGE = "too many indices for tensor of dimension 1"
NORATE_MESSAGE = "'float' object has no attribute 'cpu'"
HTEST_MESSAGE = "local variable 'dataloader_test' referenced before assignment"  # UnboundLocalError, train (:132)
MAX_PILOTS = 4
MAX_LATENT = 128       # latent_dim the training kernels take
MAX_REAL_BITS = 8      # uniform quantisers of the 'real' loss
LOSS_SKIP = 1000.0     # a step whose loss is NaN or above this is skipped (:120-121); epoch means are clipped to it
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


def _f32_device(t, name, ncols=None):
    """t as a contiguous float32 CUDA tensor (B, ncols); anything else is an error (there is no CPU path)."""
    import torch
    if not _is_tensor(t) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA tensor (the training kernels run on the device only)")
    if t.dtype != torch.float32 or t.dim() != 2 or (ncols is not None and t.shape[1] != ncols):
        raise ValueError(f"{name} must be float32 (B, {ncols if ncols is not None else 'n'}), got {t.dtype} "
                         f"{tuple(t.shape)}")
    return t.contiguous()


def _dev_stream(t):
    import torch
    return t.device.index or 0, torch.cuda.current_stream(t.device).cuda_stream


_FUNCTIONS = None


def _functions():
    """The two torch.autograd.Function classes over csrc/qce_vae_train.hip (built on first use: torch is imported
    lazily throughout this module)."""
    global _FUNCTIONS
    if _FUNCTIONS is not None:
        return _FUNCTIONS
    import torch

    class Reparameterize(torch.autograd.Function):
        @staticmethod
        def forward(ctx, enc, eps, seed, row_offset):
            enc = enc.detach()
            B, L = enc.shape[0], enc.shape[1] // 2
            z = torch.empty((B, L), dtype=torch.float32, device=enc.device)
            eps_out = torch.empty((B, L), dtype=torch.float32, device=enc.device)
            dev, st = _dev_stream(enc)
            _lib.check(_lib.load().qce_vae_sample(_lib.ptr(enc), B, L, _lib.ptr(eps), int(seed), int(row_offset),
                                                  _lib.ptr(z), _lib.ptr(eps_out), dev, st))
            ctx.save_for_backward(enc, eps_out)
            ctx.mark_non_differentiable(eps_out)
            return z, eps_out

        @staticmethod
        def backward(ctx, g_z, _g_eps):
            enc, eps = ctx.saved_tensors
            B, L = eps.shape
            g_z = g_z.to(torch.float32).contiguous()
            g_enc = torch.empty_like(enc)
            dev, st = _dev_stream(enc)
            _lib.check(_lib.load().qce_vae_sample_bwd(_lib.ptr(enc), _lib.ptr(eps), _lib.ptr(g_z), B, L,
                                                      _lib.ptr(g_enc), dev, st))
            return g_enc, None, None, None

    class ElboLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, enc, dec, target, mode, n_bits, snr_db, index):
            enc, dec = enc.detach(), dec.detach()
            B, N, L = dec.shape[0], dec.shape[1], enc.shape[1] // 2
            rows = torch.empty(B, dtype=torch.float64, device=enc.device)
            g_enc, g_dec = torch.empty_like(enc), torch.empty_like(dec)
            dev, st = _dev_stream(enc)
            _lib.check(_lib.load().qce_vae_elbo(_lib.ptr(enc), _lib.ptr(dec), _lib.ptr(target), target.shape[0], B, N, L,
                                                mode, n_bits, _lib.ptr(index), _lib.ptr(snr_db), _lib.ptr(rows),
                                                _lib.ptr(g_enc), _lib.ptr(g_dec), dev, st))
            ctx.save_for_backward(g_enc, g_dec)
            ctx.mark_non_differentiable(rows)
            return (-rows.mean()).to(torch.float32), rows  # the mean in FP64, in torch's fixed reduction order

        @staticmethod
        def backward(ctx, g_loss, _g_rows):
            g_enc, g_dec = ctx.saved_tensors  # the forward's gradients: no second pass over the data
            return g_enc * g_loss, g_dec * g_loss, None, None, None, None, None

    _FUNCTIONS = (Reparameterize, ElboLoss)
    return _FUNCTIONS


def reparameterize(enc_out, eps=None, *, seed=0, row_offset=0, return_eps=False):
    """z (B, L) float32 = mu + exp(s) eps for the encoder output enc_out (B, 2L) = [mu | s] (float32, CUDA), with
    autograd (``k_vae_sample`` / ``k_vae_sample_bwd``, FP64 arithmetic rounded once).  ``eps`` (B, L) float32, or None:
    drawn on the device (Philox4x32-10 keyed by ``seed``; element (b, l) uses counter (row_offset + b) L + l, so rows
    [B1, B) drawn with ``row_offset=B1`` equal the one-shot rows).  ``return_eps``: (z, eps)."""
    enc = _f32_device(enc_out, "enc_out")
    if enc.shape[1] % 2 or enc.shape[1] < 2:
        raise ValueError(f"enc_out must be (B, 2 L), got {tuple(enc.shape)}")
    L = enc.shape[1] // 2
    if L > MAX_LATENT:
        raise NotImplementedError(f"latent_dim up to {MAX_LATENT}, got {L}")
    if eps is not None:
        eps = _f32_device(eps, "eps", L)
        if eps.shape[0] != enc.shape[0]:
            raise ValueError(f"eps must be ({enc.shape[0]}, {L}), got {tuple(eps.shape)}")
    z, e = _functions()[0].apply(enc, eps, int(seed), int(row_offset))
    return (z, e) if return_eps else z


def elbo_loss(enc_out, dec_out, target, *, mode, n_bits=1, snr_db=None, index=None, return_rows=False,
              check_index=False):
    """The reference's ``vae_loss`` (:312-365, zeromean=True) as a float32 scalar with autograd: -mean_b of the row
    ELBOs, which ``k_vae_elbo`` computes in FP64 together with the gradient (``return_rows``: (loss, rows (B,)
    float64)).  enc_out (B, 2L) = [mu | log_var_enc], dec_out (B, N) = log_var_dec, target (T, 2N) = [re | im], all
    float32 CUDA tensors; row b uses target row (and SNR entry) ``index[b]`` (int32 (B,), values in [0, T), duplicates
    allowed), or row b without ``index``.  mode 'genie' / 'noisy': the target is the channel's DFT features; 'real':
    the observation's own features, with ``snr_db`` (T,) and a uniform quantiser of ``n_bits`` in 1..8 or inf.

    The call is asynchronous, so ``index`` is not read on the host: the kernel clamps a value outside [0, T) to the
    nearest valid row without an error, and loss and gradients are then those of the clamped rows.  ``check_index=True``
    reads the index's range first (one host synchronisation) and raises ValueError instead."""
    import torch
    if mode not in ("genie", "noisy", "real"):
        raise NotImplementedError("Choose a valid VAE-option.")
    dec = _f32_device(dec_out, "dec_out")
    B, N = dec.shape
    pilot_vector(None, N)  # the shape refusal
    enc = _f32_device(enc_out, "enc_out")
    if enc.shape[0] != B or enc.shape[1] % 2 or enc.shape[1] < 2:
        raise ValueError(f"enc_out must be ({B}, 2 L), got {tuple(enc.shape)}")
    if enc.shape[1] // 2 > MAX_LATENT:
        raise NotImplementedError(f"latent_dim up to {MAX_LATENT}, got {enc.shape[1] // 2}")
    tgt = _f32_device(target.detach() if _is_tensor(target) else target, "target", 2 * N)
    T = tgt.shape[0]
    if index is not None:
        if not _is_tensor(index) or not index.is_cuda or tuple(index.shape) != (B,):
            raise ValueError(f"index must be a CUDA tensor ({B},)")
        if T < 1:
            raise ValueError("target is empty")
        if check_index and B and (int(index.min()) < 0 or int(index.max()) >= T):
            raise ValueError(f"index must lie in [0, {T})")
        index = index.to(torch.int32).contiguous()
    elif T < B:
        raise ValueError(f"target has {T} rows for a batch of {B}")
    nb = 1.0
    if mode == "real":
        nb = _nbits(n_bits)
        if not np.isinf(nb) and (nb != int(nb) or nb < 1):
            raise ValueError("n_bits must be an integer >= 1 or inf")
        if not np.isinf(nb) and nb > MAX_REAL_BITS:
            raise NotImplementedError(f"the 'real' loss covers uniform quantisers up to {MAX_REAL_BITS} bits")
        if snr_db is None:
            raise ValueError("mode 'real' needs snr_db, one value per target row")
        snr_db = torch.as_tensor(snr_db, device=dec.device).to(torch.float64).reshape(-1).contiguous()
        if snr_db.shape[0] != T:
            raise ValueError(f"snr_db must have {T} entries, got {snr_db.shape[0]}")
    else:
        snr_db = None
    loss, rows = _functions()[1].apply(enc, dec, tgt, int(mode == "real"), float(nb), snr_db, index)
    return (loss, rows) if return_rows else loss


def _widths(params):
    """The channel counts of the pilot convolutions (P .. 1), the encoder's widths (2N .. 2L) and the decoder's (L .. N)
    in one int32 array, as ``qce_vae_net_create`` and ``qce_vae_trainer_create`` take them."""
    N, P, L, nl = (int(params[k]) for k in ("n_antennas", "n_pilots", "latent_dim", "n_layers"))
    npc = int(params.get("n_pilot_convs", 0))
    return np.concatenate([np.linspace(P, 1, npc + 1, dtype=int), np.linspace(2 * N, 2 * L, nl + 1, dtype=int),
                           np.linspace(L, N, nl + 1, dtype=int)]).astype(np.int32)


def fused_step_lds_bytes(params):
    """LDS bytes one workgroup of the fused training step (``k_vae_step``) needs for these params, as
    ``qce_vae_trainer_create`` computes them: the stored activations of 16 rows (one buffer per layer input and output,
    row stride = width rounded up to 16, plus 4 floats), the raw tile of the pilot convolutions, eps and the KL
    gradient, two delta buffers of the widest layer, and the gather table."""
    N, P, L, nl = (int(params[k]) for k in ("n_antennas", "n_pilots", "latent_dim", "n_layers"))
    npc = 0 if params["vae_mode"] == "genie" else int(params.get("n_pilot_convs", 0))
    conv = np.linspace(P, 1, npc + 1, dtype=int)
    widths = [2 * N] + [int(v) for v in np.linspace(2 * N, 2 * L, nl + 1, dtype=int)[1:]]
    widths += [int(v) for v in np.linspace(L, N, nl + 1, dtype=int)]
    up16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    floats = sum(16 * (up16(v) + 4) for v in widths)
    floats = max(floats, 256 * sum(int(conv[i + 1] * conv[i] + conv[i + 1]) for i in range(npc)))
    if npc:
        floats += 16 * P * 2 * N
    floats += 16 * L + 16 * 2 * L + 2 * 16 * (up16(max(widths)) + 4)
    return 4 * floats + 256


FUSED_STEP_LDS_LIMIT = 160 * 1024  # bytes of LDS per workgroup
FUSED_STEP_SLOTS = 4096            # entries of the trainer's loss record (QCE_VAE_TRAINER_SLOTS)
_MODE_CODE = {"genie": 0, "noisy": 1, "real": 2}


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
        self._net = None  # the packed handle of the fused forward (qce_vae_net), built on first use
        self._trainer = None  # (handle, max_batch) of the fused training step (qce_vae_trainer), built on first use

    def __del__(self):
        try:
            self._drop_net()
            self._drop_trainer()
        except Exception:  # interpreter teardown
            pass

    # ------------------------------------------------------------------ weights
    def _drop_net(self):
        """Destroy the packed handle: the weights it was built from are being replaced (or the object goes)."""
        net, self._net = getattr(self, "_net", None), None
        if net is not None:
            _lib.load().qce_vae_net_destroy(net)

    def _net_handle(self):
        """The library's handle for the current weights (``qce_vae_net_create``), cached until they change."""
        if self._w is None:
            raise RuntimeError("no weights: call load_state_dict, from_checkpoint or train first")
        if self._net is not None:
            return self._net
        import ctypes
        import torch
        p = self.params
        N, P, L, nl = (int(p[k]) for k in ("n_antennas", "n_pilots", "latent_dim", "n_layers"))
        npc = int(p.get("n_pilot_convs", 0))
        widths = _widths(p)
        flat = torch.cat([self._w[name].detach().reshape(-1) for name in layer_shapes(p)]).contiguous()
        out = ctypes.c_void_p()
        _lib.check(_lib.load().qce_vae_net_create(N, P, L, nl, npc, int(p["vae_mode"] == "genie"), _lib.ptr(widths),
                                                  _lib.ptr(flat), flat.numel(), _lib.IO_DEVICE, flat.device.index or 0,
                                                  ctypes.byref(out)))
        self._net = out
        _lib._live["vae_net"].add(self)  # closed at exit while the HIP runtime is still up
        return out

    def close(self):
        """Free the library's handles (fused forward, fused training step); they are rebuilt on the next fused call."""
        self._drop_net()
        self._drop_trainer()

    def _drop_trainer(self):
        tr, self._trainer = getattr(self, "_trainer", None), None
        if tr is not None:
            _lib.load().qce_vae_trainer_destroy(tr[0])

    def _trainer_handle(self, max_batch):
        """The library's trainer for the current weights (``qce_vae_trainer_create``: it copies them and starts Adam
        from zero moments), cached until the weights are replaced or a larger batch comes."""
        if self._w is None:
            raise RuntimeError("no weights: call load_state_dict, from_checkpoint or train first")
        if self._trainer is not None and self._trainer[1] >= max_batch:
            return self._trainer[0]
        self._drop_trainer()
        import ctypes
        import torch
        p = self.params
        N, P, L, nl = (int(p[k]) for k in ("n_antennas", "n_pilots", "latent_dim", "n_layers"))
        flat = torch.cat([self._w[name].detach().reshape(-1) for name in layer_shapes(p)]).contiguous()
        out = ctypes.c_void_p()
        _lib.check(_lib.load().qce_vae_trainer_create(N, P, L, nl, int(p.get("n_pilot_convs", 0)), _MODE_CODE[p["vae_mode"]],
                                                      _lib.ptr(_widths(p)), _lib.ptr(flat), flat.numel(),
                                                      float(p.get("lr", 1e-3)), int(max_batch), _lib.IO_DEVICE,
                                                      flat.device.index or 0, ctypes.byref(out)))
        self._trainer = (out, int(max_batch))
        _lib._live["vae_net"].add(self)  # closed at exit while the HIP runtime is still up
        return out

    def _step_inputs(self, x, target, snr_db, index, eps):
        """The checked device arguments of one fused step: (x, n_x, target, n_target, snr, index, B, n_bits, eps)."""
        import torch
        p = self.params
        N, L, mode = int(p["n_antennas"]), int(p["latent_dim"]), p["vae_mode"]
        pin = int(p["n_pilots"]) if (mode != "genie" and int(p.get("n_pilot_convs", 0))) else 1
        if not _is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 2:
            raise TypeError("x must be a float32 CUDA tensor (n, P, 2N) or (n, 2N)")
        n_x = x.shape[0]
        x = x.contiguous()
        if x.numel() != n_x * pin * 2 * N:
            raise ValueError(f"x must be ({n_x}, {pin}, {2 * N}), got {tuple(x.shape)}")
        tgt = _f32_device(target.detach() if _is_tensor(target) else target, "target", 2 * N)
        B = n_x
        if index is not None:
            if not _is_tensor(index) or not index.is_cuda or index.dim() != 1:
                raise ValueError("index must be a CUDA tensor (B,)")
            B = index.shape[0]
            index = index.to(torch.int32).contiguous()
        elif tgt.shape[0] < B:
            raise ValueError(f"target has {tgt.shape[0]} rows for a batch of {B}")
        if B < 1 or n_x < 1 or tgt.shape[0] < 1:
            raise ValueError("empty batch")
        nb = 1.0
        if mode == "real":
            nb = _nbits(p["n_bits"])
            if snr_db is None:
                raise ValueError("mode 'real' needs snr_db, one value per target row")
            snr_db = torch.as_tensor(snr_db, device=x.device).to(torch.float64).reshape(-1).contiguous()
            if snr_db.shape[0] != tgt.shape[0]:
                raise ValueError(f"snr_db must have {tgt.shape[0]} entries, got {snr_db.shape[0]}")
        else:
            snr_db = None
        if eps is not None:
            eps = _f32_device(eps, "eps", L)
            if eps.shape[0] != B:
                raise ValueError(f"eps must be ({B}, {L}), got {tuple(eps.shape)}")
        return x, n_x, tgt, tgt.shape[0], snr_db, index, B, float(nb), eps

    def step_gradients(self, x, target, *, eps=None, seed=0, row_offset=0, snr_db=None, index=None):
        """(loss, rows, {name: grad}) of one training batch from the fused step kernel (``qce_vae_trainer_grads``:
        forward, ELBO, backward and the reduction over the batch in libqce.so, no update): the loss -mean_b l_b
        (float), the row ELBOs (B,) float64 and the gradient of the loss for every parameter, float32 tensors under the
        state-dict names.  x (n, P, 2N) (or (n, 2N)) and target (T, 2N) are float32 CUDA tensors; row b uses row
        ``index[b]`` of both (and of ``snr_db`` (T,), 'real' mode), or row b.  ``eps`` (B, L), or None: drawn as
        ``reparameterize`` draws it from ``seed`` / ``row_offset``.  For tests and for an optimiser of the caller's."""
        import torch
        self._check_fused()
        x, n_x, tgt, T, snr, index, B, nb, eps = self._step_inputs(x, target, snr_db, index, eps)
        tr = self._trainer_handle(B)
        dev, st = _dev_stream(x)
        shapes = layer_shapes(self.params)
        grads = torch.empty(sum(int(np.prod(s)) for s in shapes.values()), dtype=torch.float32, device=x.device)
        rows = torch.empty(B, dtype=torch.float64, device=x.device)
        loss = torch.empty(1, dtype=torch.float64, device=x.device)
        _lib.check(_lib.load().qce_vae_trainer_grads(tr, _lib.ptr(x), n_x, _lib.ptr(tgt), T, _lib.ptr(snr), _lib.ptr(index),
                                                     B, nb, _lib.ptr(eps), int(seed), int(row_offset), _lib.ptr(grads),
                                                     _lib.ptr(rows), _lib.ptr(loss), st))
        out, off = {}, 0
        for name, shape in shapes.items():
            n = int(np.prod(shape))
            out[name] = grads[off:off + n].view(shape)
            off += n
        return float(loss.item()), rows, out

    def _fused_step(self, x, target, *, eps=None, seed=0, row_offset=0, snr_db=None, index=None, slot=0, max_batch=None):
        """One fused training step (``qce_vae_trainer_step``) on the trainer's state; asynchronous.  The loss and the
        skip flag go to entry ``slot`` of the trainer's record (``_fused_read``)."""
        x, n_x, tgt, T, snr, index, B, nb, eps = self._step_inputs(x, target, snr_db, index, eps)
        tr = self._trainer_handle(max(B, max_batch or 0))
        _lib.check(_lib.load().qce_vae_trainer_step(tr, _lib.ptr(x), n_x, _lib.ptr(tgt), T, _lib.ptr(snr), _lib.ptr(index),
                                                    B, nb, _lib.ptr(eps), int(seed), int(row_offset), int(slot),
                                                    _dev_stream(x)[1]))
        return x, tgt, snr, index, eps  # what the step reads: the caller keeps them until it has synchronised

    def _fused_read(self, n):
        """(losses (n,) float64, skipped (n,) bool) of the trainer's record: one synchronising copy."""
        import torch
        losses, skipped = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int32)
        dev = self._device()
        _lib.check(_lib.load().qce_vae_trainer_read(self._trainer[0], _lib.ptr(losses), _lib.ptr(skipped), n,
                                                    torch.cuda.current_stream(dev).cuda_stream))
        return losses, skipped.astype(bool)

    def _fused_state(self):
        """({name: weight}, {name: exp_avg}, {name: exp_avg_sq}, step count) of the trainer, as fresh tensors."""
        import ctypes
        import torch
        dev = self._device()
        shapes = layer_shapes(self.params)
        n = sum(int(np.prod(s)) for s in shapes.values())
        flat = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)]
        step = ctypes.c_int64()
        _lib.check(_lib.load().qce_vae_trainer_get_state(self._trainer[0], _lib.ptr(flat[0]), _lib.ptr(flat[1]),
                                                         _lib.ptr(flat[2]), ctypes.byref(step),
                                                         torch.cuda.current_stream(dev).cuda_stream))
        out = []
        for f in flat:
            d, off = {}, 0
            for name, shape in shapes.items():
                k = int(np.prod(shape))
                d[name] = f[off:off + k].view(shape)
                off += k
            out.append(d)
        return out[0], out[1], out[2], int(step.value)

    def _fused_set_state(self, weights=None, exp_avg=None, exp_avg_sq=None, step=0):
        """Replace the trainer's weights / moments ({name: tensor}, or None: kept) and its step count."""
        import torch
        dev = self._device()
        flat = [None if d is None else torch.cat([d[name].detach().to(device=dev, dtype=torch.float32).reshape(-1)
                                                  for name in layer_shapes(self.params)]).contiguous()
                for d in (weights, exp_avg, exp_avg_sq)]
        _lib.check(_lib.load().qce_vae_trainer_set_state(self._trainer[0], _lib.ptr(flat[0]), _lib.ptr(flat[1]),
                                                         _lib.ptr(flat[2]), int(step),
                                                         torch.cuda.current_stream(dev).cuda_stream))
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
        self._drop_net()
        self._drop_trainer()
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
        if self._w is None:
            raise RuntimeError("no weights: call load_state_dict or from_checkpoint first")
        x = self._encode(x)
        return self._decode(x[:, :x.shape[-1] // 2])

    def _encode(self, x, sums=False):
        """Encoder output (B, 2L) = [mu | log_var_enc]: the pilot convolutions (not in 'genie' mode) and enc.
        ``sums``: the pilot convolutions (kernel size 1) written as weighted sums over the pilots.  The training
        forward uses that form: the library behind conv1d accumulates its weight gradient in an order that changes
        from call to call, and a training step is to be reproducible to the bit."""
        import torch.nn.functional as Fn
        p, w = self.params, self._w
        nl = int(p["n_layers"])
        if p["vae_mode"] != "genie":
            for i in range(int(p.get("n_pilot_convs", 0))):
                cw, cb = w[f"pre_pilot.conv{i}.weight"], w[f"pre_pilot.conv{i}.bias"]
                if sums:  # (B, out, in, 2N) summed over in
                    x = Fn.relu((cw[None, :, :, 0, None] * x[:, None, :, :]).sum(2) + cb[None, :, None])
                else:
                    x = Fn.relu(Fn.conv1d(x, cw, cb))
            x = x.squeeze(1)
        for i in range(nl):
            x = Fn.linear(x, w[f"enc.linear{i}.weight"], w[f"enc.linear{i}.bias"])
            if i < nl - 1:
                x = Fn.relu(x)
        return x

    def _decode(self, x):
        import torch.nn.functional as Fn
        w = self._w
        nl = int(self.params["n_layers"])
        for i in range(nl):
            x = Fn.linear(x, w[f"dec.linear{i}.weight"], w[f"dec.linear{i}.bias"])
            if i < nl - 1:
                x = Fn.relu(x)
        return x

    def forward(self, x, eps=None, *, seed=0, row_offset=0):
        """The sampling forward of ``DNN_VAE.forward`` (:272-291): (enc (B, 2L) = [mu | log_var_enc], dec (B, N) =
        log_var_dec) with z = ``reparameterize(enc, eps, seed=..., row_offset=...)`` between encoder and decoder."""
        if self._w is None:
            raise RuntimeError("no weights: call load_state_dict, from_checkpoint or train first")
        enc = self._encode(x, sums=True)
        return enc, self._decode(reparameterize(enc, eps, seed=seed, row_offset=row_offset))

    # ------------------------------------------------------------------ training
    def _snr_scaling(self):
        p = self.params
        if not p.get("snr_scale", False):
            return None
        s = np.linspace(1, p["snr_scale_fac"], len(p["snrs"]))  # :18-20
        return s / np.sum(s)

    def _check_fused(self):
        """The refusals of the fused training step alone (``qce_vae_trainer_create`` repeats them)."""
        p = self.params
        if not p.get("zeromean", True):
            raise ValueError(ZEROMEAN_MESSAGE)
        N, P, L = int(p["n_antennas"]), int(p["n_pilots"]), int(p["latent_dim"])
        pilot_vector(None, N)
        if N == 256:
            raise NotImplementedError("n_antennas = 256 is not covered by the fused training step: the activations of 16 "
                                      "rows do not fit the LDS of one workgroup (train with fused=False)")
        if P > MAX_PILOTS:
            raise NotImplementedError(f"at most {MAX_PILOTS} pilots, got {P}")
        if L < 1 or L > MAX_LATENT:
            raise NotImplementedError(f"latent_dim must lie in [1, {MAX_LATENT}], got {L}")
        need = fused_step_lds_bytes(p)
        if need > FUSED_STEP_LDS_LIMIT:
            raise NotImplementedError(f"the fused training step needs {need} bytes of LDS per workgroup for this network, "
                                      f"it covers up to {FUSED_STEP_LDS_LIMIT} (train with fused=False)")

    def _check_trainable(self, h_test, fused=False):
        """The refusals of ``train``, before anything is uploaded."""
        p = self.params
        if not p.get("zeromean", True):
            raise ValueError(ZEROMEAN_MESSAGE)
        N, P, L = int(p["n_antennas"]), int(p["n_pilots"]), int(p["latent_dim"])
        pilot_vector(None, N)
        if L < 1 or L > MAX_LATENT:
            raise NotImplementedError(f"latent_dim must lie in [1, {MAX_LATENT}], got {L}")
        if p["vae_mode"] == "real":
            nb = _nbits(p["n_bits"])
            if not np.isinf(nb) and p.get("quantizer_type", "uniform") != "uniform":
                raise NotImplementedError("the 'real' loss needs the uniform quantiser's Bussgang gain (:328-331)")
            if not np.isinf(nb) and nb > MAX_REAL_BITS:
                raise NotImplementedError(f"the 'real' loss covers uniform quantisers up to {MAX_REAL_BITS} bits")
            if P > 1:
                raise NotImplementedError("vae_mode 'real' trains with one pilot: the reference transforms the whole "
                                          "row of length P N and its encoder takes 2 N inputs")
        if fused:
            self._check_fused()
        if h_test is None:
            raise UnboundLocalError(HTEST_MESSAGE)  # the reference's first validation pass (:132)

    def _init_weights(self, gen):
        """Fresh leaf tensors under the reference's names, drawn as nn.Linear / nn.Conv1d (kernel size 1) draw
        theirs: weight and bias uniform in +-1 / sqrt(fan_in)."""
        import torch
        dev = self._device()
        w = {}
        for name, shape in layer_shapes(self.params).items():
            fan_in = shape[1] if name.endswith(".weight") else w[name[:-4] + "weight"].shape[1]
            bound = 1.0 / np.sqrt(fan_in)
            t = (torch.rand(shape, generator=gen, device=dev, dtype=torch.float32) * 2 - 1) * bound
            w[name] = t.requires_grad_(True)
        self._drop_net()
        self._drop_trainer()
        self._w = w

    def _train_data(self, h_dev, snr_list, seed, row_offset):
        """(encoder input, target, per-row SNRs) of one epoch for the channels h_dev, on the device."""
        p = self.params
        N, mode = int(p["n_antennas"]), p["vae_mode"]
        if mode == "genie":
            f = observe.encoder_features(h_dev, N, True).reshape(-1, 2 * N)
            return f, f, None
        feat = "fft" if (mode == "real" or p.get("fft_pre", True)) else "raw"
        x, snrs = observe.get_observation_nbit_randSNR(h_dev, snr_list, p.get("A"), p["n_bits"], p.get("quantizer"),
                                                       self._snr_scaling(), seed=seed, row_offset=row_offset,
                                                       features=feat)
        if mode == "real":
            return x, x.reshape(-1, 2 * N), snrs
        return x, None, None

    def train(self, h_train, h_test, snr_list, *, seed=0, file_vae=None, fused=False):
        """The reference's training loop (:15-154) on the device; returns (losses_all, losses_all_test), the clipped
        epoch means of the training and validation loss.  ``params`` additionally needs lr, batch_size, epochs,
        snr_scale (and snr_scale_fac, snrs), and for the default checkpoint name sim_id, model_type, n_paths, n_train.
        The trained weights stay in the object (``forward_nosamp`` / ``estimate_from_y`` work at once) and are saved
        after every epoch to ``file_vae`` (default: the reference's name pattern), a file ``from_checkpoint`` reads.
        ``seed`` keys every draw: initial weights, batches, observations and eps.

        ``fused``: every training step runs as two kernels of libqce.so (``k_vae_step``: gather, forward, ELBO and
        backward; ``k_vae_update``: reduction, skip rule, Adam; csrc/qce_vae_step.hip) on weights and Adam state the
        library holds, and the host reads the losses once per epoch.  Same initial weights, batches, observations and
        eps as the default loop; N = 256 and networks beyond 160 KiB of LDS per workgroup are refused."""
        self._check_trainable(h_test, fused)
        import torch
        p = self.params
        mode, N, bs = p["vae_mode"], int(p["n_antennas"]), int(p["batch_size"])
        dev = self._device()
        h_tr, h_te = (torch.as_tensor(h if _is_tensor(h) else np.array(h, dtype=np.complex128), device=dev)
                      .to(torch.complex128).reshape(-1, N).contiguous() for h in (h_train, h_test))
        n_train, n_test, epochs = h_tr.shape[0], h_te.shape[0], int(p["epochs"])
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        self._init_weights(gen)
        opti = torch.optim.Adam(list(self._w.values()), lr=p["lr"])
        if fused:
            self._trainer_handle(bs)  # takes a copy of the initial weights; the optimiser above only shapes the checkpoint
        if file_vae is None:
            file_vae = (f'results/vae/saves/VAE{p["vae_mode"]}_{p["sim_id"]}_{p["model_type"]}_paths={p["n_paths"]}_ant='
                        f'{p["n_antennas"]}_ntrain={p["n_train"]}.pt')  # :76-78
        p["file_vae"] = file_vae
        nb = _nbits(p["n_bits"])

        t_train = t_test = None
        if mode == "noisy":
            t_train = observe.encoder_features(h_tr, N, True).reshape(-1, 2 * N)
            t_test = observe.encoder_features(h_te, N, True).reshape(-1, 2 * N)
        # validation observations: drawn once, from rows beyond every training epoch's
        x_te, tt, snr_te = self._train_data(h_te, snr_list, seed, epochs * n_train)
        t_test = tt if tt is not None else t_test
        x_tr, tt, snr_tr = self._train_data(h_tr, snr_list, seed, 0) if mode == "genie" else (None, None, None)
        t_train = tt if tt is not None else t_train

        drawn = [0]  # rows of eps drawn so far: every forward takes fresh counters

        def loss_of(x_all, t_all, snr_all, n_rows):
            # the first batch of a fresh shuffle (next(iter(dataloader))): bs distinct, uniformly drawn rows
            idx = torch.randperm(n_rows, generator=gen, device=dev)[:bs]
            enc, dec = self.forward(x_all.index_select(0, idx), seed=seed, row_offset=drawn[0])
            drawn[0] += bs
            return elbo_loss(enc, dec, t_all, mode=mode, n_bits=nb, snr_db=snr_all, index=idx.to(torch.int32))

        losses_all, losses_all_test = [], []
        for epoch in range(epochs):
            if mode != "genie":
                x_tr, tt, snr_tr = self._train_data(h_tr, snr_list, seed, epoch * n_train)
                t_train = tt if tt is not None else t_train
            loss_epoch = []
            if fused:
                loss_epoch = self._fused_epoch(x_tr, t_train, snr_tr, n_train, bs, gen, seed, drawn)
            for _ in range(0 if fused else n_train // bs):
                opti.zero_grad()
                loss = loss_of(x_tr, t_train, snr_tr, n_train)
                val = float(loss.detach())  # the skip rule's host read (:120)
                if np.isnan(val) or val > LOSS_SKIP:
                    continue
                loss.backward()
                opti.step()
                loss_epoch.append(val)
            if not loss_epoch or np.isnan(np.mean(loss_epoch)):
                continue
            losses_all.append(np.clip(np.mean(loss_epoch), -np.inf, LOSS_SKIP))
            optim_state = self._fused_pull(opti) if fused else opti.state_dict()
            with torch.no_grad():
                loss_test = [loss_of(x_te, t_test, snr_te, n_test) for _ in range(n_test // bs)]
                loss_test = torch.stack(loss_test).cpu().numpy().astype(np.float64) if loss_test else np.full(1, np.nan)
                losses_all_test.append(np.clip(np.mean(loss_test), -np.inf, LOSS_SKIP))
            parent = os.path.dirname(file_vae)
            if parent:
                os.makedirs(parent, exist_ok=True)
            torch.save({"model": {k: v.detach() for k, v in self._w.items()}, "optim": optim_state,
                        "loss_all": losses_all, "epoch": epoch, "params": p}, file_vae)
        for v in self._w.values():
            v.requires_grad_(False)
        self._drop_net()  # the optimiser has updated the weights in place
        self._drop_trainer()
        return losses_all, losses_all_test

    def _fused_epoch(self, x_all, t_all, snr_all, n_rows, bs, gen, seed, drawn):
        """The training steps of one epoch on the fused step (two kernels each, no host read); returns the losses of
        the steps that were not skipped, from one read of the trainer's record per FUSED_STEP_SLOTS steps.  The
        batches and the eps counters are those of the unfused loop."""
        import torch
        dev = x_all.device
        if snr_all is not None:
            snr_all = torch.as_tensor(snr_all, device=dev).to(torch.float64).reshape(-1).contiguous()
        steps, kept = n_rows // bs, []
        for s0 in range(0, steps, FUSED_STEP_SLOTS):
            n = min(FUSED_STEP_SLOTS, steps - s0)
            alive = []  # the steps' inputs, until the read below has synchronised
            for s in range(n):
                idx = torch.randperm(n_rows, generator=gen, device=dev)[:bs].to(torch.int32)
                alive.append(self._fused_step(x_all, t_all, snr_db=snr_all, index=idx, seed=seed, row_offset=drawn[0],
                                              slot=s, max_batch=bs))
                drawn[0] += bs
            losses, skipped = self._fused_read(n)
            kept += [float(np.float32(v)) for v, sk in zip(losses, skipped) if not sk]
        return kept

    def _fused_pull(self, opti):
        """Copy the trainer's weights into ``_w`` (in place) and return its Adam state as a state dict of ``opti``."""
        import torch
        w, m, v, step = self._fused_state()
        with torch.no_grad():
            for name, t in self._w.items():
                t.copy_(w[name])
        self._drop_net()
        sd = opti.state_dict()
        if step > 0:
            sd["state"] = {i: {"step": torch.tensor(float(step)), "exp_avg": m[name], "exp_avg_sq": v[name]}
                           for i, name in enumerate(self._w)}
        return sd

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

    # ------------------------------------------------------------------ fused forward
    def _net_call(self, y, h, snr=None, return_mu=False, want_lv=True):
        """One ``qce_vae_net_forward``: (lv, mu, h_hat), each None when not asked for (h_hat with ``snr``).  numpy
        arrays go through the library's host staging, CUDA tensors are used in place on the current stream."""
        p = self.params
        if not p.get("zeromean", True):
            raise ValueError(ZEROMEAN_MESSAGE)
        N, P, L = int(p["n_antennas"]), int(p["n_pilots"]), int(p["latent_dim"])
        genie = p["vae_mode"] == "genie"
        x, nb, other = None, 1.0, False
        if snr is not None:  # the refusals of the unfused path, before anything is uploaded or launched
            x = pilot_vector(p.get("A"), N)
            nb = _nbits(p["n_bits"])
            qt = p.get("quantizer_type", "uniform")
            if nb != 1.0 and not np.isinf(nb) and qt == "lloyd":
                raise TypeError(LLOYD_MESSAGE)
            if x.size != P:
                raise ValueError(f"A has {x.size} pilots, n_pilots is {P}")
            other = nb != 1.0 and not np.isinf(nb) and qt != "uniform"  # the gain stays 0 (:421-426): h = 0
        if genie and h is None:
            raise ValueError("vae_mode 'genie' encodes the true channel: pass h")
        tensors = _is_tensor(y) or (genie and _is_tensor(h))
        if tensors:
            import torch
            dev = y.device if _is_tensor(y) else h.device
            if dev.type != "cuda":
                dev = self._device()

            def prep(v, cols):
                v = torch.as_tensor(v, device=dev).to(torch.complex128)
                return v.reshape(v.numel() // cols, cols).contiguous()

            def new(shape, dtype):
                return torch.empty(shape, dtype={"f": torch.float32, "c": torch.complex128}[dtype], device=dev)
            io, stream = _lib.IO_DEVICE, torch.cuda.current_stream(dev).cuda_stream
        else:
            def prep(v, cols):
                v = np.ascontiguousarray(v, dtype=np.complex128)
                return v.reshape(v.size // cols, cols)

            def new(shape, dtype):
                return np.empty(shape, dtype={"f": np.float32, "c": np.complex128}[dtype])
            io, stream = _lib.IO_HOST, None
        net = self._net_handle()
        y_c = None if (genie and y is None) else prep(y, P * N)
        src = prep(h, N) if genie else y_c
        B = int(src.shape[0])
        if y_c is not None and int(y_c.shape[0]) != B:
            raise ValueError(f"y has {int(y_c.shape[0])} rows, h has {B}")
        lv = new((B, N), "f") if want_lv else None
        mu = new((B, L), "f") if return_mu else None
        hh = None
        if snr is not None:
            hh = new((B, N), "c")
            if other or not B:
                hh[...] = 0
        run_lmmse = snr is not None and not other
        if B and (want_lv or return_mu or run_lmmse):
            _lib.check(_lib.load().qce_vae_net_forward(
                net, _lib.ptr(src), int(bool(p.get("fft_pre", True))), B, _lib.ptr(mu) if return_mu else None,
                _lib.ptr(lv) if want_lv else None, _lib.ptr(y_c) if run_lmmse else None,
                _lib.ptr(x) if run_lmmse else None, float(snr) if run_lmmse else 0.0, nb,
                _lib.ptr(hh) if run_lmmse else None, io, stream))
        return lv, mu, hh

    def forward_fused(self, y, h=None, *, return_mu=False):
        """Decoder log-variances (B, N) float32 from the raw observations y (B, P N) complex (``h`` (B, N): the true
        channels, which a 'genie' network encodes instead), computed by one kernel of libqce.so (``k_vae_net``);
        ``return_mu``: (lv, mu (B, L) float32).  numpy in, numpy out; CUDA tensor in, tensor out (asynchronous on
        the current stream)."""
        lv, mu, _ = self._net_call(y, h, return_mu=return_mu)
        return (lv, mu) if return_mu else lv

    def estimate_from_y(self, y, snr, h=None, *, fused=False):
        """Channel estimates (B, N) for observations y (B, P N); any B >= 1.  ``h``: the true channels, needed by
        vae_mode 'genie' only.  numpy in, numpy out; CUDA tensor in, tensor out.  ``fused``: the network runs
        inside libqce.so (``qce_vae_net_forward``), two launches per chunk instead of the torch calls."""
        if fused:
            return self._net_call(y, h, snr=snr, want_lv=False)[2]
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

    def eval(self, h_eval, y_eval, snr, h_train, *, fused=False):
        """(mse, rate, params) as the reference's eval (:157-228): MSE = sum |h_hat - h|^2 / h.size on the device,
        rate = the statistical lower bound with the global Bussgang pair of the training channels' sample covariance
        (g = h_hat / ||h_hat||^2; torch.var's n - 1 normalisation of the inner products).  ``fused``: the estimates
        come from ``estimate_from_y(..., fused=True)``."""
        p = self.params
        h_eval = np.asarray(h_eval)
        B = h_eval.shape[0]
        if p["vae_mode"] != "genie" and B % EVAL_BATCH == 1:
            raise IndexError(BATCH1_MESSAGE)
        import torch
        if fused:
            dev = self._device()
            hh = self._net_call(torch.as_tensor(y_eval, device=dev),
                                torch.as_tensor(h_eval, device=dev) if p["vae_mode"] == "genie" else None,
                                snr=snr, want_lv=False)[2]
        else:
            hh = self._estimate(y_eval, snr, h_eval)
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


def forward_fused(model, y, h=None, *, return_mu=False):
    """``model.forward_fused(y, h, return_mu=...)`` for a ``VAE_nbit`` with weights: the decoder log-variances (B, N)
    float32 of the raw observations, from one kernel of libqce.so (csrc/qce_vae_net.hip)."""
    return model.forward_fused(y, h, return_mu=return_mu)
