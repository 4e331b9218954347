"""Drop-in estimator classes: ``Gmm_nbit`` / ``Gmm_quant`` / ``GaussianMixtureCplx``.

Same constructor, attributes and estimate-side methods as the reference's
``modules.gmm_cplx_bussgang.Gmm_nbit`` (gmm_cplx_bussgang.py:85-435) and
``modules.gmm_cplx_quant.Gmm_quant`` (gmm_cplx_quant.py:85-457), so the experiment scripts'
estimate loop (``mp_gmm(obj, *args)``, Bussgang_GMM.py:16-17, :284-289) runs unchanged.  All
arithmetic of ``estimate_from_y`` / ``predict_proba_cplx`` / ``_predict_cplx`` runs in libqce.so
on the GPU; this module only orchestrates and mirrors the reference's state mutations
(``gm.means_``, ``gm.covariances_``, ``gm.precisions_cholesky_``, ``gm.n_features_in_`` become the
observation-domain model of the last SNR, :262-313).

Models come from the device EM ``fit`` (:96-163, :437-790; ``_em.py``), from a reference-fitted
object (``from_reference``), or from ``from_params``.
"""
import copy
import numbers
import warnings

import numpy as np

from . import _lib
from .covrec import check_solver
from .kmeans import check_kmeans_option

try:  # the reference keeps its hyper-parameters and fitted weights in an sklearn object (:86-87)
    from sklearn.mixture import GaussianMixture as _SkGaussianMixture
except Exception:  # pragma: no cover - sklearn is part of the image
    _SkGaussianMixture = None


_MIRRORED = ("means_", "covariances_", "precisions_cholesky_")


def _materialize(gm):
    """Fetch the observation-domain state a previous estimate left pending (see _mirror)."""
    pend = gm.__dict__.pop("_qce_pending", None)
    if pend is not None:
        pend(gm)


def _drop_pending(gm):
    """Forget a pending state mirror (and the device model its closure keeps alive) without fetching it."""
    if hasattr(gm, "__dict__"):
        gm.__dict__.pop("_qce_pending", None)


if _SkGaussianMixture is not None:
    class _GaussianMixtureState(_SkGaussianMixture):
        """sklearn's GaussianMixture parameter bag (the reference keeps its fitted state in one,
        gmm_cplx_bussgang.py:86-87) whose observation-domain attributes ``means_``, ``covariances_``
        and ``precisions_cholesky_`` — rewritten by every estimate (:262-264, :288, :309-313) — are
        copied from the device only when first read: an estimate does not pay for ~50 MB of table
        transfers that the scripts never look at."""

        def __getattr__(self, name):
            if name in _MIRRORED and "_qce_pending" in self.__dict__:
                _materialize(self)
                return self.__dict__[name]
            raise AttributeError(name)

        def __getstate__(self):
            _materialize(self)
            return super().__getstate__()
else:  # pragma: no cover
    _GaussianMixtureState = None


def _owns_chain(a):
    """True if every array in a's base chain is an ndarray and the last one owns its data (no foreign buffer that
    could change behind a read-only view)."""
    while isinstance(a, np.ndarray):
        if a.base is None:
            return a.flags.owndata
        a = a.base
    return isinstance(a, bytes)  # immutable Python buffer


def _immutable(a):
    """A read-only array whose data cannot change through another object: itself and every array of its base chain
    read-only, the chain ending in memory it owns (a read-only view of a writable base can still change)."""
    if not isinstance(a, np.ndarray) or not _owns_chain(a):
        return False
    while isinstance(a, np.ndarray):
        if a.flags.writeable:
            return False
        a = a.base
    return True


def _fingerprint(*arrays):
    """Content key of the model parameters (in-place edits of means_cplx / covs_cplx / weights_
    invalidate the device model, as the reference re-reads them on every estimate_from_y)."""
    try:
        import xxhash
        hs = xxhash.xxh3_64()
    except Exception:  # pragma: no cover
        import hashlib
        hs = hashlib.blake2b(digest_size=8)
    for a in arrays:
        if a is None:
            hs.update(b"none")
            continue
        a = np.ascontiguousarray(a)
        hs.update(str((a.shape, a.dtype.str)).encode())
        hs.update(a.view(np.uint8).reshape(-1))
    return hs.hexdigest()


class _ParamBag:
    """Minimal stand-in for sklearn's GaussianMixture when sklearn is not importable."""

    def __init__(self, n_components=1, covariance_type="full", **kw):
        self.n_components = n_components
        self.covariance_type = covariance_type
        for k, v in kw.items():
            setattr(self, k, v)


def _mode_of(n_summands_or_proba, K):
    """Map the reference's mode argument (:197-242) to (mode, param).  Returns None for an empty
    top-n selection (the reference divides by an empty sum -> NaN rows)."""
    v = n_summands_or_proba
    if isinstance(v, int):  # bool and int, exactly the reference's isinstance test (:197)
        n = int(v)
        if n < 0:  # idx_sort[:n] with negative n keeps K + n entries
            n = max(K + n, 0)
        if n == 0:
            return None
        return (_lib.MODE_TOPN, float(n))
    if isinstance(v, str) and v == "all":
        return (_lib.MODE_ALL, 0.0)
    if isinstance(v, str):
        raise ValueError(f"unsupported n_summands_or_proba {v!r}")
    return (_lib.MODE_CUMP, float(v))  # floats and numpy integers take the probability branch (:229)


def _nbits_of(n_bits):
    if isinstance(n_bits, str):
        # the reference's prepare compares the string with an int (uniform_quantizer.py via :281) and raises
        # this TypeError (golden: tests/golden/quirks.npz str_inf)
        raise TypeError("'<=' not supported between instances of 'str' and 'int'")
    return float(n_bits)


class Gmm_nbit:
    """Complex GMM with Bussgang-conditioned per-component LMMSE estimation on MI355X.

    Mirrors ``Gmm_nbit`` (gmm_cplx_bussgang.py:85-94): ``gm`` is the sklearn GaussianMixture
    parameter bag (``n_components``, ``covariance_type``, ``weights_`` ...), ``means_cplx``
    (K,N) and ``covs_cplx`` (K,N,N) the channel-domain model.
    """

    def __init__(self, *gmm_args, device=0, precision="f64", fourier_pilots=False, kmeans="host", **gmm_kwargs):
        if _SkGaussianMixture is not None:
            self.gm = _GaussianMixtureState(*gmm_args, **gmm_kwargs)
        else:
            self.gm = _ParamBag(*gmm_args, **gmm_kwargs)
        self.means_cplx = None
        self.covs_cplx = None
        self.fft_covs = None
        self.fft_means = None
        self.chol = None
        self.params = dict()
        self.F2 = None
        self.device = device
        # arithmetic of the dense 'all' mode: "f64" = the reference's complex128 (FP64 MFMA products and
        # accumulation, the default), "fast" = fp16 two-term split products with fp32 accumulation (opt-in), "int8" =
        # int8_slices digit planes of the tables on the i8 MFMA for quantised observations (opt-in; FP64 elsewhere)
        self.precision = precision
        self.int8_slices = 7
        # opt-in: a (block-)circulant model observed through A = kron(x, I_N), 2..4 pilots, is estimated per DFT bin
        # (P x P blocks) instead of densely at M = P N
        self.fourier_pilots = bool(fourier_pilots)
        # K-means initialisation of fit: "host" = sklearn's KMeans as in the reference (the default), "device" = the
        # same seeds and the Lloyd loop on the resident training data (kmeans.DeviceKMeans; opt-in), "device-seeded"
        # = the same, with the k-means++ seeds chosen on the device from pre-drawn uniforms (opt-in)
        self.kmeans = check_kmeans_option(kmeans)
        self.mirror_state = True
        self._dev = None
        self._dev_key = None
        self._state = None  # "obs" after an observation-domain prepare, "chan" for the fit-state model

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_reference(cls, ref, device=0, kmeans=None):
        """Adopt a fitted reference ``Gmm_nbit``/``Gmm_quant`` (e.g. a joblib-loaded object,
        Bussgang_GMM.py:270-278): reads means_cplx, covs_cplx and the sklearn parameter bag.  kmeans: the option of
        later fits (None: the one `ref` carries, else "host")."""
        obj = cls.__new__(cls)
        Gmm_nbit.__init__(obj, device=device, kmeans=getattr(ref, "kmeans", "host") if kmeans is None else kmeans)
        obj.gm = copy.deepcopy(ref.gm)
        if _GaussianMixtureState is not None and type(obj.gm) is _SkGaussianMixture:
            obj.gm.__class__ = _GaussianMixtureState
        for name in ("means_cplx", "covs_cplx", "fft_covs", "fft_means", "chol", "F2"):
            setattr(obj, name, copy.deepcopy(getattr(ref, name, None)))
        obj.params = copy.deepcopy(getattr(ref, "params", {}))
        if hasattr(ref, "recovery"):  # a Gmm_quant's option of later fits
            obj.recovery = check_solver(ref.recovery, "recovery")
        return obj

    @classmethod
    def from_params(cls, means_cplx, covs_cplx, weights, covariance_type="full", device=0, precision="f64",
                    fourier_pilots=False):
        covs = np.asarray(covs_cplx, dtype=complex)
        obj = cls(n_components=covs.shape[0], covariance_type=covariance_type, device=device, precision=precision,
                  fourier_pilots=fourier_pilots)
        obj.means_cplx = np.zeros(covs.shape[:2], complex) if means_cplx is None else np.asarray(means_cplx, complex)
        obj.covs_cplx = covs
        obj.gm.weights_ = np.asarray(weights, dtype=float)
        obj.gm.means_ = obj.means_cplx.copy()
        obj.gm.covariance_type = "full"
        return obj

    def fit(self, h, blocks=None, zero_mean=False):
        """EM training on the device (gmm_cplx_bussgang.py:96-163).

        'full': EM on h.  'circulant' / 'block-circulant': EM with diagonal covariances on the
        (block-)DFT of h, then C_k = F^H diag(c_k) F (:104-134).  'toeplitz' / 'block-toeplitz': the
        inverse-EM M-step (:792-826) with the partial DFT F2 (:143-163)."""
        from . import _em
        _drop_pending(self.gm)  # a previous estimate's lazy state mirror must not overwrite the new fit
        self.params["zero_mean"] = bool(zero_mean)
        h = np.asarray(h)
        ct = self.gm.covariance_type
        self._dev = None
        self._dev_key = None
        self._state = None
        if ct == "circulant":
            self.gm.covariance_type = "diag"
            N = h.shape[-1]
            F = np.fft.fft(np.eye(N, dtype=complex)) / np.sqrt(N)
            self.fit_cplx(np.fft.fft(h, axis=1) / np.sqrt(N))
            self.fft_covs = self.gm.covariances_
            self.fft_means = self.gm.means_
            self._fourier_params(F)
            self.gm.covariances_ = self.covs_cplx
        elif ct == "block-circulant":
            self.gm.covariance_type = "diag"
            n_1, n_2 = blocks
            F = np.kron(np.fft.fft(np.eye(n_1)) / np.sqrt(n_1), np.fft.fft(np.eye(n_2)) / np.sqrt(n_2))
            self.F2 = F
            self.fit_cplx(np.ascontiguousarray((F @ h.T).T))
            self._fourier_params(F)  # the reference leaves gm.covariances_ diagonal here (:118-134)
        elif ct == "full":
            self.fit_cplx(h)
            self.means_cplx = self.gm.means_.copy()
            self.covs_cplx = self.gm.covariances_.copy()
            self.chol = self.gm.precisions_cholesky_.copy()
        elif ct == "toeplitz":  # :143-151
            self.params["inv-em"] = True
            self.gm.covariance_type = "full"
            n_1 = h.shape[1]
            self.F2 = np.fft.fft(np.eye(2 * n_1))[:, :n_1] / np.sqrt(2 * n_1)
            self.fit_cplx(h)
            self.means_cplx = self.gm.means_.copy()
            self.covs_cplx = self.gm.covariances_.copy()
            self.chol = self.gm.precisions_cholesky_.copy()
        elif ct == "block-toeplitz":  # :152-163
            self.params["inv-em"] = True
            self.gm.covariance_type = "full"
            n_1, n_2 = blocks
            F2_1 = np.fft.fft(np.eye(2 * n_1))[:, :n_1] / np.sqrt(2 * n_1)
            F2_2 = np.fft.fft(np.eye(2 * n_2))[:, :n_2] / np.sqrt(2 * n_2)
            self.F2 = np.kron(F2_1, F2_2)
            self.fit_cplx(h)
            self.means_cplx = self.gm.means_.copy()
            self.covs_cplx = self.gm.covariances_.copy()
            self.chol = self.gm.precisions_cholesky_.copy()
        else:
            raise NotImplementedError(f"Fitting for covariance_type = {ct} is not implemented.")
        return self

    def _fourier_params(self, F):
        """Channel-domain model of a diagonal fit in the F basis (:109-117, :127-134)."""
        from . import _em
        c = np.asarray(self.gm.covariances_)
        self.means_cplx = self.gm.means_ @ F.conj()
        self.covs_cplx = np.einsum("ji,kj,jl->kil", F.conj(), c.astype(complex), F)
        self.chol = _em.precision_cholesky(self.covs_cplx, device=self.device)
        self.gm.covariance_type = "full"
        self.gm.means_ = self.means_cplx
        self.gm.precisions_cholesky_ = self.chol

    def fit_cplx(self, X, y=None):
        """gmm_cplx_bussgang.py:437-460."""
        self.fit_predict(X, y)
        return self

    def fit_predict(self, X, y=None):
        """gmm_cplx_bussgang.py:462-536: EM on the device, returns the component labels of X."""
        from . import _em
        return _em.fit_predict(self, X)

    # ------------------------------------------------------------------ pickling (pool.starmap, :282-287)
    def __getstate__(self):
        if hasattr(self.gm, "__dict__"):
            _materialize(self.gm)
        d = self.__dict__.copy()
        d["_dev"] = None
        d["_dev_key"] = None
        d["_state"] = None
        d.pop("_digest_cache", None)
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def __deepcopy__(self, memo):
        cls = self.__class__
        obj = cls.__new__(cls)
        memo[id(self)] = obj
        for k, v in self.__getstate__().items():
            setattr(obj, k, copy.deepcopy(v, memo))
        return obj

    # ------------------------------------------------------------------ device model
    def _device_model(self):
        if self.covs_cplx is None:
            raise ValueError("the model has no parameters (means_cplx / covs_cplx) yet")
        if getattr(self.gm, "covariance_type", "full") != "full":
            # every fit variant leaves covariance_type == 'full' (:116, :134, :144, :153); the
            # reference raises for anything else (:316-317)
            raise NotImplementedError(f"Estimation for covariance_type = {self.gm.covariance_type} is not implemented.")
        covs = np.asarray(self.covs_cplx)
        means = self.means_cplx
        w = np.asarray(self.gm.weights_, dtype=float)
        precision = getattr(self, "precision", "f64")
        slices = int(getattr(self, "int8_slices", 7)) if precision == "int8" else None
        pilots = bool(getattr(self, "fourier_pilots", False))  # getattr: objects pickled before the option existed
        key = (self._param_digest(covs, means, w), self.device, precision, slices, pilots)
        if self._dev is None or self._dev_key != key:
            self._dev = _lib.DeviceModel(means, covs, w, device=self.device)
            if precision != "f64":
                self._dev.set_precision(precision, **({} if slices is None else {"slices": slices}))
            if pilots:
                self._dev.set_fourier_pilots(True)
            self._dev_key = key
            self._state = None
        return self._dev

    def _param_digest(self, covs, means, w):
        """Content digest of the parameters (0.8 ms for the metric model's 8.4 MB of covariances).  Read-only arrays
        (``freeze_params``) cannot change in place, so while the same read-only objects are attached the digest
        is reused instead of re-hashed."""
        arrs = (covs, means, w)
        frozen = all(a is None or _immutable(a) for a in arrs)
        c = self.__dict__.get("_digest_cache")
        if frozen and c is not None and all(x is y for x, y in zip(c[0], arrs)):
            return c[1]
        d = _fingerprint(covs, means, w)
        self.__dict__["_digest_cache"] = (arrs, d) if frozen else None
        return d

    def freeze_params(self):
        """Mark means_cplx, covs_cplx and gm.weights_ read-only: estimates then skip the per-call content digest
        that detects in-place edits (the reference re-reads the arrays on every estimate_from_y).  Assigning new
        arrays still takes effect."""
        for name in ("means_cplx", "covs_cplx"):
            a = getattr(self, name, None)
            if isinstance(a, np.ndarray):
                if a.base is not None:  # a view: its memory can still change elsewhere -- freeze a private copy
                    a = a.copy()
                    setattr(self, name, a)
                a.flags.writeable = False
        wts = getattr(self.gm, "weights_", None)
        if isinstance(wts, np.ndarray):
            if wts.dtype != np.float64 or wts.base is not None:
                self.gm.weights_ = wts = wts.astype(np.float64, copy=True)
            wts.flags.writeable = False
        return self

    def _mirror(self, dev, M):
        """Reproduce the reference's mutation of ``self.gm`` (:262-264, :288, :309-313)."""
        if not self.mirror_state:
            return
        self.gm.n_features_in_ = M

        def fetch(gm, dev=dev):
            t = dev.tables(("means_y", "Cr", "P"))
            gm.__dict__.update(means_=t["means_y"], covariances_=t["Cr"], precisions_cholesky_=t["P"])

        if _GaussianMixtureState is not None and isinstance(self.gm, _GaussianMixtureState):
            for n in _MIRRORED:
                self.gm.__dict__.pop(n, None)
            self.gm.__dict__["_qce_pending"] = fetch  # read lazily (_GaussianMixtureState.__getattr__)
        else:
            fetch(self.gm)

    def _prepare(self, A, snr_dB, n_bits, quantizer_type, quantizer, allow_inf=True):
        dev = self._device_model()
        nb = _nbits_of(n_bits)
        qkind, thr, lab = _lib.QUANT_UNIFORM, None, None
        if nb != 1 and not np.isinf(nb):
            if quantizer_type == "uniform":
                qkind = _lib.QUANT_UNIFORM
                if nb > 8:  # uniform_quantizer.py:19 (the asymptotic step replaces J. Max's table)
                    warnings.warn("Optimal standard step size is unknown and thus approximated!")
            elif quantizer_type == "lloyd":
                qkind = _lib.QUANT_LLOYD
                if quantizer is None or quantizer[0] is None:
                    raise ValueError("lloyd quantizer needs (thresholds, labels, rho)")
                thr, lab = np.asarray(quantizer[0], float), np.asarray(quantizer[1], float)
            else:
                qkind = _lib.QUANT_OTHER
        if np.isinf(nb) and not allow_inf and quantizer_type == "lloyd":
            raise OverflowError("cannot convert float infinity to integer")
        dev.prepare(A, snr_dB, nb, qkind, thr, lab)
        self._state = "obs"
        return dev

    def _ensure_state(self):
        """Device model matching the current ``gm`` state: after an estimate it is the
        observation-domain model; before, the channel-domain model of the fit, which equals the
        prepare with A = I, sigma^2 = 0 and no quantisation (Cr = C)."""
        dev = self._device_model()
        if self._state is None:
            dev.prepare(None, float("inf"), float("inf"))
            self._state = "chan"
        return dev

    # ------------------------------------------------------------------ reference API
    def estimate_from_y(self, y, snr_dB, n_antennas, A=None, n_summands_or_proba=1, n_bits=1,
                        quantizer_type="uniform", quantizer=None):
        """gmm_cplx_bussgang.py:166-243 — returns h_est (B, N) complex128."""
        y = np.asarray(y)
        if y.ndim != 2:
            # the reference unpacks y.shape at :405 (golden: tests/golden/quirks.npz y1d)
            raise ValueError(f"not enough values to unpack (expected 2, got {y.ndim})")
        N = self.covs_cplx.shape[-1]
        if A is not None:
            A = np.asarray(A)
            if A.shape[0] == A.shape[1] and np.array_equal(A, np.eye(A.shape[0])):
                A = None  # identity: same arithmetic, fast path
        elif n_antennas != N:
            raise ValueError(f"n_antennas={n_antennas} does not match the model dimension {N}")
        dev = self._prepare(A, snr_dB, n_bits, quantizer_type, quantizer, allow_inf=self._allow_inf())
        M = dev.M
        if self.mirror_state:
            self._mirror(dev, M)
        mode = _mode_of(n_summands_or_proba, dev.K)
        B = y.shape[0]
        if mode is None:
            return np.full((B, N), np.nan + 0j)
        yc = np.ascontiguousarray(y, dtype=np.complex128)
        return dev.estimate(yc, mode[0], mode[1])

    def _allow_inf(self):
        return True

    def _predict_cplx(self, X):
        """gmm_cplx_bussgang.py:335-349."""
        dev = self._ensure_state()
        return dev.log_prob(X, want_lp=False, want_labels=True)[2]

    def predict_proba_cplx(self, X):
        """gmm_cplx_bussgang.py:351-367."""
        dev = self._ensure_state()
        return dev.log_prob(X, want_lp=False, want_proba=True)[1]

    def _estimate_weighted_log_prob(self, X):
        """gmm_cplx_bussgang.py:369-380."""
        dev = self._ensure_state()
        return dev.log_prob(X)[0]

    def _estimate_log_weights(self):
        """gmm_cplx_bussgang.py:382-383."""
        return np.log(self.gm.weights_)

    def _estimate_log_prob(self, X):
        """gmm_cplx_bussgang.py:385-386 (weighted minus log weights)."""
        return self._estimate_weighted_log_prob(X) - self._estimate_log_weights()

    def _estimate_log_prob_resp(self, X):
        """gmm_cplx_bussgang.py:632-656."""
        wlp = self._estimate_weighted_log_prob(X)
        from scipy.special import logsumexp
        norm = logsumexp(wlp, axis=1)
        with np.errstate(under="ignore"):
            return norm, wlp - norm[:, None]


class Gmm_quant(Gmm_nbit):
    """Estimate side of ``Gmm_quant`` (gmm_cplx_quant.py:85-457): same tables and arithmetic as
    ``Gmm_nbit`` (verified bit-identical).  Its prepare has no n_bits = inf
    branch (:300-327): inf goes through the uniform-quantiser gain, which is the identity, so the
    result is the same; with a Lloyd quantiser the reference overflows, which is mirrored."""

    def __init__(self, *gmm_args, device=0, precision="f64", fourier_pilots=False, kmeans="host", recovery="host",
                 **gmm_kwargs):
        super().__init__(*gmm_args, device=device, precision=precision, fourier_pilots=fourier_pilots, kmeans=kmeans,
                         **gmm_kwargs)
        # covariance recovery of fit's M-step: "host" = the NumPy algebra as in the reference (the default), "device" =
        # the scalar variance fits and the eigenvalue clips in libqce.so (covrec.variance_fits / eig_clip; opt-in)
        self.recovery = check_solver(recovery, "recovery")
        self.quantizer = None
        self.sigma2 = None
        self.n_bits = None
        self.quant_type = None
        self.covariances_quant = None
        self.eval_mode = False
        self.precisions_cholesky_quant = None

    def fit(self, h, n_bits, sigma2, quantizer, quant_type, blocks=None, zero_mean=False, _backend=None):
        """EM on quantised observations with covariance recovery (gmm_cplx_quant.py:103-189): 'full' (:155-159) and
        the inverse-EM 'toeplitz' / 'block-toeplitz' (:160-181, with the partial DFT F2), zero mean or with means;
        device E-step on covariances_quant and device moments, the recovery algebra on the host (_em_quant.py) or,
        with recovery="device", its variance fits and eigenvalue clips on the device.
        The covariance types the reference cannot fit end in the reference's own exception
        (_em_quant.reference_fit_error)."""
        from . import _em_quant
        _drop_pending(self.gm)
        self.params["zero_mean"] = bool(zero_mean)
        self.n_bits, self.sigma2, self.quantizer, self.quant_type = n_bits, sigma2, quantizer, quant_type
        ct = self.gm.covariance_type
        err = _em_quant.reference_fit_error(ct, self.gm.n_components, n_bits)
        if err is not None:
            raise err
        if ct == "toeplitz":  # :166-172
            self.params["inv-em"] = True
            self.gm.covariance_type = "full"
            n_1 = np.asarray(h).shape[1]
            self.F2 = np.fft.fft(np.eye(2 * n_1))[:, :n_1] / np.sqrt(2 * n_1)
        elif ct == "block-toeplitz":  # :173-181
            self.params["inv-em"] = True
            self.gm.covariance_type = "full"
            n_1, n_2 = blocks
            F2_1 = np.fft.fft(np.eye(2 * n_1))[:, :n_1] / np.sqrt(2 * n_1)
            F2_2 = np.fft.fft(np.eye(2 * n_2))[:, :n_2] / np.sqrt(2 * n_2)
            self.F2 = np.kron(F2_1, F2_2)
        elif ct != "full":
            raise NotImplementedError(f"Fitting for covariance_type = {ct} is not implemented.")
        self._dev = None
        self._dev_key = None
        self._state = None
        _em_quant.fit_predict(self, np.asarray(h), backend=_backend)  # _backend: tests' CPU stand-in
        self.means_cplx = self.gm.means_.copy()
        self.covs_cplx = self.gm.covariances_.copy()
        self.chol = self.gm.precisions_cholesky_.copy()
        return self

    def _allow_inf(self):
        return False

    def estimate_from_y(self, y, snr_dB, n_antennas, A=None, n_summands_or_proba=1, n_bits=1,
                        quantizer_type="uniform", quantizer=None):
        self.eval_mode = True  # gmm_cplx_quant.py:214
        return super().estimate_from_y(y, snr_dB, n_antennas, A, n_summands_or_proba, n_bits, quantizer_type,
                                       quantizer)


class GaussianMixtureCplx(Gmm_nbit):
    """The API name used by the project brief: ``estimate`` = ``estimate_from_y``,
    ``predict_proba`` = ``predict_proba_cplx``, ``predict`` = ``_predict_cplx``."""

    def estimate(self, *args, **kwargs):
        return self.estimate_from_y(*args, **kwargs)

    def predict_proba(self, X):
        return self.predict_proba_cplx(X)

    def predict(self, X):
        return self._predict_cplx(X)


def mp_gmm(obj, *args):
    """The reference's pool worker (Bussgang_GMM.py:16-17)."""
    return obj.estimate_from_y(*args)
