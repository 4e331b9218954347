"""MI355X-native Bussgang-GMM channel estimator (drop-in for the estimate path of
benediktfesl/Quantized_Channel_Estimation, modules/gmm_cplx_bussgang.py).

The compute path is libqce.so (hand-written HIP for gfx950, include/qce.h) bound through
ctypes; there is no CPU fallback.
"""
from .gmm import GaussianMixtureCplx, Gmm_nbit, Gmm_quant, mp_gmm  # noqa: F401
from .mofa import Mofa  # noqa: F401
from .kmeans import DeviceKMeans  # noqa: F401
from . import baselines, covrec, experiment, inputs, kmeans, observe, rate, scm, vae  # noqa: F401
from .covrec import est_cov_from_quant, quant_moments, recover_covariances  # noqa: F401
from .observe import encoder_features, get_observation_nbit_randSNR  # noqa: F401
from .vae import VAE_nbit, elbo_loss, forward_fused, lmmse_from_decoder, reparameterize  # noqa: F401

__all__ = ["Gmm_nbit", "Gmm_quant", "GaussianMixtureCplx", "mp_gmm", "Mofa", "DeviceKMeans", "kmeans", "VAE_nbit", "lmmse_from_decoder", "elbo_loss", "reparameterize", "forward_fused", "est_cov_from_quant", "quant_moments", "recover_covariances", "get_observation_nbit_randSNR", "encoder_features", "baselines", "covrec", "experiment", "inputs", "observe", "rate", "scm", "vae"]
