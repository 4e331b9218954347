"""The float64 restatement of one VAE training step (tests/vae_step_ref.py) against the reference's own float32 loss and
autograd parameter gradients (tests/golden/vae_train.npz, the two seeded networks), and the refusals of the fused step
that need no GPU.

Bound: 16 e32, e32 being the reference's own float32-vs-float64 difference on that quantity (relative for the loss,
relative Frobenius per gradient tensor): the yardstick of test_autograd_parameter_gradients_match_reference.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_fro
import vae_step_ref as S

NET_TAGS = ["net_noisy_n16p2", "net_real_n64"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "vae_train.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "vae_train_meta.json")) as fh:
        return json.load(fh)


def net_case(fx, meta, tag):
    """(case, weights, x, t, eps, snr) of a fixture network."""
    c = meta["net_cases"][tag]
    pre = tag + "__w__"
    w = {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}
    snr = fx[tag + "__snr"] if c["mode"] == "real" else None
    return c, w, fx[tag + "__x"], fx[tag + "__t"], fx[tag + "__eps"], snr


@pytest.mark.parametrize("tag", NET_TAGS)
def test_step_restatement_matches_reference(fx, meta, tag):
    c, w, x, t, eps, snr = net_case(fx, meta, tag)
    loss, rows, grads = S.loss_and_grads(w, x, t, eps, c["mode"], c["n_bits"], snr)
    l32 = float(fx[tag + "__loss32"])
    e_loss = abs(loss - l32) / abs(l32)
    print(tag, "loss %.3g of e32 %.3g" % (e_loss, c["e32_loss"]))
    assert e_loss <= 16 * c["e32_loss"]
    assert set(grads) == set(c["e32"])
    worst = {k: rel_fro(fx[f"{tag}__g32__{k}"].astype(np.float64), grads[k]) / c["e32"][k] for k in grads}
    print(tag, "gradient error in units of e32:", {k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 16, k
    # the reference's float64 run: the same formulas, so far closer than its float32 run
    for k in grads:
        assert rel_fro(fx[f"{tag}__g64__{k}"], grads[k]) <= 16 * c["e32"][k], k


def test_adam_restatement_first_step_moves_by_lr():
    """After one step from zero moments every weight with a non-zero gradient moves by lr (bias-corrected m / sqrt(v)
    is the gradient's sign, up to eps)."""
    rng = np.random.default_rng(3)
    w = {"a": rng.standard_normal((3, 4)), "b": rng.standard_normal(3)}
    g = {k: rng.standard_normal(v.shape) for k, v in w.items()}
    z = {k: np.zeros_like(v) for k, v in w.items()}
    w2, m2, v2, t = S.adam(w, z, z, g, 0, 1e-2)
    assert t == 1
    for k in w:
        assert np.allclose(w2[k], w[k] - 1e-2 * np.sign(g[k]), rtol=0, atol=1e-8)
        assert np.allclose(m2[k], 0.1 * g[k]) and np.allclose(v2[k], 1e-3 * g[k] ** 2)


def _params(**kw):
    p = dict(n_antennas=16, n_pilots=1, latent_dim=4, n_layers=3, n_pilot_convs=0, vae_mode="noisy", fft_pre=True,
             zeromean=True, apply_batchnorm=False, n_bits=1, quantizer_type="uniform", quantizer=None, A=None,
             eval_rate=False, device=0, lr=2e-2, batch_size=128, epochs=1, snr_scale=False, snrs=[0], sim_id="t",
             model_type="scm", n_paths=1, n_train=128)
    p.update(kw)
    return p


# N = 256; L = 129; a network over the LDS limit (N = 128, four pilots through two convolutions, eight layers)
REFUSED = [dict(n_antennas=256), dict(latent_dim=129),
           dict(n_antennas=128, n_pilots=4, n_pilot_convs=2, n_layers=8, latent_dim=128)]


@pytest.mark.parametrize("kw", REFUSED)
def test_fused_train_refusals_need_no_gpu(kw):
    from quantized_channel_estimation_amd import vae
    p = _params(**kw)
    h = np.zeros((4, p["n_antennas"]), dtype=complex)
    with pytest.raises(NotImplementedError):
        vae.VAE_nbit(p).train(h, h, [0], fused=True)


def test_lds_refusal_states_the_need():
    from quantized_channel_estimation_amd import vae
    p = _params(**REFUSED[2])
    need = vae.fused_step_lds_bytes(p)
    assert need > vae.FUSED_STEP_LDS_LIMIT
    with pytest.raises(NotImplementedError, match=str(need)):
        vae.VAE_nbit(p)._check_fused()
    assert vae.fused_step_lds_bytes(_params(n_antennas=64, latent_dim=16, n_layers=4)) <= vae.FUSED_STEP_LDS_LIMIT


def test_unfused_refusals_are_unchanged():
    """What train refuses without fused stays refused with it, with the same exception."""
    from quantized_channel_estimation_amd import vae
    h = np.zeros((4, 16), dtype=complex)
    for fused in (False, True):
        with pytest.raises(ValueError, match="too many values to unpack"):
            vae.VAE_nbit(_params(zeromean=False)).train(h, h, [0], fused=fused)
        with pytest.raises(NotImplementedError):
            vae.VAE_nbit(_params(vae_mode="real", n_bits=3, quantizer_type="lloyd")).train(h, h, [0], fused=fused)
        with pytest.raises(NotImplementedError):
            vae.VAE_nbit(_params(vae_mode="real", n_pilots=2, n_pilot_convs=1)).train(h, h, [0], fused=fused)
        with pytest.raises(UnboundLocalError):
            vae.VAE_nbit(_params(vae_mode="genie")).train(h, None, [0], fused=fused)


def test_c_abi_refuses_trainer_shapes_before_any_launch():
    """qce_vae_trainer_create refuses on its arguments, before the first HIP call: the same cases through the C ABI,
    with the library's shape-refusal code, and the LDS need in the message."""
    import ctypes
    from quantized_channel_estimation_amd import _lib, vae
    lib = _lib.load()
    buf = np.zeros(4, dtype=np.float32)  # never read: every call below is refused before the weights are touched

    def create(p):
        out = ctypes.c_void_p()
        rc = lib.qce_vae_trainer_create(p["n_antennas"], p["n_pilots"], p["latent_dim"], p["n_layers"],
                                        p["n_pilot_convs"], 1, _lib.ptr(vae._widths(p)), _lib.ptr(buf), 4, 1e-3, 128,
                                        _lib.IO_HOST, 0, ctypes.byref(out))
        assert not out.value
        return rc

    for kw in REFUSED:
        assert create(_params(**kw)) == _lib.QCE_ENOTIMPL
    msg = lib.qce_last_error().decode()
    assert str(vae.fused_step_lds_bytes(_params(**REFUSED[2]))) in msg and "LDS" in msg
    assert create(_params(n_antennas=48)) == _lib.QCE_ENOTIMPL
    assert create(_params(n_pilots=5, n_pilot_convs=1)) == _lib.QCE_ENOTIMPL
    assert create(_params()) == _lib.QCE_EARG  # the widths imply more than 4 weights
