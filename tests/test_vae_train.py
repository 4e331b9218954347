"""Training side of the VAE estimator (quantized_channel_estimation_amd.vae: reparameterize, elbo_loss,
VAE_nbit.train; csrc/qce_vae_train.hip) against the reference's own loss and autograd gradients
(tests/golden/vae_train.npz, made by tests/golden/make_golden_vae_train.py) and against the float64 NumPy restatement
tests/vae_train_ref.py.

Bounds:

* restatement or kernel against the reference's float32 values: 16 e32, e32 being the reference's own
  float32-vs-float64 difference on that quantity (relative for the loss, relative Frobenius for a gradient tensor) --
  the end-to-end float32 margin of tests/test_vae.py;
* restatement against central differences of its own loss (float64, step 1e-6): relative Frobenius 1e-6;
* kernel against the restatement: row ELBOs relative Frobenius 1e-9 (the project's FP64 bar on the GPU); gradients and
  z element by element |got - ref| <= 2^-23 |ref| + 1e-12 max|ref|, one float32 rounding of an FP64 value, no element
  excluded;
* drawn eps: mean within 5 / sqrt(n) of 0 and variance within 5 sqrt(2 / n) of 1 (five standard errors), n = 2^16.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_fro
import vae_train_ref as R

LOSS_TAGS = ["noisy_b1_n16", "genie_b1_n64", "real_b1_n16", "real_b3_n64", "real_b2_n256", "real_inf_n64"]
NET_TAGS = ["net_noisy_n16p2", "net_real_n64"]
SNRS = [-10, -5, 0, 5, 10, 15, 20]
# mode, n_bits, N, L, B, index (None / "perm" / "dup"): one row, several workgroups with a ragged tail, the ends of the
# latent range, every lane layout (N = 16 ... 256), the longest gain sum, and gathered targets
SHAPE_CASES = [
    ("real", 2, 16, 4, 1, None),
    ("real", 3, 16, 4, 67, None),
    ("noisy", 1, 64, 1, 67, None),
    ("real", 8, 32, 128, 9, None),
    ("real", 4, 128, 5, 9, "perm"),
    ("genie", 1, 64, 16, 13, "dup"),
    ("real", np.inf, 256, 7, 3, "dup"),
]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "vae_train.npz"))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "vae_train_meta.json")) as fh:
        return json.load(fh)


def _loss_case(fx, meta, tag):
    c = meta["loss_cases"][tag]
    nb = np.inf if c["n_bits"] == "inf" else int(c["n_bits"])
    p = tag + "__"
    snr = fx[p + "snr"] if c["mode"] == "real" else None
    return c, nb, fx[p + "enc"], fx[p + "dec"], fx[p + "t"], snr


_ref_cache = {}


def _ref(key, enc, dec, t, mode, nb, snr, index=None):
    """(rows, g_enc, g_dec) of the restatement, computed once per case and shared (read-only)."""
    if key not in _ref_cache:
        out = (R.elbo_rows(enc, dec, t, mode, nb, snr, index),) + R.loss_grads(enc, dec, t, mode, nb, snr, index)
        for a in out:
            a.setflags(write=False)
        _ref_cache[key] = out
    return _ref_cache[key]


def _shape_inputs(ci):
    mode, nb, N, L, B, ix = SHAPE_CASES[ci]
    rng = np.random.default_rng(900 + ci)
    T = B if ix != "dup" else 5
    enc = (0.5 * rng.standard_normal((B, 2 * L))).astype(np.float32)
    dec = rng.standard_normal((B, N)).astype(np.float32)
    t = (np.sqrt(0.5) * rng.standard_normal((T, 2 * N))).astype(np.float32)
    snr = rng.choice(SNRS, T).astype(np.float64) if mode == "real" else None
    index = None if ix is None else (rng.permutation(B) if ix == "perm" else rng.integers(0, T, B)).astype(np.int32)
    return mode, nb, enc, dec, t, snr, index


def _elementwise_ok(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.all(np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-12 * np.max(np.abs(ref)))


def _train_params(mode, nb, **kw):
    from quantized_channel_estimation_amd import inputs
    snrs = [0, 10, 20]
    p = dict(n_antennas=16, n_pilots=1, latent_dim=4, n_layers=3, n_pilot_convs=0, vae_mode=mode, fft_pre=True,
             zeromean=True, apply_batchnorm=False, n_bits=nb, quantizer_type="uniform",
             quantizer=inputs.get_quantizer(snrs, nb, "uniform"), A=None, eval_rate=False, device=0, lr=2e-2,
             batch_size=128, epochs=4, snr_scale=False, snrs=snrs, sim_id="t", model_type="scm", n_paths=1, n_train=2048)
    p.update(kw)
    return p


# ---------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("tag", LOSS_TAGS)
def test_restatement_matches_reference(fx, meta, tag):
    c, nb, enc, dec, t, snr = _loss_case(fx, meta, tag)
    rows, g_enc, g_dec = _ref(tag, enc, dec, t, c["mode"], nb, snr)
    loss = -np.mean(rows)
    p = tag + "__"
    e_loss = abs(loss - float(fx[p + "loss32"])) / abs(loss)
    e_enc, e_dec = rel_fro(fx[p + "genc32"].astype(np.float64), g_enc), rel_fro(fx[p + "gdec32"].astype(np.float64), g_dec)
    print(tag, "loss %.3g enc %.3g dec %.3g of e32 %s" % (e_loss, e_enc, e_dec, c["e32"]))
    assert e_loss <= 16 * c["e32"]["loss"]
    assert e_enc <= 16 * c["e32"]["enc"]
    assert e_dec <= 16 * c["e32"]["dec"]
    # the float64 run of the reference: the same formulas up to its float32 gain accumulation
    assert abs(loss - float(fx[p + "loss64"])) / abs(loss) <= 16 * c["e32"]["loss"]


@pytest.mark.parametrize("tag", ["noisy_b1_n16", "real_b1_n16"])
def test_restatement_gradients_match_central_differences(fx, meta, tag):
    c, nb, enc, dec, t, snr = _loss_case(fx, meta, tag)
    enc, dec = enc.astype(np.float64), dec.astype(np.float64)
    _, g_enc, g_dec = _ref(tag, enc, dec, t, c["mode"], nb, snr)
    step = 1e-6

    def diff(arr, other_first):
        out = np.empty_like(arr)
        for i in np.ndindex(*arr.shape):
            v = []
            for s in (step, -step):
                a = arr.copy()
                a[i] += s
                args = (enc, a) if other_first else (a, dec)
                v.append(R.loss(args[0], args[1], t, c["mode"], nb, snr))
            out[i] = (v[0] - v[1]) / (2 * step)
        return out

    assert rel_fro(diff(enc, False), g_enc) <= 1e-6
    assert rel_fro(diff(dec, True), g_dec) <= 1e-6


def test_train_refusals_need_no_gpu(meta):
    from quantized_channel_estimation_amd import vae
    h = np.zeros((4, 16), dtype=complex)
    with pytest.raises(NotImplementedError):
        vae.VAE_nbit(_train_params("noisy", 1, apply_batchnorm=True))
    with pytest.raises(ValueError, match="too many values to unpack"):
        vae.VAE_nbit(_train_params("noisy", 1, zeromean=False)).train(h, h, [0])
    with pytest.raises(NotImplementedError):
        vae.VAE_nbit(_train_params("real", 3, quantizer_type="lloyd", quantizer=None)).train(h, h, [0])
    with pytest.raises(NotImplementedError):
        vae.VAE_nbit(_train_params("real", 1, n_pilots=2, n_pilot_convs=1)).train(h, h, [0])
    q = meta["quirks"]["h_test_none"]
    assert q["type"] == "UnboundLocalError" and vae.HTEST_MESSAGE == q["message"]
    with pytest.raises(UnboundLocalError) as ei:
        vae.VAE_nbit(_train_params("genie", 1)).train(h, None, [0])
    assert str(ei.value) == q["message"]


def test_loss_on_host_tensors_is_an_error():
    """No CPU fall-back: the loss and the reparameterisation run on the device or not at all."""
    import torch
    from quantized_channel_estimation_amd import vae
    enc, dec, t = torch.zeros(2, 8), torch.zeros(2, 16), torch.zeros(2, 32)
    with pytest.raises(TypeError):
        vae.elbo_loss(enc, dec, t, mode="noisy")
    with pytest.raises(TypeError):
        vae.reparameterize(enc)


def test_c_abi_refuses_shapes_before_any_launch():
    """The shape refusals of the three entry points come before the first HIP call, so they show without a GPU."""
    from quantized_channel_estimation_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float64)  # never read: every call below is refused on its arguments
    p = _lib.ptr(buf)
    elbo = lambda N, L, mode, nb: lib.qce_vae_elbo(p, p, p, 1, 1, N, L, mode, nb, None, p, p, p, p, 0, None)  # noqa: E731
    assert elbo(48, 4, 0, 1.0) == _lib.QCE_ENOTIMPL
    assert elbo(512, 4, 0, 1.0) == _lib.QCE_ENOTIMPL
    assert elbo(16, 129, 0, 1.0) == _lib.QCE_ENOTIMPL
    assert elbo(16, 4, 1, 9.0) == _lib.QCE_ENOTIMPL
    assert elbo(16, 4, 2, 1.0) == _lib.QCE_EARG
    assert elbo(16, 4, 1, 2.5) == _lib.QCE_EARG
    assert elbo(16, 0, 0, 1.0) == _lib.QCE_EARG
    assert lib.qce_vae_elbo(p, p, p, 1, 2, 16, 4, 0, 1.0, None, None, p, p, p, 0, None) == _lib.QCE_EARG  # target rows < B
    assert lib.qce_vae_elbo(p, p, p, 1, 1, 16, 4, 1, 3.0, None, None, p, p, p, 0, None) == _lib.QCE_EARG  # no snr_db
    assert lib.qce_vae_sample(p, 1, 129, p, 0, 0, p, p, 0, None) == _lib.QCE_ENOTIMPL
    assert lib.qce_vae_sample(p, 1, 4, None, 0, 0, p, None, 0, None) == _lib.QCE_EARG  # drawn eps needs eps_out
    assert lib.qce_vae_sample_bwd(p, p, None, 1, 4, p, 0, None) == _lib.QCE_EARG
    with pytest.raises(NotImplementedError):
        _lib.check(elbo(48, 4, 0, 1.0))


# ---------------------------------------------------------------------------------------------------------- GPU
def _dev(a, dtype=None):
    import torch
    return None if a is None else torch.as_tensor(a, dtype=dtype, device="cuda:0")


def _run_kernel(enc, dec, t, mode, nb, snr, index):
    """(loss, rows, g_enc, g_dec) of elbo_loss with enc and dec as leaves."""
    from quantized_channel_estimation_amd import vae
    e, d = _dev(enc).requires_grad_(True), _dev(dec).requires_grad_(True)
    loss, rows = vae.elbo_loss(e, d, _dev(t), mode=mode, n_bits=nb, snr_db=_dev(snr), index=_dev(index),
                               return_rows=True)
    loss.backward()
    return float(loss.detach()), rows.cpu().numpy(), e.grad.cpu().numpy(), d.grad.cpu().numpy()


def _check_against_restatement(name, got, ref):
    _, rows, g_enc, g_dec = got
    r_rows, r_enc, r_dec = ref
    print(name, "rows %.3g" % rel_fro(rows, r_rows), "enc max rel %.3g" % np.max(np.abs(g_enc - r_enc) / np.abs(r_enc).max()),
          "dec max rel %.3g" % np.max(np.abs(g_dec - r_dec) / np.abs(r_dec).max()))
    assert rows.dtype == np.float64 and g_enc.dtype == np.float32 and g_dec.dtype == np.float32
    assert rel_fro(rows, r_rows) <= 1e-9
    assert _elementwise_ok(g_enc, r_enc)
    assert _elementwise_ok(g_dec, r_dec)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", LOSS_TAGS)
def test_kernel_matches_restatement_and_reference(fx, meta, tag):
    c, nb, enc, dec, t, snr = _loss_case(fx, meta, tag)
    got = _run_kernel(enc, dec, t, c["mode"], nb, snr, None)
    _check_against_restatement(tag, got, _ref(tag, enc, dec, t, c["mode"], nb, snr))
    p = tag + "__"
    l32 = float(fx[p + "loss32"])
    e_loss = abs(got[0] - l32) / abs(l32)
    e_enc, e_dec = rel_fro(got[2], fx[p + "genc32"]), rel_fro(got[3], fx[p + "gdec32"])
    print(tag, "vs reference: loss %.3g enc %.3g dec %.3g of e32 %s" % (e_loss, e_enc, e_dec, c["e32"]))
    assert e_loss <= 16 * c["e32"]["loss"]
    assert e_enc <= 16 * c["e32"]["enc"]
    assert e_dec <= 16 * c["e32"]["dec"]


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(SHAPE_CASES)))
def test_kernel_matches_restatement_on_shapes(ci):
    mode, nb, enc, dec, t, snr, index = _shape_inputs(ci)
    got = _run_kernel(enc, dec, t, mode, nb, snr, index)
    _check_against_restatement(str(SHAPE_CASES[ci]), got, _ref(("shape", ci), enc, dec, t, mode, nb, snr, index))
    again = _run_kernel(enc, dec, t, mode, nb, snr, index)
    assert got[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], again[1:]))


@pytest.mark.gpu
def test_reparameterize_with_given_eps():
    from quantized_channel_estimation_amd import vae
    rng = np.random.default_rng(41)
    B, L = 67, 5
    enc = (0.5 * rng.standard_normal((B, 2 * L))).astype(np.float32)
    eps = rng.standard_normal((B, L)).astype(np.float32)
    g_z = rng.standard_normal((B, L)).astype(np.float32)
    e = _dev(enc).requires_grad_(True)
    z, eps_out = vae.reparameterize(e, _dev(eps), return_eps=True)
    z.backward(_dev(g_z))
    assert np.array_equal(eps_out.cpu().numpy(), eps)
    assert _elementwise_ok(z.detach().cpu().numpy(), R.reparameterize(enc, eps))
    assert _elementwise_ok(e.grad.cpu().numpy(), R.reparameterize_bwd(enc, eps, g_z))


@pytest.mark.gpu
def test_reparameterize_draws():
    import torch
    from quantized_channel_estimation_amd import vae
    B, L, B1 = 512, 128, 200
    enc = torch.zeros((B, 2 * L), dtype=torch.float32, device="cuda:0")
    enc[:, :L] = 0.25
    z, eps = vae.reparameterize(enc, seed=7, return_eps=True)
    z2, eps2 = vae.reparameterize(enc[B1:], seed=7, row_offset=B1, return_eps=True)
    assert torch.equal(eps[B1:], eps2) and torch.equal(z[B1:], z2)
    assert not torch.equal(eps, vae.reparameterize(enc, seed=8, return_eps=True)[1])
    e = eps.cpu().numpy().astype(np.float64)
    assert np.array_equal(z.cpu().numpy(), (0.25 + e).astype(np.float32))  # exp(0) = 1
    n = e.size
    assert n == 2 ** 16
    print("eps mean %.4g var %.4g" % (e.mean(), e.var()))
    assert abs(e.mean()) <= 5 / np.sqrt(n)
    assert abs(e.var() - 1) <= 5 * np.sqrt(2 / n)


def _net(fx, meta, tag):
    from quantized_channel_estimation_amd import vae
    c = meta["net_cases"][tag]
    p = dict(n_antennas=c["N"], n_pilots=c["P"], latent_dim=c["L"], n_layers=c["n_layers"],
             n_pilot_convs=c["n_pilot_convs"], vae_mode=c["mode"], fft_pre=True, zeromean=True, apply_batchnorm=False,
             n_bits=c["n_bits"], quantizer_type="uniform", device=0)
    pre = tag + "__w__"
    est = vae.VAE_nbit(p).load_state_dict({k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)})
    for w in est._w.values():
        w.requires_grad_(True)
    return c, est


def _net_grads(fx, c, est, tag):
    from quantized_channel_estimation_amd import vae
    p = tag + "__"
    for w in est._w.values():
        w.grad = None
    x = _dev(fx[p + "x"])
    enc, dec = est.forward(x if c["mode"] != "real" else x.reshape(c["B"], 1, -1), _dev(fx[p + "eps"]))
    snr = _dev(fx[p + "snr"]) if c["mode"] == "real" else None
    loss = vae.elbo_loss(enc, dec, _dev(fx[p + "t"]), mode=c["mode"], n_bits=c["n_bits"], snr_db=snr)
    loss.backward()
    return float(loss.detach()), {k: w.grad.cpu().numpy() for k, w in est._w.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", NET_TAGS)
def test_autograd_parameter_gradients_match_reference(fx, meta, tag):
    c, est = _net(fx, meta, tag)
    loss, grads = _net_grads(fx, c, est, tag)
    l32 = float(fx[tag + "__loss32"])
    print(tag, "loss %.3g of e32 %.3g" % (abs(loss - l32) / abs(l32), c["e32_loss"]))
    assert abs(loss - l32) / abs(l32) <= 16 * c["e32_loss"]
    assert set(grads) == set(c["e32"])
    worst = {k: rel_fro(grads[k], fx[f"{tag}__g32__{k}"]) / c["e32"][k] for k in grads}
    print(tag, "gradient error in units of e32:", {k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 16, k
    loss2, grads2 = _net_grads(fx, c, est, tag)
    assert loss2 == loss and all(np.array_equal(grads[k], grads2[k]) for k in grads)


@pytest.fixture(scope="module")
def scm_channels():
    from quantized_channel_estimation_amd import scm
    # one path per channel: what there is to learn (the path's angle) shows within the 64 steps of the training test
    h, _ = scm.SCMMulti(path_sigma=2.0, n_path=1).generate_channel(2048 + 512, 1, 16, seed=17)
    h = h[:, 0, :].astype(np.complex128)
    h.setflags(write=False)
    return h[:2048], h[2048:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,nb", [("noisy", 1), ("real", 3)])
def test_training_reduces_the_validation_loss(scm_channels, tmp_path, mode, nb):
    import torch
    from quantized_channel_estimation_amd import observe, vae
    h_train, h_test = scm_channels
    p = _train_params(mode, nb)
    path = str(tmp_path / "saves" / "vae.pt")
    est = vae.VAE_nbit(p)
    tr, te = est.train(h_train, h_test, p["snrs"], seed=3, file_vae=path)
    print(mode, "train", [round(float(v), 3) for v in tr], "validation", [round(float(v), 3) for v in te])
    assert len(tr) == 4 and len(te) == 4
    assert all(v <= 1000 for v in tr) and all(v <= 1000 for v in te)
    assert te[-1] < te[0]
    assert p["file_vae"] == path
    loaded = vae.VAE_nbit.from_checkpoint(path)
    y = observe.get_observation_nbit(h_test[:256], 10.0, None, nb, *p["quantizer"][10][:2], seed=5)
    x = loaded._inputs(torch.as_tensor(y, device="cuda:0"), None, 256)
    assert torch.equal(loaded.forward_nosamp(x), est.forward_nosamp(x))
    hh = est.estimate_from_y(y, 10.0)
    assert hh.shape == (256, 16) and np.all(np.isfinite(hh))


@pytest.mark.gpu
def test_steps_with_a_large_loss_are_skipped(scm_channels, tmp_path, monkeypatch):
    from quantized_channel_estimation_amd import vae
    h_train, h_test = scm_channels
    init = vae.VAE_nbit._init_weights

    def scaled(self, gen):
        import torch
        init(self, gen)
        with torch.no_grad():
            for w in self._w.values():
                w.mul_(1e3)

    monkeypatch.setattr(vae.VAE_nbit, "_init_weights", scaled)
    path = str(tmp_path / "vae.pt")
    p = _train_params("noisy", 1, epochs=2)
    tr, te = vae.VAE_nbit(p).train(h_train[:256], h_test[:128], p["snrs"], file_vae=path)
    assert tr == [] and te == []
    assert not os.path.exists(path)


@pytest.mark.gpu
def test_index_out_of_range_is_clamped_or_refused():
    """An index outside the target's rows: clamped by the kernel (documented), refused with check_index=True."""
    import torch
    from quantized_channel_estimation_amd import vae
    mode, nb, enc, dec, t, snr, _ = _shape_inputs(5)  # 'genie', N = 64, B = 13, T = 5
    bad = np.array([0, 7, -3] + [1] * 10, dtype=np.int32)
    with pytest.raises(ValueError):
        vae.elbo_loss(_dev(enc), _dev(dec), _dev(t), mode=mode, index=_dev(bad), check_index=True)
    got = vae.elbo_loss(_dev(enc), _dev(dec), _dev(t), mode=mode, index=_dev(bad), return_rows=True)[1]
    ref = vae.elbo_loss(_dev(enc), _dev(dec), _dev(t), mode=mode, index=_dev(np.clip(bad, 0, 4)), return_rows=True)[1]
    assert torch.equal(got, ref)
    with pytest.raises(TypeError):
        vae.elbo_loss(_dev(enc), _dev(dec), t, mode=mode)  # a host array as target
