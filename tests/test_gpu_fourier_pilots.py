"""Fourier-domain path for (block-)circulant models observed through A = kron(x, I_N) (QCE_OPT_FOURIER_PILOTS,
csrc/qce_fft_pilot_kernel.h) on the GPU against the CPU oracle, at the cases and bars of
tests/fourier_pilots_ref.py (the bars of the A = I Fourier path; the NumPy restatement reaches them on the CPU,
tests/test_fourier_pilots_ref.py).  B = 37: two 16-row tiles and a ragged one; K = 20: one 16-component block and a
ragged one."""
import pickle

import numpy as np
import pytest

import fourier_pilots_ref as R
from conftest import rel_fro

pytestmark = pytest.mark.gpu

# the family each case's prepare reports without the option (select_backend at M = P N), keyed by (N, P)
DENSE_KERNEL = {(16, 2): "f64_3m", (32, 3): "f64_4m", (64, 4): "f64_wide", (256, 2): "big"}


def _gpu():
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")


def _proba_rtol(n_bits):
    # an lp error e moves a probability by the factor e^e: the lp atol (1e-5 at 1 bit, 1e-8 otherwise) times the
    # few units an lp difference accumulates, as in test_gpu_parity.py::test_logprob_proba_labels_after_estimate
    return 1e-4 if n_bits == 1 else 1e-7


@pytest.mark.parametrize("case", R.CASES, ids=[f"c{i}" for i in range(len(R.CASES))])
def test_cases_vs_oracle(case):
    _gpu()
    from quantized_channel_estimation_amd import Gmm_nbit
    K, N, blocks, P, ptype, n_bits, qtype, mean, snr = case
    means, covs, w, A, y, qz = R.make_case(case)
    ref = R.oracle_results(case)
    h_tol, rtol, atol = R.bars(n_bits)
    g = Gmm_nbit.from_params(means, covs, w, fourier_pilots=True)
    res = {}
    for mode in R.MODES:
        hg = g.estimate_from_y(y, snr, N, A, mode, n_bits, qtype, qz)
        assert g._dev.structure()[2] == 1
        assert g._dev.kernel() == "fourier_pilots"
        err = rel_fro(hg, ref[mode])
        print(case, mode, "h rel_fro", err)
        assert err < h_tol, (mode, err)
        res[mode] = hg
    lp = g._estimate_weighted_log_prob(y)
    print(case, "lp max abs err", np.max(np.abs(lp - ref["lp"])))
    np.testing.assert_allclose(lp, ref["lp"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(g.predict_proba_cplx(y), ref["proba"], rtol=_proba_rtol(n_bits), atol=1e-13)
    np.testing.assert_array_equal(g._predict_cplx(y), ref["labels"])
    # the same calls with the option off: today's family, within the same bars of the option-on result
    g0 = Gmm_nbit.from_params(means, covs, w)
    for mode in R.MODES:
        h0 = g0.estimate_from_y(y, snr, N, A, mode, n_bits, qtype, qz)
        assert g0._dev.structure()[2] == 0
        assert g0._dev.kernel() == DENSE_KERNEL[(N, P)]
        err = rel_fro(h0, res[mode])
        print(case, mode, "off vs on rel_fro", err)
        assert err < h_tol, (mode, err)
    np.testing.assert_allclose(g0._estimate_weighted_log_prob(y), lp, rtol=rtol, atol=atol)
    np.testing.assert_array_equal(g0._predict_cplx(y), ref["labels"])


def test_device_io_equals_host_io():
    _gpu()
    import torch
    from quantized_channel_estimation_amd import _lib
    case = R.CASES[2]
    K, N, blocks, P, ptype, n_bits, qtype, mean, snr = case
    means, covs, w, A, y, qz = R.make_case(case)
    dm = _lib.DeviceModel(means, covs, w)
    dm.set_fourier_pilots(True)
    dm.prepare(A, snr, float(n_bits), _lib.QUANT_LLOYD, qz[0], qz[1])
    assert dm.kernel() == "fourier_pilots"
    host = dm.estimate(y)
    yd = torch.from_numpy(y).to("cuda")
    torch.cuda.synchronize()
    out = dm.estimate(yd)
    dm.synchronize()
    assert rel_fro(out.cpu().numpy(), host) < 1e-12
    assert rel_fro(host, R.oracle_results(case)["all"]) < R.bars(n_bits)[0]
    # the dense tables of such a prepare come from the dense replay with the stored A
    t = dm.tables(("A_eff", "cconst"))
    assert t["A_eff"].shape == (K, P * N, N) and np.isfinite(t["cconst"]).all()
    assert dm.kernel() == "fourier_pilots" and dm.structure()[2] == 1
    assert np.isfinite(dm.cconst_max())
    dm.close()


def test_one_component_and_one_row():
    _gpu()
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import Gmm_nbit
    case = R.CASES[1]
    K, N, blocks, P, ptype, n_bits, qtype, mean, snr = case
    means, covs, w, A, y, qz = R.make_case(case)
    g1 = Gmm_nbit.from_params(means[:1], covs[:1], np.array([1.0]), fourier_pilots=True)
    for mode in ("all", 1):
        h1 = g1.estimate_from_y(y, snr, N, A, mode, n_bits, qtype, qz)
        assert g1._dev.kernel() == "fourier_pilots"
        assert rel_fro(h1, O.estimate(means[:1], covs[:1], np.array([1.0]), y, snr, N, A, mode, n_bits, qtype, qz)) < 1e-9
    g = Gmm_nbit.from_params(means, covs, w, fourier_pilots=True)
    for mode in R.MODES:
        hb = g.estimate_from_y(y[:1], snr, N, A, mode, n_bits, qtype, qz)
        assert hb.shape == (1, N)
        assert rel_fro(hb, R.oracle_results(case)[mode][:1]) < 1e-9
    assert g.estimate_from_y(y[:0], snr, N, A, "all", n_bits, qtype, qz).shape == (0, N)


def test_fallbacks_stay_dense(monkeypatch):
    _gpu()
    from quantized_channel_estimation_amd import _lib, inputs
    N = 16
    means, covs, w = inputs.synthetic_model(4, N, cov_type="circulant", seed=2)

    def family(means, covs, w, A, option=True):
        dm = _lib.DeviceModel(means, covs, w)
        if option:
            dm.set_fourier_pilots(True)
        dm.prepare(A, 5.0, 1.0)
        out = (dm.structure()[2], dm.kernel())
        dm.close()
        return out

    A2 = inputs.get_pilot_matrix(N, 2, 1)
    assert family(means, covs, w, A2) == (1, "fourier_pilots")
    assert family(means, covs, w, A2, option=False) == (0, "f64_3m")           # option off
    mf, cf, wf = inputs.synthetic_model(4, N, cov_type="full", seed=2)
    assert family(mf, cf, wf, A2)[0] == 0                                        # a 'full' model
    A_off = A2.copy()
    A_off[3, 7] = 1e-300                                                         # not kron(x, I): one off-diagonal entry
    assert family(means, covs, w, A_off) == (0, "f64_3m")
    A_diag = A2.copy()
    A_diag[N + 5, 5] *= 1 + 1e-15                                                # a block diagonal that is not one value
    assert family(means, covs, w, A_diag) == (0, "f64_3m")
    assert family(means, covs, w, inputs.get_pilot_matrix(N, 5, 1))[0] == 0      # P = 5
    m2, c2, w2 = inputs.synthetic_model(2, 256, cov_type="block-circulant", seed=2, blocks=(4, 64))
    assert family(m2, c2, w2, inputs.get_pilot_matrix(256, 4, 1)) == (0, "big")  # N = 256 with P = 4: P N > 512
    monkeypatch.setenv("QCE_FFT", "0")
    assert family(means, covs, w, A2) == (0, "f64_3m")


def test_not_positive_definite_raises_reference_text():
    _gpu()
    from quantized_channel_estimation_amd import Gmm_nbit, _lib, inputs
    N = 16
    means, covs, w = inputs.synthetic_model(3, N, cov_type="circulant", seed=1)
    F = np.fft.fft(np.eye(N)) / np.sqrt(N)
    c = np.ones(N)
    c[5] = -3.0  # R(5) = c_5 x x^H + s2 I has the eigenvalue -3 |x|^2 + s2 < 0
    covs[1] = F.conj().T @ np.diag(c) @ F
    A = inputs.get_pilot_matrix(N, 2, np.inf)
    rng = np.random.default_rng(0)
    y = inputs.crandn(5, 2 * N, rng=rng)
    g = Gmm_nbit.from_params(means, covs, w, fourier_pilots=True)
    g.mirror_state = False
    with pytest.raises(ValueError) as ei:
        g.estimate_from_y(y, 5.0, N, A, "all", np.inf)
    assert str(ei.value) == _lib.CHOL_MESSAGE
    assert g._dev.kernel() in ("fourier_pilots", "none")
    with pytest.raises(ValueError):
        R.prepare(means, covs, w, R.pilot_vector(A, N), 5.0, np.inf)


def test_partials_are_not_implemented_and_pickle_keeps_the_option():
    _gpu()
    from quantized_channel_estimation_amd import Gmm_nbit, _lib
    case = R.CASES[0]
    K, N, blocks, P, ptype, n_bits, qtype, mean, snr = case
    means, covs, w, A, y, qz = R.make_case(case)
    dm = _lib.DeviceModel(means, covs, w)
    dm.set_fourier_pilots(True)
    dm.prepare(A, snr, 1.0)
    assert dm.kernel() == "fourier_pilots"
    for call in (dm.partial, dm.partial64):
        with pytest.raises(NotImplementedError, match="pilots"):
            call(y)
    with pytest.raises(NotImplementedError, match="pilots"):
        dm.partial_shifted(y, 0.0)
    dm.close()
    g = Gmm_nbit.from_params(means, covs, w, fourier_pilots=True)
    h = g.estimate_from_y(y, snr, N, A, "all", n_bits)
    g2 = pickle.loads(pickle.dumps(g))
    assert g2.fourier_pilots is True and g2._dev is None
    assert rel_fro(g2.estimate_from_y(y, snr, N, A, "all", n_bits), h) == 0.0
    assert g2._dev.kernel() == "fourier_pilots"
    g2.fourier_pilots = False  # part of the device-model key: the next estimate prepares densely
    assert rel_fro(g2.estimate_from_y(y, snr, N, A, "all", n_bits), h) < 1e-7
    assert g2._dev.kernel() == "f64_3m"
