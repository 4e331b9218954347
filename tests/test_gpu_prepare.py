"""The per-SNR prepare (csrc/qce_prepare.hip, qce_fft.hip's prepare, the dense re-prepare behind qce_get_tables)
against the extended-precision reference of tests/prepare_ref.py: all eight tables, cconst and lp, for every kernel
family, at the bound

    max(F * e_oracle[table, case], G * M * 2^-53 * kappa_table)

of prepare_ref (e_oracle: the FP64 NumPy oracle's own error against the same reference, tests/test_prepare_ref.py).
lp and cconst are compared absolutely: a shift common to all components cancels in h, proba and the labels and shows
only here.  Every check prints `kernel error / e_oracle / bound` before it asserts (pytest -s); the measured table is
in DESIGN.md.

Cholesky kernel per M (qce_launch_prepare): M <= 64 -> k_chol_inv_lds2<1024> (two columns per phase) from M = 16,
k_chol_inv_lds<1024> below; 64 < M <= 128 -> k_chol_inv_tri<128>; M > 128 -> k_chol_inv.  The process-wide switches
QCE_CHOL=wave|tri, QCE_CHOL_PAIRS=0, QCE_CHOL_THREADS=256|512 move M <= 64 to k_chol_inv_wave, k_chol_inv_tri<64>,
k_chol_inv_lds<1024>, k_chol_inv_lds2<512> / k_chol_inv_lds<256>; QCE_ZGEMM=valu replaces k_zgemm_mfma by k_zgemm.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import prepare_dump as D
import prepare_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu():
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    return _lib


def _model_M(_lib, dm):
    m = ctypes.c_int(-1)
    _lib.check(_lib.load().qce_model_info(dm.handle, None, None, ctypes.byref(m), None))
    return m.value


def _check_prepared(_lib, dm, name):
    """All eight tables, lp, cconst_max, model_info and the kernel family of the case `dm` was last prepared for."""
    c = R.case(name)
    assert dm.kernel() == c["family"], (name, dm.kernel())
    assert _model_M(_lib, dm) == c["M"]
    t = dm.tables()
    t["lp"] = dm.log_prob(c["X"], want_lp=True)[0]
    R.check(name, t)
    assert dm.cconst_max() == np.max(dm.cconst()) == np.max(t["cconst"])
    return t


# M -> Cholesky kernel: 12 lds<1024>; 16, 33 (padded 64, odd), 64, 37, 24 lds2<1024>; 65, 100, 128 tri<128>;
# 129, 200, 256, 257, 272 k_chol_inv.  A = I and M <= 64: k_filter_id; A = I above: k_scale_cols + two GEMMs; a dense
# or pilot A: k_gain_cr<false> and five GEMMs (m, n off the 32 x 32 tile and k off the 16-step at 20 / 37 and 40 / 24).
@pytest.mark.parametrize("name", list(R.DENSE))
def test_dense_prepare_vs_extended_reference(name):
    _lib = _gpu()
    dm = D.device_model(name)
    D.prepare_case(dm, name)
    _check_prepared(_lib, dm, name)
    # the same model again at another SNR and bit width, with A = I where A was not (another M in the same buffers):
    # the q0 / b zero-fills of a zero-mean model and the cached device identity (a_identity_n) are reused state
    D.prepare_case(dm, name + "/2")
    _check_prepared(_lib, dm, name + "/2")
    # ... and back: the first case's A replaces the identity in the A buffer
    D.prepare_case(dm, name)
    _check_prepared(_lib, dm, name)
    dm.close()


@pytest.mark.parametrize("name", list(R.FOURIER))
def test_fourier_prepare_vs_extended_reference(name):
    """lp from the Fourier-domain tables, then the dense re-prepare behind tables() (ensure_dense), which leaves the
    Fourier tables active and the estimates bit-identical.  At 1 bit the printed line sets the Fourier formulas' lp
    error beside the oracle's: DESIGN.md attributes the gap between the two to the dense FP64 arithmetic's own
    rounding of the arcsine law's arguments."""
    _lib = _gpu()
    c = R.case(name)
    dm = D.device_model(name)
    D.prepare_case(dm, name)
    assert dm.structure()[2] == 1 and dm.kernel() == "fourier"
    lp = dm.log_prob(c["X"], want_lp=True)[0]
    R.check(name, {"lp": lp}, tables=("lp",), report=lambda s: print("fourier", s))
    h_before = np.array(dm.estimate(c["X"]))
    t = dm.tables()
    R.check(name, t, tables=R.TABLES)
    assert dm.structure()[2] == 1 and dm.kernel() == "fourier"
    assert _model_M(_lib, dm) == c["M"]
    assert dm.cconst_max() == np.max(t["cconst"])
    h_after = np.array(dm.estimate(c["X"]))
    np.testing.assert_array_equal(h_before, h_after)
    np.testing.assert_array_equal(dm.log_prob(c["X"], want_lp=True)[0], lp)
    dm.close()


@pytest.mark.parametrize("mname", ["circ", "bcirc"])
def test_fourier_one_bit_lp_on_golden_circulant_models(golden_models, mname):
    """test_logprob_proba_labels_after_estimate allows the Fourier path 1e-6 on lp at 1 bit because the reference's
    dense FP64 arithmetic loses digits in the arcsine law there.  Measured against the extended
    reference at the golden 20 dB case: the recorded lp of the reference project, the oracle and the Fourier kernel,
    the kernel held to the floor G M u kappa alone -- the Fourier formulas take the arcsine of the first circulant
    column, whose leading entry is 1 exactly, so the amplification F * e_oracle stands for does not apply to them."""
    from conftest import case_args
    from oracle import qce_oracle as O
    _lib = _gpu()
    fx = golden_models[mname]
    y, snr, N, A, n_bits, qtype, quantizer = case_args(fx, "b1_20")
    means, covs, w = fx["means_cplx"], fx["covs_cplx"], fx["weights"]
    t = R.prepare(means, covs, w, None, snr, n_bits)
    ref = R.log_prob(t, y)
    o = O.prepare(means, covs, np.eye(N), snr, n_bits)
    e_oracle = R.error("lp", O.weighted_log_prob(y, o["means_y"], o["P"], w), ref)
    e_fixture = R.error("lp", fx["b1_20__lp"], ref)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, snr, 1.0)
    assert dm.structure()[2] == 1
    e_fourier = R.error("lp", dm.log_prob(y, want_lp=True)[0], ref)
    kappa = max(np.linalg.cond(t["Cr"][k].astype(complex)) for k in range(covs.shape[0]))
    bound = R.G * N * R.U * kappa
    print(f"{mname} b1_20 lp: fourier kernel {e_fourier:.2e}  oracle {e_oracle:.2e}  reference's record "
          f"{e_fixture:.2e}  kappa {kappa:.1e}  bound {bound:.2e}")
    assert e_fourier <= bound
    dm.close()


@pytest.mark.parametrize("M", R.NONPD_M)
def test_nonpd_component_detected_per_cholesky_family(M):
    """Component 2 fails at its last pivot (-1e-3 s) only; 12 -> k_chol_inv_lds, 33 -> k_chol_inv_lds2,
    100 -> k_chol_inv_tri<128>, 200 and 264 -> k_chol_inv (264: the estimates go through qce_big.hip)."""
    import torch
    _lib = _gpu()
    ok = f"ok{M}"
    X = R.case(ok)["X"]
    dm = _lib.DeviceModel(*R.nonpd_mixture(M))
    dm.prepare(None, 300.0, float("inf"))
    with pytest.raises(ValueError) as ei:
        dm.estimate(X)
    assert str(ei.value) == _lib.CHOL_MESSAGE
    # device I/O: no host round trip, the shard shift carries the failure as +inf (a failure the library already
    # knows of -- the status copy of the prepare has landed -- is raised at once instead)
    dm.prepare(None, 300.0, float("inf"))
    out = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    try:
        dm.cconst_max(out=out)
    except ValueError as e:
        assert str(e) == _lib.CHOL_MESSAGE
    else:
        torch.cuda.synchronize()
        assert out.item() == float("inf")
    # the same handle with a valid mixture
    c = R.case(ok)
    dm.set_params(c["means"], c["covs"], c["w"])
    D.prepare_case(dm, ok)
    _check_prepared(_lib, dm, ok)
    dm.close()


@pytest.mark.parametrize("switch", ["QCE_CHOL=wave", "QCE_CHOL=tri", "QCE_CHOL_PAIRS=0", "QCE_CHOL_THREADS=256",
                                    "QCE_CHOL_THREADS=512", "QCE_ZGEMM=valu"])
def test_process_wide_switches_hold_the_same_bounds(switch, tmp_path):
    _gpu()
    key, val = switch.split("=")
    env = dict(os.environ)
    for k in ("QCE_CHOL", "QCE_CHOL_PAIRS", "QCE_CHOL_THREADS", "QCE_ZGEMM"):
        env.pop(k, None)
    env[key] = val
    out = str(tmp_path / "tables.npz")
    gemm = key == "QCE_ZGEMM"
    r = subprocess.run([sys.executable, os.path.join(HERE, "prepare_dump.py"), out] + (["--gemm"] if gemm else []),
                       env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    from quantized_channel_estimation_amd import _lib
    z = np.load(out)
    assert str(z["nonpd33"]) == _lib.CHOL_MESSAGE
    for name in R.SMALL + (R.SMALL_GEMM if gemm else ()):
        assert str(z[f"{name}__family"]) == R.case(name)["family"]
        R.check(name, {tb: z[f"{name}__{tb}"] for tb in R.TABLES + ("lp",)},
                report=lambda s: print(switch, s))
