"""The int8-slice precision (precision="int8": k_pack_i8, k_est_all_i8) on the GPU against its NumPy contract
(tests/int8_ref.py), the FP64 kernels and the FP64 oracle.

Bars: the raw digit-plane sums are integers below 2^53 at S <= 5, so they equal the model's bit for bit.  The kernel
against the model on the device's own tables at the same S differs only by FP64 rounding order: 1e-12, the project's
bar between two FP64 kernels on one prepared model (tests/test_gpu_f64.py), at least four decades below one plane
step at S <= 6.  Against the oracle at the default S = 7: F64_TOL = 1e-9.
"""
import functools

import numpy as np
import pytest

import fast_ref as R
import int8_ref as I8
from conftest import load_model, rel_fro

pytestmark = pytest.mark.gpu

SAME_TOL = 1e-12
F64_TOL = 1e-9
TILE = 128  # samples per workgroup of k_est_all_i8


def _id(c):
    return f"K{c.K}-{c.M}x{c.N}-B{c.B}-b{c.n_bits}-m{int(c.mean)}"


def _lib():
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    return _lib


def _device(c, precision="int8", slices=None, expect="int8"):
    lib = _lib()
    d = R.inputs(c)
    dm = lib.DeviceModel(d["means"], d["covs"], d["w"])
    if precision == "int8":
        dm.set_precision("int8", **({} if slices is None else {"slices": slices}))
    elif precision != "f64":
        dm.set_precision(precision)
    dm.prepare(d["A"], c.snr, float(c.n_bits))
    if expect is not None:
        assert dm.kernel() == expect
    return dm


def _tables(dm):
    return dm.tables(("means_y", "P", "W", "b", "cconst"))


def _same_s(c, S, what):
    """kernel at S planes against the model at S planes on the device's own tables"""
    dm = _device(c, slices=S)
    h = dm.estimate(R.inputs(c)["y"])
    ref = I8.model(c, S, tables=_tables(dm), with_oracle=False)
    assert ref["on_grid"].all()
    e = rel_fro(h, ref["h"])
    print(f"{what}: rel_fro(kernel, model at S={S}) {e:.3e} (bar {SAME_TOL:.0e})")
    assert np.isfinite(h).all()
    assert e < SAME_TOL
    return dm, h


# ---- 1: raw products, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("S", [3, 5])
@pytest.mark.parametrize("shape", [(12, 12), (52, 16)])
def test_1_raw_products_bit_for_bit(shape, S, mean):
    M, N = shape
    c = R.case(3, M, N, 300, R._exact_bits(M, N), mean)
    dm = _device(c, slices=S)
    y = R.inputs(c)["y"]
    ref = I8.model(c, S, tables=_tables(dm), with_oracle=False)
    assert ref["max_acc"] * 128.0 ** (S - 1) * S < 2.0 ** 53  # every partial sum is an exact double
    MP, NP = R.padded_shape(M, N)
    for k in range(c.K):
        raw_l, raw_w, exps = dm.debug_i8_products(y, k)
        assert raw_l.shape == (300, 2 * MP) and raw_w.shape == (300, 2 * NP)
        assert np.array_equal(exps, ref["exps"][k]), (k, "exponents")
        assert np.array_equal(raw_l, ref["raw_L"][k]), (k, "raw_L", np.argwhere(raw_l != ref["raw_L"][k])[:4])
        assert np.array_equal(raw_w, ref["raw_W"][k]), (k, "raw_W", np.argwhere(raw_w != ref["raw_W"][k])[:4])
        assert np.any(raw_l != 0) and np.any(raw_w != 0)


# ---- 2: the kernel against the model at the same S -------------------------------------------------------------------
CASES_2 = [R.case(3, M, N, 300, R._exact_bits(M, N), mean) for (M, N) in R.H2_SIZES.values() for mean in (False, True)]


@pytest.mark.parametrize("c", CASES_2, ids=_id)
def test_2_same_s_model_every_shape(c):
    _same_s(c, 5, "2 " + _id(c))


@pytest.mark.parametrize("S", [3, 7, 8])
def test_2_same_s_model_slice_counts(S):
    c = R.case(3, 64, 64, 300, 1, True)
    _same_s(c, S, f"2 64x64 S={S}")


# ---- 3: against the FP64 kernel and the oracle at the default S ------------------------------------------------------
@pytest.mark.parametrize("c", [R.case(3, 64, 64, 300, 1, True), R.case(3, 60, 32, 300, 2, True)], ids=_id)
def test_3_default_slices_against_fp64(c):
    y = R.inputs(c)["y"]
    dm = _device(c)
    h = dm.estimate(y)
    h64 = _device(c, "f64", expect=None).estimate(y)
    ho, _ = R.oracle(c)
    e64, eo = rel_fro(h, h64), rel_fro(h, ho)
    print(f"3 {_id(c)}: rel_fro(int8, f64 kernel) {e64:.3e} (bar {SAME_TOL:.0e})  rel_fro(int8, oracle) {eo:.3e} "
          f"(bar {F64_TOL:.0e})")
    assert dm.kernel() == "int8"
    assert e64 < SAME_TOL
    assert eo < F64_TOL


# ---- 4: the top and a middle level count -----------------------------------------------------------------------------
def test_4_seven_bits_reach_127():
    c = R.case(3, 48, 48, 300, 7, True, 5.0, 1.5)  # channel scale 1.5: the quantiser saturates
    ti = np.rint(R.embed_vec(R.inputs(c)["y"]) * R.y_scale_of(c))
    assert ti.max() == 127 and ti.min() == -127
    _same_s(c, 5, "4 7-bit 48x48")


def test_4_four_bits():
    _same_s(R.case(3, 32, 32, 300, 4, True), 5, "4 4-bit 32x32")


# ---- 5: ragged batches -----------------------------------------------------------------------------------------------
def test_5_ragged_batches():
    c = R.case(3, 64, 64, 300, 1, True)
    dm = _device(c)
    y = R.inputs(c)["y"]
    full = dm.estimate(y)
    for B in (1, TILE - 1, TILE, TILE + 1):
        e = rel_fro(dm.estimate(y[:B]), full[:B])
        print(f"5 B={B}: rel_fro against the leading rows of B=300 {e:.3e}")
        assert e < SAME_TOL


# ---- 6: off-grid rows -------------------------------------------------------------------------------------------------
def test_6_off_grid_rows_are_nan_and_only_they():
    c = R.case(3, 64, 64, 300, 1, True)
    dm = _device(c)
    y = R.inputs(c)["y"]
    clean = dm.estimate(y)
    bad = np.array(y)
    rng = np.random.default_rng(5)
    for r in (3, 257):
        bad[r] = 0.4 * (rng.standard_normal(c.M) + 1j * rng.standard_normal(c.M))
    h = dm.estimate(bad)
    nan_rows = np.isnan(h).any(axis=1)
    assert np.flatnonzero(nan_rows).tolist() == [3, 257]
    assert np.isnan(h[[3, 257]].real).all() and np.isnan(h[[3, 257]].imag).all()
    assert np.array_equal(h[~nan_rows], clean[~nan_rows])
    assert np.isfinite(clean).all()


# ---- 7: fallbacks ------------------------------------------------------------------------------------------------------
def _both(means, covs, w, A, snr, n_bits, y, **prep):
    lib = _lib()
    out = {}
    for prec in ("int8", "f64"):
        dm = lib.DeviceModel(means, covs, w)
        if prec == "int8":
            dm.set_precision("int8")
        dm.prepare(A, snr, float(n_bits), **prep)
        out[prec] = (dm.kernel(), dm.estimate(y))
    return out


@pytest.mark.parametrize("which", ["inf", "8bit", "lloyd", "100x64", "circulant"])
def test_7_fallbacks_are_the_f64_family_bit_for_bit(which):
    lib = _lib()
    prep = {}
    if which == "circulant":
        fx = load_model("circ")
        args = (fx["means_cplx"], fx["covs_cplx"], fx["weights"], None, float(fx["b1_5__snr"]), 1, fx["b1_5__y"])
    else:
        c = {"inf": R.case(3, 32, 32, 300, np.inf, True), "8bit": R.case(3, 32, 32, 300, 8, True),
             "lloyd": R.case(3, 32, 32, 300, 2, True), "100x64": R.case(3, 100, 64, 260, 2, True)}[which]
        d = R.inputs(c)
        if which == "lloyd":
            from quantized_channel_estimation_amd import inputs as I
            thr, lab, _ = I.load_quantizer(c.snr, 2)[c.snr]
            prep = dict(quant_kind=lib.QUANT_LLOYD, thresholds=thr, labels=lab)
        args = (d["means"], d["covs"], d["w"], d["A"], c.snr, c.n_bits, d["y"])
    r = _both(*args, **prep)
    print(f"7 {which}: int8 -> {r['int8'][0]}, f64 -> {r['f64'][0]}")
    assert r["int8"][0] == r["f64"][0] != "int8"
    assert r["int8"][0] in ("f64_3m", "f64_4m", "f64_wide", "fourier", "big")
    assert np.array_equal(r["int8"][1], r["f64"][1])


def test_7_partials_and_slice_range():
    c = R.case(3, 32, 32, 300, 1, True)
    dm = _device(c)
    y = R.inputs(c)["y"]
    for call in (lambda: dm.partial(y), lambda: dm.partial64(y), lambda: dm.partial_shifted(y, 0.0)):
        with pytest.raises(NotImplementedError):
            call()
    for s in (2, 9):
        with pytest.raises(ValueError):
            dm.set_precision("int8", slices=s)


# ---- 8: drop-in --------------------------------------------------------------------------------------------------------
def test_8_drop_in_estimator():
    from quantized_channel_estimation_amd.gmm import Gmm_nbit
    c = R.case(3, 32, 32, 300, 1, True)
    d = R.inputs(c)
    g = Gmm_nbit.from_params(d["means"], d["covs"], d["w"], precision="int8")
    h7 = g.estimate_from_y(d["y"], c.snr, c.N, None, "all", 1)
    assert g._dev.kernel() == "int8"
    assert np.array_equal(h7, _device(c).estimate(d["y"]))
    g.int8_slices = 3
    h3 = g.estimate_from_y(d["y"], c.snr, c.N, None, "all", 1)
    assert np.array_equal(h3, _device(c, slices=3).estimate(d["y"]))
    assert not np.array_equal(h3, h7)
