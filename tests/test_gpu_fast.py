"""The fast-precision estimate kernels (precision="fast": k_est_all_h2, k_est_all_h2w, k_est_all_h2x with
k_merge_streamk / k_merge_splits, k_y_exact, k_pack_h2; QCE_KERNEL=f32: k_est_all_f32, k_est_weighted_f32 with the
f32 weights of k_select) against the FP64 oracle, every case held to the bars of the arithmetic model in
tests/fast_ref.py (case matrix and derivation there):

    rel_fro < min(1e-5, 8 e_model_fro),     worst row < 8 e_model_row.

Families: a -- the 9 padded shapes of k_est_all_h2; b -- its stream-K schedules, the wide variant, ragged batches;
c -- the 8 shapes of k_est_all_h2x, K splits, ragged batches; d -- the FP32-MFMA kernel; e -- the fast selective
modes; f -- K-shard outputs; g -- small amplitudes on the inexact-y path.  'all' mode has no discrete decision, so
no row is excluded anywhere; in the selective modes the log-probabilities are FP64 (k_lp_f64), so the labels must
equal the oracle's and again no row is excluded.

Measured on an MI355X: DESIGN.md, "Fast family against an arithmetic model" (every kernel error within 3.4x of the
model's, bars at 8x).  Family g found the unscaled y_lo split of the inexact path losing bits below |y| ~ 1e-2; the
kernels now scale the batch first, and the last test pins the exact path bit for bit across that change.
"""
import numpy as np
import pytest

import fast_ref as R

pytestmark = pytest.mark.gpu


def _id(c):
    return f"K{c.K}-{c.M}x{c.N}-B{c.B}-b{c.n_bits}-m{int(c.mean)}-s{c.scale:g}"


def _device(c, lo=0, hi=None):
    """DeviceModel of the case's components [lo, hi) with precision='fast', prepared for the case."""
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    d = R.inputs(c)
    dm = _lib.DeviceModel(d["means"][lo:hi], d["covs"][lo:hi], d["w"][lo:hi])
    dm.set_precision("fast")
    dm.prepare(d["A"], c.snr, float(c.n_bits))
    assert dm.kernel() == "fast"
    return dm


def _check(h, ref, what, rows=None):
    ho = ref["oracle"] if rows is None else ref["oracle"][:rows]
    e = R.errors(h, ho)
    fro_bar, row_bar = R.bars(ref, rows)
    print(f"{what}: rel_fro {e['e_fro']:.3e} (bar {fro_bar:.3e})  worst row {e['e_row']:.3e} (bar {row_bar:.3e})")
    assert np.isfinite(np.asarray(h)).all(), what
    assert e["e_fro"] < fro_bar, (what, e["e_fro"], fro_bar)
    assert e["e_row"] < row_bar, (what, e["e_row"], row_bar)


def _final_and_partial(dm, y, N):
    from quantized_channel_estimation_amd.sharding import combine_partials_numpy
    return dm.estimate(y), combine_partials_numpy([dm.partial(y)], N)


# ---- a: k_est_all_h2, every padded shape ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_a(), ids=_id)
def test_a_h2_shapes(c):
    dm = _device(c)
    _check(dm.estimate(R.inputs(c)["y"]), R.reference(c), "a " + _id(c))


# ---- b: scheduling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wg", ["1", "2", "5", "5000"])
def test_b_streamk_cuts_final_and_partial(wg, monkeypatch):
    """K = 7 over 3 tiles of 256: one workgroup (whole rounds), 2 and 5 (tiles cut between workgroups, merged by
    k_merge_streamk into h and, for the partial, with h == nullptr), 5000 (more slots than items)."""
    monkeypatch.setenv("QCE_WORKGROUPS", wg)
    c = R.CASE_B
    dm = _device(c)
    hf, hp = _final_and_partial(dm, R.inputs(c)["y"], c.N)
    _check(hf, R.reference(c), f"b wg={wg} final")
    _check(hp, R.reference(c), f"b wg={wg} partial")


@pytest.mark.parametrize("c", R.CASES_B_WIDE, ids=_id)
def test_b_wide_variant(c, monkeypatch):
    """QCE_H2_WIDE=1: k_est_all_h2w on exact y; on inexact y it returns and the 8-wave instance runs."""
    monkeypatch.setenv("QCE_H2_WIDE", "1")
    dm = _device(c)
    hf, hp = _final_and_partial(dm, R.inputs(c)["y"], c.N)
    _check(hf, R.reference(c), "b wide final " + _id(c))
    _check(hp, R.reference(c), "b wide partial " + _id(c))


def test_b_ragged_batches():
    c = R.CASE_B
    dm = _device(c)
    for B in R.B_SIZES_H2:
        _check(dm.estimate(R.inputs(c)["y"][:B]), R.reference(c), f"b B={B}", rows=B)


# ---- c: k_est_all_h2x ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_c(), ids=_id)
def test_c_h2x_shapes(c):
    dm = _device(c)
    _check(dm.estimate(R.inputs(c)["y"]), R.reference(c), "c " + _id(c))


@pytest.mark.parametrize("ksplit", ["1", "2", "3"])
@pytest.mark.parametrize("c", R.CASES_C_KSPLIT, ids=_id)
def test_c_k_splits_final_and_partial(c, ksplit, monkeypatch):
    """K = 5 in 1, 2, 3 splits: records merged by k_merge_splits into h and into the (m, s, acc) partial."""
    monkeypatch.setenv("QCE_KSPLIT", ksplit)
    dm = _device(c)
    hf, hp = _final_and_partial(dm, R.inputs(c)["y"], c.N)
    _check(hf, R.reference(c), f"c ksplit={ksplit} final " + _id(c))
    _check(hp, R.reference(c), f"c ksplit={ksplit} partial " + _id(c))


def test_c_ragged_batches():
    c = R.CASES_C_KSPLIT[0]
    dm = _device(c)
    for B in R.B_SIZES_H2X:
        _check(dm.estimate(R.inputs(c)["y"][:B]), R.reference(c), f"c B={B}", rows=B)


# ---- d: the FP32-MFMA kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_d(), ids=_id)
def test_d_f32_kernel_final_and_partial(c, monkeypatch):
    monkeypatch.setenv("QCE_KERNEL", "f32")
    dm = _device(c)
    hf, hp = _final_and_partial(dm, R.inputs(c)["y"], c.N)
    ref = R.reference(c, "f32")
    _check(hf, ref, "d final " + _id(c))
    _check(hp, ref, "d partial " + _id(c))


# ---- e: fast selective modes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mtag", list(R.SELECTIVE_MODES))
@pytest.mark.parametrize("c", R.cases_e(), ids=_id)
def test_e_selective_modes(c, mtag):
    """FP64 log-probabilities, f32 selection weights into k_est_weighted_f32: labels bit-exact, h on the f32 model's
    bars."""
    from oracle import qce_oracle as O
    from quantized_channel_estimation_amd import _lib
    mode = R.SELECTIVE_MODES[mtag]
    d = R.inputs(c)
    dm = _device(c)
    kmode, param = (_lib.MODE_TOPN, float(mode)) if isinstance(mode, int) else (_lib.MODE_CUMP, float(mode))
    h = dm.estimate(d["y"], kmode, param)
    ref = R.reference(c, "f32", mode)
    t = ref["tables"]
    np.testing.assert_array_equal(dm.log_prob(d["y"], want_lp=False, want_labels=True)[2],
                                  O.predict(d["y"], t["means_y"], t["P"], d["w"]))
    _check(h, ref, f"e {mtag} " + _id(c))


# ---- f: K-shard outputs of a fast model ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES_F, ids=_id)
def test_f_kshard_outputs(c):
    """partial (f32 accumulator), partial64 (widened) and partial_shifted of two component shards combine to the
    unsharded estimate, on the unsharded case's bars."""
    from quantized_channel_estimation_amd.sharding import combine_packed_numpy, combine_partials_numpy
    y = R.inputs(c)["y"]
    shards = [_device(c, lo, hi) for lo, hi in R.SHARDS]
    ref = R.reference(c)
    _check(combine_partials_numpy([dm.partial(y) for dm in shards], c.N), ref, "f partial " + _id(c))
    _check(combine_partials_numpy([dm.partial64(y) for dm in shards], c.N), ref, "f partial64 " + _id(c))
    shift = max(dm.cconst_max() for dm in shards)
    _check(combine_packed_numpy([dm.partial_shifted(y, shift) for dm in shards]), ref, "f shifted " + _id(c))


# ---- g: small amplitudes on the inexact path -------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.cases_g(), ids=_id)
def test_g_small_amplitudes(c):
    """The inexact path scales the batch by a power of two taken from its largest entry before the y_hi + y_lo
    split, so the bars hold at every amplitude.  (With the unscaled split this case measured, at 32x32 / 128x128:
    s = 1e-2: 1.7e-6 / 3.4e-6 rel_fro; s = 1e-3: 2.2e-5 / 2.8e-5, worst row 4.1e-4 / 4.4e-4; s = 1e-4: 3.2e-4 /
    4.9e-4, worst row 4.6e-3 / 1.3e-2.)"""
    dm = _device(c)
    _check(dm.estimate(R.inputs(c)["y"]), R.reference(c), "g " + _id(c))


def test_exact_path_is_bit_identical_to_the_unscaled_kernels():
    """The observation scale of the inexact path must not touch exact observations: h and the partial's accumulator
    of the two (64, 64) 1-bit cases equal, bit for bit, what the kernels gave before that scale existed (recorded on
    an MI355X from a build of the preceding commit, run in its own process)."""
    import os
    from conftest import GOLDEN
    gold = np.load(os.path.join(GOLDEN, "fast_exact_64x64.npz"))
    for tag, c in zip(("m0", "m1"), R.EXACT_PIN):
        y = R.inputs(c)["y"]
        dm = _device(c)
        np.testing.assert_array_equal(np.asarray(dm.estimate(y))[R.EXACT_PIN_ROWS], gold[tag])
        np.testing.assert_array_equal(np.asarray(dm.partial(y)[2])[R.EXACT_PIN_ROWS], gold[tag + "_acc"])
