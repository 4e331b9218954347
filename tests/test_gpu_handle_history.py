"""A model handle's results do not depend on its history (csrc/qce_model.h: the reused buffers and the flags that say
which lazily built tables belong to the current prepare).

Every scenario of tests/handle_history.py walks one long-lived DeviceModel through its steps.  After every call that
reads prepared state the result is held

a. to the same call made alone on a fresh handle (created, the options in force applied, the last prepare run): worst
   row, 1e-12 -- the project's bar for the same FP64 arithmetic on another schedule (tests/test_gpu_hostio.py,
   test_snr_sweep_double_buffered_matches_serial); labels, the int8 digit-plane sums, kernel() and structure() equal.
   The kernels use no floating-point atomics, so the two are expected to be bit-equal; the count is printed.
b. to the FP64 oracle, at the bar the family's own test uses for that kind of case (``_bars``).

No row is excluded anywhere (tests/test_handle_history_cpu.py keeps every row away from its selection boundaries).
"""
import numpy as np
import pytest

import fast_ref as R
import fourier_pilots_ref as FP
import handle_history as H
import int8_ref as I8
from conftest import rel_fro

pytestmark = pytest.mark.gpu

SAME_TOL = 1e-12  # tests/test_gpu_hostio.py, tests/test_gpu_f64.py test_snr_sweep_double_buffered_matches_serial


def _lib():
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")
    return _lib


# ---- a: against the fresh handle -----------------------------------------------------------------------------------------
def _rows(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1, 1)


def worst_row(a, b):
    """max over rows of ||a_r - b_r|| / ||b_r|| (a zero reference row must be matched exactly)"""
    a, b = _rows(a), _rows(b)
    if a.shape != b.shape or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return np.inf
    d, n = np.linalg.norm(a - b, axis=1), np.linalg.norm(b, axis=1)
    return float(np.max(np.where(n > 0, d / np.where(n > 0, n, 1.0), np.where(d > 0, np.inf, 0.0))))


def scaled_abs(a, b):
    """max |a - b| / max(1, |b|): log-probabilities and other log-domain scalars"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.shape != b.shape or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return np.inf
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


EXACT = ("labels", "raw_l", "raw_w", "exps")
LOG_DOMAIN = ("lp", "m", "cconst", "cconst_max", "mean_lse")
PROBA = ("proba", "resp")


def against_fresh(got, fresh):
    """[(key, error, bar)] of the keys that miss, and whether every key is bit-equal"""
    miss = []
    assert got.keys() == fresh.keys()
    sc = np.exp(got["m"] - fresh["m"])[:, None] if "m" in got else None  # (m, s, acc): one running maximum
    for k in got:
        g, f = np.asarray(got[k]), np.asarray(fresh[k])
        if k in EXACT:
            if not np.array_equal(g, f):
                miss.append((k, float(np.sum(g != f)) if g.shape == f.shape else np.inf, 0.0))
        elif k in LOG_DOMAIN:
            e = scaled_abs(g, f)
            if not e <= SAME_TOL:
                miss.append((k, e, SAME_TOL))
        elif k in PROBA:
            if g.shape != f.shape or not np.allclose(g, f, rtol=1e-12, atol=1e-15, equal_nan=False):
                miss.append((k, float(np.max(np.abs(g - f))) if g.shape == f.shape else np.inf, 1e-12))
        else:  # estimates, partial accumulators, tables: per row
            if k in ("s", "acc"):
                g = g.reshape(g.shape[0], -1) * sc
            e = worst_row(g, f)
            if not e <= SAME_TOL:
                miss.append((k, e, SAME_TOL))
    biteq = all(np.array_equal(np.asarray(got[k]), np.asarray(fresh[k])) for k in got)
    return miss, biteq


# ---- b: against the oracle ----------------------------------------------------------------------------------------------
def _bars(scn, idx):
    """(h rel_fro, (lp rtol, lp atol), (proba rtol, proba atol), table sensitivity) of the case a step is."""
    fam = H.family(scn, idx)
    c = H.contexts(scn)[idx]
    Aname, _, nb, _ = H.prepare_args(scn, c.prepare)
    if fam in ("fourier", "fourier_pilots"):
        # tests/fourier_pilots_ref.py bars (the A = I Fourier path's, tests/test_gpu_parity.py
        # test_fourier_path_vs_oracle_and_dense); proba: test_gpu_fourier_pilots._proba_rtol, atol 1e-13
        h, rtol, atol = FP.bars(1 if nb == 1 else nb)
        return h, (rtol, atol), (1e-4 if nb == 1 else 1e-7, 1e-13), 1e4 if (nb == 1 and Aname is not None) else 1.0
    if nb == 1 and Aname is not None:
        # 1 bit with a non-identity A, the arcsine law at |rho| ~ 1: tests/test_gpu_configs.py
        # test_wide_dimensions_all_modes (h 1e-6, proba rtol 1e-6 / atol 1e-12), lp and the tables' sensitivity:
        # tests/test_gpu_parity.py test_logprob_proba_labels_after_estimate / test_prepare_tables_match_reference
        return 1e-6, (1e-8, 1e-6), (1e-5, 1e-12), 1e4
    # A = I, or more than one bit: tests/test_gpu_f64.py F64_TOL; lp (1e-10, 1e-8) and proba rtol 1e-7 / atol 1e-13:
    # tests/test_gpu_parity.py test_logprob_proba_labels_after_estimate
    return 1e-9, (1e-10, 1e-8), (1e-7, 1e-13), 1.0


def _h_bar(scn, idx, name):
    """The estimate's bar: the case's, or the fast family's cap where fp16-split / FP32 kernels produce it."""
    fam = H.family(scn, idx)
    h = _bars(scn, idx)[0]
    if name in ("assigned", "ls", "ls_general"):
        return h  # FP64 dense tables under every precision
    if fam == "fast" or (fam == "int8" and name in H.SELECTIVE):
        return R.H_TOL  # tests/fast_ref.py: the cap of every fast-family bar (int8: f32 selection weights, as 'fast')
    if name == "partial":
        return max(h, 1e-6)  # an f32 accumulator by its ABI: tests/test_gpu_f64.py test_f64_partials_combine
    return h


def _int8_slices(scn, idx):
    prec = dict(H.contexts(scn)[idx].options)["precision"]
    return prec[1] if isinstance(prec, tuple) else None


def _int8_contract(scn, idx):
    """h of the int8 contract (tests/int8_ref.py) at the step's S on a fresh handle's own tables"""
    c = H.contexts(scn)[idx]
    Aname, snr, nb, _ = H.prepare_args(scn, c.prepare)
    hd = H.HANDLES[c.handle]
    y = H.inputs_of(scn, idx)["y"]
    dm = H.fresh_handle(scn, idx)
    try:
        t = dm.tables(("means_y", "P", "W", "b", "cconst"))
    finally:
        dm.close()
    case = R.case(hd.K, y.shape[1], hd.N, 8, int(nb), c.params != "zero", snr)
    ref = I8.model(case, _int8_slices(scn, idx), tables=t, y=y, with_oracle=False)
    assert ref["on_grid"].all()
    return ref["h"]


TABLE_BARS = dict(Cy=(1e-12, 0), Cr=(1e-12, 1), P=(1e-10, 1), A_eff=(1e-12, 0), means_y=(1e-12, 0), W=(1e-9, 1))


def against_oracle(scn, idx, name, got):
    """[(key, error, bar)] of what misses the oracle"""
    from quantized_channel_estimation_amd.sharding import combine_packed_numpy, combine_partials_numpy
    ref = H.oracle_of(scn, idx)
    hbar, (lrt, lat), (prt, pat), sens = _bars(scn, idx)
    N = H.HANDLES[H.SCENARIOS[scn][0]].N
    miss = []

    def hold(key, e, bar):
        if not e < bar:
            miss.append((key + "@oracle", float(e), bar))

    def close(key, a, b, rtol, atol):
        a, b = np.asarray(a), np.asarray(b)
        if not np.allclose(a, b, rtol=rtol, atol=atol):
            miss.append((key + "@oracle", float(np.max(np.abs(a - b) - rtol * np.abs(b))), atol))

    if name == "est_all" and H.family(scn, idx) == "int8" and _int8_slices(scn, idx) != 7:
        # tests/test_gpu_int8.py sets no oracle bar below the default S = 7; its bar at another S is the contract
        # model at that S on the device's own tables, 1e-12 (test_2_same_s_model_every_shape)
        hold("h(int8 contract)", rel_fro(got["h"], _int8_contract(scn, idx)), SAME_TOL)
    elif name == "est_all" or name in H.SELECTIVE or name in ("assigned", "ls", "ls_general"):
        hold("h", rel_fro(got["h"], ref["h"]), _h_bar(scn, idx, name))
    elif name in ("partial", "partial64"):
        hold("h(partial)", rel_fro(combine_partials_numpy([(got["m"], got["s"], got["acc"])], N), ref["h"]),
             _h_bar(scn, idx, name))
    elif name == "partial_shifted":
        hold("h(packed)", rel_fro(combine_packed_numpy([got["packed"]]), ref["h"]), _h_bar(scn, idx, name))
    elif name == "lp":
        close("lp", got["lp"], ref["lp"], lrt, lat)
        close("proba", got["proba"], ref["proba"], prt, pat)
        if not np.array_equal(got["labels"], ref["labels"]):
            miss.append(("labels@oracle", float(np.sum(got["labels"] != ref["labels"])), 0.0))
    elif name == "estep":
        close("resp", got["resp"], ref["resp"], prt, pat)
        close("mean_lse", got["mean_lse"], ref["mean_lse"], lrt, lat)
    elif name == "cconst_max":
        close("cconst_max", got["cconst_max"], ref["cconst_max"], lrt, lat)
    elif name == "tables":  # tests/test_gpu_parity.py test_prepare_tables_match_reference
        for k, (bar, sensitive) in TABLE_BARS.items():
            hold(k, rel_fro(got[k], ref[k]), bar * (sens if sensitive else 1.0))
        close("cconst", got["cconst"], ref["cconst"], lrt, lat)
    return miss


# ---- the walk -----------------------------------------------------------------------------------------------------------
_walked = {}


def _walk(scn):
    """The walk of a scenario's handle, made once per process (an exception is kept and raised again, never re-run)."""
    if scn not in _walked:
        try:
            _walked[scn] = _walk_once(scn)
        except BaseException as e:  # noqa: BLE001 - kept for the other tests that ask for this walk
            _walked[scn] = e
    if isinstance(_walked[scn], BaseException):
        raise _walked[scn]
    return _walked[scn]


def _walk_once(scn):
    """(misses, kernel names seen, counts).  Every step is checked; the misses are collected so that one run names
    every step a defect reaches."""
    lib = _lib()
    handle, pname, steps = H.SCENARIOS[scn]
    dm = lib.DeviceModel(*H.params(handle, pname))
    misses, seen = [], {dm.kernel()}
    n = dict(calls=0, biteq=0, refused=0)
    worst = dict(fresh=0.0, oracle=0.0)
    try:
        for i, s in enumerate(steps):
            where = f"{scn}[{i}] {s['op']} {s.get('name', s.get('A'))}"
            if s["op"] == "params":
                dm.set_params(*H.params(handle, s["name"]))
                seen.add(dm.kernel())
            elif s["op"] == "option":
                H.apply_option(dm, s["name"], s["value"])
                seen.add(dm.kernel())
            elif s["op"] == "prepare":
                H.run_prepare(dm, handle, s["A"], s["snr"], s["n_bits"], s["qtype"])
                if s["fails"]:  # an error return, not a fault: the reference's message at the first sync point
                    with pytest.raises(ValueError) as err:
                        dm.synchronize()
                    assert str(err.value) == lib.CHOL_MESSAGE
                    n["refused"] += 1
                    continue
                seen.add(dm.kernel())
                if dm.kernel() != s["kernel"]:
                    misses.append((where, "kernel", dm.kernel(), s["kernel"]))
            else:
                if s["raises"] is not None:
                    with pytest.raises(s["raises"]):
                        H.run_call(dm, scn, i)
                    n["refused"] += 1
                    continue
                got = H.run_call(dm, scn, i)
                fresh, fkernel, fstruct = H.replay_fresh(scn, i)
                if (dm.kernel(), dm.structure()) != (fkernel, fstruct):
                    misses.append((where, "kernel/structure", (dm.kernel(), dm.structure()), (fkernel, fstruct)))
                if dm.kernel() != H.family(scn, i):
                    misses.append((where, "family", dm.kernel(), H.family(scn, i)))
                miss, biteq = against_fresh(got, fresh)
                n["calls"] += 1
                n["biteq"] += bool(biteq)
                for key, e, bar in miss:
                    misses.append((where, key + "@fresh", e, bar))
                for key, e, bar in against_oracle(scn, i, s["name"], got):
                    misses.append((where, key, e, bar))
    finally:
        dm.close()
    print(f"{scn}: {n['calls']} calls checked, {n['biteq']} bit-equal to the fresh handle, {n['refused']} refused calls, "
          f"{len(misses)} misses")
    for m in misses:
        print("  MISS", m)
    return tuple(misses), frozenset(seen), n


@pytest.mark.parametrize("scn", list(H.SCENARIOS))
def test_handle_history(scn):
    misses, _, n = _walk(scn)
    assert n["calls"] > 0
    assert not misses, f"{len(misses)} misses, first: {misses[:6]}"


def test_every_kernel_name_was_visited():
    seen = set()
    for scn in H.SCENARIOS:
        seen |= _walk(scn)[1]
    from quantized_channel_estimation_amd import _lib
    assert seen == set(_lib.DeviceModel.KERNELS.values()) == set(H.KERNEL_NAMES), seen


# ---- one level up: the estimator objects through a scrambled script loop --------------------------------------------------
@pytest.mark.parametrize("cls_name", ["Gmm_nbit", "Gmm_quant"])
def test_estimator_object_script_loop(cls_name):
    """One object through (snr, n_bits, quantiser, A, mode) in non-monotone order, predict_proba_cplx / _predict_cplx
    between the estimates and the means edited in place once: every result equals a fresh object's (1e-12 per row)
    and meets the oracle at the case's bar."""
    _lib()
    from quantized_channel_estimation_amd import gmm
    cls = getattr(gmm, cls_name)
    means, covs, w = (np.array(a) for a in H.script_params(0))
    g = cls.from_params(means, covs, w)
    biteq = 0
    for j, (snr, nb, qtype, Aname, mode) in enumerate(H.SCRIPT):
        if j == H.SCRIPT_EDIT_AT:
            g.means_cplx[0] *= 1.5  # in place: the reference re-reads its arrays on every estimate_from_y
        assert np.array_equal(g.means_cplx, H.script_params(j)[0])
        y, A, qz = H.script_inputs(j), H.matrix("full40", Aname), H.quantizer(snr, nb, qtype)
        args = (y, snr, 40, A, mode, nb, qtype, qz)
        got = dict(h=g.estimate_from_y(*args), proba=g.predict_proba_cplx(y), labels=g._predict_cplx(y))
        f = cls.from_params(*(np.array(a) for a in H.script_params(j)))
        fresh = dict(h=f.estimate_from_y(*args), proba=f.predict_proba_cplx(y), labels=f._predict_cplx(y))
        assert g._dev.kernel() == f._dev.kernel()
        miss, eq = against_fresh(got, fresh)
        assert not miss, (j, miss)
        biteq += bool(eq)
        ref = H.script_oracle(j)
        one_bit_general = nb == 1 and Aname is not None
        # the bars of _bars for dense FP64 families
        assert rel_fro(got["h"], ref["h"]) < (1e-6 if one_bit_general else 1e-9), (j, rel_fro(got["h"], ref["h"]))
        np.testing.assert_allclose(got["proba"], ref["proba"], rtol=1e-5 if one_bit_general else 1e-7,
                                   atol=1e-12 if one_bit_general else 1e-13)
        np.testing.assert_array_equal(got["labels"], ref["labels"])
    print(f"{cls_name}: {len(H.SCRIPT)} script entries, {biteq} bit-equal to a fresh object")
