"""Two-pass form of the FP64 3M estimate kernel (k_est_all_f64g2: a log-prob pass over the GL blocks, one exact
softmax per segment through the per-workgroup scratch, a filter pass over the GW blocks; padded M = 64).

Every case compares the 3M default with the 4M kernel (QCE_F64_3M=0 at prepare: same FP64 computation up to
rounding, 1e-12 relative Frobenius) and with the FP64 oracle (1e-9), at the smallest shapes that reach the new
code's corners: segments that are whole tiles, stream-K slices with klo > 0 and khi < K, whole rounds followed by a
tail; padded dimensions and mean / bias blocks; softmax corners (weights of zero, the exp floor, the maximum in the
last component); reuse of the scratch; and K-split partials merged by the stream-K merge kernel and on the host.

Cases with a pilot matrix A (M != N) are unquantised: with 1 bit and a general A the prepare's arcsine law limits
the agreement with the oracle to ~1e-7 (test_gpu_f64.py), which is not what these cases are about.
"""
import numpy as np
import pytest

from conftest import rel_fro

pytestmark = pytest.mark.gpu

TOL_4M = 1e-12
TOL_ORACLE = 1e-9


def _gpu_or_fail():
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible for a gpu-marked test")


def _model(K, N, seed, mean=False):
    from quantized_channel_estimation_amd import inputs
    means, covs, w = inputs.synthetic_model(K, N, seed=seed)
    if mean:
        means = 0.3 * inputs.crandn(K, N, rng=np.random.default_rng(seed + 7))
    return means, covs, w


def _obs(B, N, seed, A=None, n_bits=1):
    from quantized_channel_estimation_amd import inputs
    rng = np.random.default_rng(seed)
    h, _ = inputs.scm_generate(B, 1, N, rng, n_path=3)
    h = h[:, 0, :].astype(complex)
    return inputs.get_observation_nbit(h, 5.0, A, n_bits, rng=rng)


def _estimates(means, covs, w, ys, monkeypatch, A=None, n_bits=1.0, partial=False):
    """[(h3, h4)] (or partial64 triples) for every y of ys: the 3M default, then the 4M kernel on the same model."""
    from quantized_channel_estimation_amd import _lib
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(A, 5.0, n_bits)
    assert dm.kernel() == "f64_3m"
    r3 = [dm.partial64(y) if partial else dm.estimate(y) for y in ys]
    monkeypatch.setenv("QCE_F64_3M", "0")
    dm.prepare(A, 5.0, n_bits)
    assert dm.kernel() == "f64_4m"
    r4 = [dm.partial64(y) if partial else dm.estimate(y) for y in ys]
    monkeypatch.delenv("QCE_F64_3M")
    dm.close()
    return list(zip(r3, r4))


def _check(h3, h4, ho, what):
    e4, eo = rel_fro(h3, h4), rel_fro(h3, ho)
    print(f"{what}: vs 4M {e4:.3e}, vs oracle {eo:.3e}")
    assert np.isfinite(h3).all(), what
    assert e4 < TOL_4M, (what, e4)
    assert eo < TOL_ORACLE, (what, eo)


@pytest.mark.parametrize("K", [1, 3, 5])
def test_tail_segments_small_batches(K, monkeypatch):
    """B in {1, 17, 129, 300}: fewer tiles than workgroups, every segment a stream-K slice of a tile."""
    _gpu_or_fail()
    from oracle import qce_oracle as O
    N = 64
    means, covs, w = _model(K, N, 700 + K)
    y = _obs(300, N, 710 + K)
    Bs = (1, 17, 129, 300)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    for B, (h3, h4) in zip(Bs, _estimates(means, covs, w, [y[:B] for B in Bs], monkeypatch)):
        _check(h3, h4, ho[:B], f"K={K} B={B}")


def test_whole_rounds_then_tail(monkeypatch):
    """B just above 256 tiles of 128: one data-parallel round of whole tiles on a 256-CU grid, then a cut tail."""
    _gpu_or_fail()
    from oracle import qce_oracle as O
    K, N, B = 4, 64, 33000
    means, covs, w = _model(K, N, 720, mean=True)
    y = _obs(B, N, 721)
    (h3, h4), = _estimates(means, covs, w, [y], monkeypatch)
    rows = np.r_[0:300, B - 300:B]  # the oracle on the first round's and the tail's rows
    ho = O.estimate(means, covs, w, y[rows], 5.0, N, None, "all", 1)
    assert rel_fro(h3, h4) < TOL_4M, rel_fro(h3, h4)
    _check(h3[rows], h4[rows], ho, "rounds + tail")


@pytest.mark.parametrize("wg", ["2", "5"])
def test_forced_grid_cuts_inside_tiles(wg, monkeypatch):
    """K = 7 over 3 tiles: 5 workgroups take 5 items each (slices with klo > 0 and khi < K, e.g. components 1..5 of
    the last tile); 2 workgroups run one whole round and split the third tile 4 + 3."""
    _gpu_or_fail()
    from oracle import qce_oracle as O
    monkeypatch.setenv("QCE_WORKGROUPS", wg)
    K, N, B = 7, 64, 300
    means, covs, w = _model(K, N, 730, mean=True)
    y = _obs(B, N, 731)
    ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    (h3, h4), = _estimates(means, covs, w, [y], monkeypatch)
    _check(h3, h4, ho, f"QCE_WORKGROUPS={wg}")


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("M,N", [(64, 64), (60, 52), (64, 32), (64, 16)])
def test_padded_dimensions_and_means(M, N, mean, monkeypatch):
    """Padded M = 64 with padded N = 64 (exact and from M = 60, N = 52), 32 and 16: each has its own chunk size and
    region lengths; with means the -q0 and bias blocks join the regions."""
    _gpu_or_fail()
    from oracle import qce_oracle as O
    K, B = 5, 200
    means, covs, w = _model(K, N, 740 + N, mean=mean)
    rng = np.random.default_rng(M * N)
    A, nb = None, 1
    if M != N:
        A = (rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))) / np.sqrt(2 * N)
        nb = np.inf
    y = _obs(B, N, 750 + N, A, nb)
    ho = O.estimate(means, covs, w, y, 5.0, N, A, "all", nb)
    (h3, h4), = _estimates(means, covs, w, [y], monkeypatch, A=A, n_bits=nb)
    _check(h3, h4, ho, f"M={M} N={N} mean={mean}")


def _corner_weights(K):
    w0 = np.full(K, 1.0 / K)
    one_zero = w0.copy()
    one_zero[2] = 0.0
    one_zero /= one_zero.sum()
    single = np.zeros(K)
    single[K - 2] = 1.0
    floor = w0.copy()
    floor[1] = 5e-324  # log weight -744: more than 708 below the largest lp, the exp floor
    last_max = np.full(K, 1e-30)
    last_max[K - 1] = 1.0 - (K - 1) * 1e-30  # the last lp exceeds every earlier one by ~69
    return {"one_zero": one_zero, "all_but_one_zero": single, "exp_floor": floor, "max_in_last": last_max}


@pytest.mark.parametrize("corner", ["one_zero", "all_but_one_zero", "exp_floor", "max_in_last"])
def test_softmax_corners(corner, monkeypatch):
    _gpu_or_fail()
    from oracle import qce_oracle as O
    K, N, B = 6, 64, 200
    means, covs, _ = _model(K, N, 760, mean=True)
    w = _corner_weights(K)[corner]
    y = _obs(B, N, 761)
    with np.errstate(divide="ignore"):
        ho = O.estimate(means, covs, w, y, 5.0, N, None, "all", 1)
    (h3, h4), = _estimates(means, covs, w, [y], monkeypatch)
    _check(h3, h4, ho, corner)


def test_scratch_reuse():
    """The scratch keeps nothing between launches: B = 300 then B = 17 on one model, then new parameters (another
    K-slice of a larger mixture) and B = 17 again, each equal to a fresh model's result bit for bit."""
    _gpu_or_fail()
    from quantized_channel_estimation_amd import _lib
    N = 64
    means, covs, w = _model(10, N, 770, mean=True)
    y = _obs(300, N, 771)

    def fresh(lo, hi, yy):
        d = _lib.DeviceModel(means[lo:hi], covs[lo:hi], w[lo:hi])
        d.prepare(None, 5.0, 1.0)
        out = d.estimate(yy)
        d.close()
        return out

    dm = _lib.DeviceModel(means[:5], covs[:5], w[:5])
    dm.prepare(None, 5.0, 1.0)
    dm.estimate(y)
    assert np.array_equal(dm.estimate(y[:17]), fresh(0, 5, y[:17]))
    dm.set_params(means[5:], covs[5:], w[5:])
    dm.prepare(None, 5.0, 1.0)
    assert np.array_equal(dm.estimate(y[:17]), fresh(5, 10, y[:17]))
    dm.close()


def test_k_split_partials_combine(monkeypatch):
    """(m, s, acc) partials of two component ranges -- m now the exact maximum of the range -- combine to the
    whole-range estimate: on the device across a cut tile (k_merge_f64, forced by a 2-workgroup grid over one tile),
    and on the host from the partials of two K-slice models (the K-shard format)."""
    _gpu_or_fail()
    from quantized_channel_estimation_amd import _lib
    from quantized_channel_estimation_amd.sharding import combine_partials_numpy
    K, N, B = 9, 64, 100
    means, covs, w = _model(K, N, 780, mean=True)
    y = _obs(B, N, 781)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, 5.0, 1.0)
    monkeypatch.setenv("QCE_WORKGROUPS", "1")
    whole = dm.estimate(y)  # one workgroup, one segment [0, K)
    m, s, _ = dm.partial64(y)
    monkeypatch.setenv("QCE_WORKGROUPS", "2")
    merged = dm.estimate(y)  # segments [0, 5) and [5, 9) merged by k_merge_f64
    monkeypatch.delenv("QCE_WORKGROUPS")
    dm.close()
    assert rel_fro(merged, whole) < TOL_4M, rel_fro(merged, whole)
    # the partial's m is the exact row maximum: the largest weight is exactly 1, so 1 <= s <= K
    assert np.all(s >= 1.0) and np.all(s <= K) and np.all(np.isfinite(m))
    parts = []
    for lo, hi in [(0, 5), (5, 9)]:
        d = _lib.DeviceModel(means[lo:hi], covs[lo:hi], w[lo:hi])
        d.prepare(None, 5.0, 1.0)
        parts.append(d.partial64(y))
        d.close()
    e = rel_fro(combine_partials_numpy(parts, N), whole)
    print(f"K-split partials vs whole range: {e:.3e}")
    assert e < TOL_4M, e
