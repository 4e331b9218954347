"""Scenarios for one long-lived ``DeviceModel`` handle -- TEST INFRASTRUCTURE ONLY (CPU: NumPy and the oracle).

A scenario is a handle (tests/handle_history.py ``HANDLES``) and an ordered list of steps.  A step is a ``set_params``
(``params``), an option change (``option``), a ``prepare`` or a call that reads prepared state (``call``).  Everything a
step needs is built from seeds that depend on the scenario's name and the step's index only, so a step's inputs and
its oracle result do not depend on which steps were evaluated before it, and ``replay_fresh`` can run one step alone
on a fresh handle: create, apply the options in force, run the last prepare, make that one call.

The scenario tables carry tags (``TRANSITIONS`` lists the required ones) and, per prepare, the kernel family the shape
must land in; tests/test_handle_history_cpu.py checks both as data, tests/test_gpu_handle_history.py walks the handles.
"""
import collections
import functools
import os
import sys
import zlib

import numpy as np

if __name__ == "__main__":  # `python tests/handle_history.py` prints the SALT table of the scenario tables
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import qce_oracle as O

INF = float("inf")

# ---- handles and their parameter sets ----------------------------------------------------------------------------------
Handle = collections.namedtuple("Handle", "N K cov blocks")
HANDLES = {
    "full40": Handle(40, 5, "full", None),
    "full72": Handle(72, 3, "full", None),
    "circ32": Handle(32, 5, "circulant", None),
    "bcirc64": Handle(64, 5, "block-circulant", (4, 16)),
}

KERNEL_NAMES = ("none", "f64_4m", "f64_3m", "f64_wide", "big", "fourier", "fast", "int8", "fourier_pilots")

# every transition the scenario tables must contain (a tag on the step that follows the transition)
TRANSITIONS = (
    "M_shrinks_in_pad", "M_grows_in_pad",                                    # 40 -> 24 -> 40
    "3m_to_4m", "4m_to_wide", "wide_to_big", "big_to_3m",                    # across padded sizes and families
    "mean_to_zero", "zero_to_mean", "M_grows_after_zero_mean",               # the q0 / bvec zero counters
    "b1_to_lloyd3", "lloyd3_to_uniform2", "uniform2_to_inf", "inf_to_b1",     # thr / lab, y_scale, the int8 group
    "f64_to_fast", "fast_to_int8s5", "int8s5_to_int8s7", "int8s7_to_f64",     # precision at one shape
    "beta_first_on", "beta_first_off", "reserve_0_16", "reserve_16_0",
    "fourier_tables_replay", "fourier_after_replay", "fourier_tables_replay_again",
    "fourier_assigned", "fourier_after_assigned", "fourier_cconst_then_estimate",
    "fourier_to_pilots", "pilots_to_dense_A", "dense_A_to_identity",
    "structure_flips_to_full", "structure_flips_back",
    "lazy_all_top3_lp:f64_3m", "lazy_lp_top3_all:f64_3m", "lazy_all_top3_lp:f64_wide", "lazy_lp_top3_all:f64_wide",
    "lazy_all_top3_lp:big", "lazy_lp_top3_all:big",
    "batch_130_7_24",
    "refused_partial_int8", "after_refused_partial", "refused_prepare_chol", "after_refused_prepare",
)

SELECTIVE = {"est_top1": 1, "est_top3": 3, "est_p09": 0.9}
MARGIN = 1e-6  # the smallest selection margin a scenario row may have (tests/test_handle_history_cpu.py)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (1 << 30)


@functools.lru_cache(maxsize=None)
def params(handle, name):
    """(means, covs, w) of a named parameter set of a handle.  'zero' / 'mean': the handle's own covariance type without
    and with means; 'full_mean': a 'full' mixture with means on a (block-)circulant handle (structure detection flips);
    'bad': 'mean' with component 1 made indefinite (eigenvalue -5) -- the reference's ValueError at the Cholesky."""
    from quantized_channel_estimation_amd import inputs
    hd = HANDLES[handle]
    cov = "full" if name in ("full_mean",) else hd.cov
    means, covs, w = inputs.synthetic_model(hd.K, hd.N, cov_type=cov, seed=_seed(handle, "model") % 1000 + 1,
                                            blocks=hd.blocks if cov != "full" else None)
    if name != "zero":
        means = 0.3 * inputs.crandn(hd.K, hd.N, rng=np.random.default_rng(_seed(handle, "means")))
    if name == "bad":
        covs = covs.copy()
        covs[1] = np.eye(hd.N)
        covs[1, 0, 1] = covs[1, 1, 0] = 6.0
    for a in (means, covs, w):
        a.flags.writeable = False
    return means, covs, w


@functools.lru_cache(maxsize=None)
def matrix(handle, name):
    """The observation matrix of a name: None (A = I), 'rectM' (seeded Gaussian, M rows), 'pP' (kron(x, I_N), P pilots,
    the reference's angle_amp pilots), 'dense' (seeded Gaussian, N rows: not kron(x, I))."""
    from quantized_channel_estimation_amd import inputs
    if name is None:
        return None
    N = HANDLES[handle].N
    if name.startswith("p"):
        A = inputs.get_pilot_matrix(N, int(name[1:]), 1, "angle_amp")
    else:
        M = N if name == "dense" else int(name[4:])
        rng = np.random.default_rng(_seed(handle, name))
        A = (rng.standard_normal((M, N)) + 1j * rng.standard_normal((M, N))) / np.sqrt(2 * N)
    A = np.ascontiguousarray(A, dtype=complex)
    A.flags.writeable = False
    return A


@functools.lru_cache(maxsize=None)
def quantizer(snr, n_bits, qtype):
    from quantized_channel_estimation_amd import inputs
    if n_bits in (1, INF):
        return (None, None, None)
    return inputs.get_quantizer([snr], int(n_bits), qtype)[snr]


# ---- steps -----------------------------------------------------------------------------------------------------------
def P(name, *tags):
    return dict(op="params", name=name, tags=tags)


def OPT(name, value, *tags):
    """name: 'precision' ('f64' | 'fast' | ('int8', S)), 'beta_first', 'reserve_cus', 'fourier_pilots'"""
    return dict(op="option", name=name, value=value, tags=tags)


def PREP(A, snr, n_bits, kernel, *tags, qtype="uniform", fails=False):
    return dict(op="prepare", A=A, snr=float(snr), n_bits=float(n_bits), qtype=qtype, kernel=kernel, fails=fails,
                tags=tags)


def C(name, B=24, io="host", *tags, raises=None):
    return dict(op="call", name=name, B=B, io=io, tags=tags, raises=raises)


def _lazy(order_tag, B=24):
    """The lazily built tables (pack32 / pack64 / WT / big_ws) in both orders on a fresh prepare each."""
    if order_tag.startswith("lazy_all"):
        return [C("est_all", B, "host", order_tag), C("est_top3", B, "dev"), C("lp", B)]
    return [C("lp", B, "host", order_tag), C("est_top3", B, "dev"), C("est_all", B)]


def _stale(B=24):
    """Before a transition: every lazy table built (a selective-mode call, a log_prob, an estimate_assigned)."""
    return [C("est_p09", B), C("lp", B), C("assigned", B)]


SNR_A, SNR_B, SNR_C = -10.0, -5.0, -14.0

SCENARIOS = collections.OrderedDict()

# N = 40, 'full': M inside one padded size, then across padded sizes and families, means toggled through set_params
SCENARIOS["full40_shapes"] = ("full40", "mean", [
    PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 130), *_stale(),
    PREP("rect24", SNR_B, 2, "f64_3m", "M_shrinks_in_pad"), C("est_all", 24), C("est_top3", 7, "dev"), C("partial64", 24),
    C("tables", 7), C("ls_general", 7, raises=NotImplementedError), *_stale(),
    PREP(None, SNR_A, 1, "f64_3m", "M_grows_in_pad"), C("est_all", 130, "dev"), C("est_top1", 24), C("partial", 7),
    C("partial_shifted", 24, "dev"), C("ls", 7), C("ls_general", 7), C("cconst_max", 1), *_stale(),
    PREP("p2", SNR_B, 1, "f64_4m", "3m_to_4m"), C("est_all", 130), C("est_top3", 24), C("partial64", 7, "dev"),
    C("partial_shifted", 24), C("ls", 7), *_stale(),
    PREP("p4", SNR_A, 2, "f64_wide", "4m_to_wide"), C("est_all", 130), C("est_top1", 7, "dev"), C("partial", 24),
    C("partial64", 24), C("partial_shifted", 7), C("tables", 7), *_stale(),
    PREP("p7", SNR_C, 1, "big", "wide_to_big"), C("est_all", 24), C("est_top3", 7), C("est_p09", 24, "dev"), C("lp", 130),
    C("partial64", 7), C("partial_shifted", 24), C("cconst_max", 1), C("assigned", 7, raises=NotImplementedError),
    PREP(None, SNR_B, 3, "f64_3m", "big_to_3m"), C("est_all", 130), C("est_top3", 24), C("lp", 7), C("assigned", 24),
    # means -> zero means -> means (q0_zeroed / bvec_zeroed), with M growing right after the zero-mean prepare
    PREP("p2", SNR_A, 1, "f64_4m"), *_stale(),
    P("zero", "mean_to_zero"), PREP("rect24", SNR_B, 1, "f64_3m"), C("est_all", 24), C("est_p09", 7), C("partial64", 24),
    C("tables", 7),
    PREP("p2", SNR_B, 1, "f64_4m", "M_grows_after_zero_mean"), C("est_all", 130), C("est_top3", 24), C("assigned", 7),
    C("partial_shifted", 7), C("tables", 7),
    P("mean", "zero_to_mean"), PREP("p2", SNR_B, 1, "f64_4m"), C("est_all", 24), C("est_top1", 7), C("tables", 7),
    # an E-step on the handle (set_params, the channel-domain prepare, qce_em_estep), then an estimate's prepare again
    P("zero"), PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 24), C("estep", 24), PREP(None, SNR_B, 1, "f64_3m"),
    C("est_all", 7), C("est_top3", 24),
])

# quantisers at one shape under f64, int8 and fast (thr / lab, y_scale, the int8 group)
def _quantisers(on_grid, off_grid):
    """on_grid: the family the 1-bit and uniform prepares land in; off_grid: the Lloyd and unquantised ones"""
    return [
        PREP(None, SNR_A, 1, on_grid), C("est_all", 130), C("est_top3", 24), C("lp", 24),
        PREP(None, SNR_B, 3, off_grid, "b1_to_lloyd3", qtype="lloyd"), C("est_all", 24), C("est_p09", 7), C("lp", 7),
        PREP(None, SNR_A, 2, on_grid, "lloyd3_to_uniform2"), C("est_all", 130, "dev"), C("est_top3", 24),
        PREP(None, SNR_B, INF, off_grid, "uniform2_to_inf"), C("est_all", 24), C("est_top1", 7), C("lp", 24),
        PREP(None, SNR_A, 1, on_grid, "inf_to_b1"), C("est_all", 24), C("est_top3", 7, "dev"), C("lp", 7),
    ]


SCENARIOS["full40_quantisers_f64"] = ("full40", "mean", _quantisers("f64_3m", "f64_3m"))
SCENARIOS["full40_quantisers_int8"] = ("full40", "mean", [OPT("precision", ("int8", 7))] + _quantisers("int8", "f64_3m") +
                                       [C("i8_products", 24)])
SCENARIOS["full40_quantisers_fast"] = ("full40", "mean", [OPT("precision", "fast")] + _quantisers("fast", "fast"))

# precision, beta_first and reserve_cus at one shape; the refused calls
SCENARIOS["full40_options"] = ("full40", "mean", [
    PREP("rect24", SNR_B, 2, "f64_3m"), C("est_all", 130), *_stale(),
    OPT("precision", "fast", "f64_to_fast"), PREP("rect24", SNR_B, 2, "fast"), C("est_all", 130), C("est_top3", 24),
    C("partial", 24), C("partial64", 7, "dev"), C("partial_shifted", 7), C("lp", 24), C("assigned", 7),
    OPT("precision", ("int8", 5), "fast_to_int8s5"), PREP("rect24", SNR_B, 2, "int8"), C("est_all", 130),
    C("est_top3", 24), C("i8_products", 7), C("lp", 24),
    C("partial", 24, raises=NotImplementedError), C("est_all", 7, "dev", "refused_partial_int8"),
    P("mean"), PREP("rect24", SNR_A, 2, "int8", "after_refused_partial"), C("est_all", 24), C("i8_products", 24),
    OPT("precision", ("int8", 7), "int8s5_to_int8s7"), PREP("rect24", SNR_B, 2, "int8"), C("est_all", 130),
    C("i8_products", 7), C("est_p09", 24),
    OPT("precision", "f64", "int8s7_to_f64"), PREP("rect24", SNR_B, 2, "f64_3m"), C("est_all", 130), C("est_top3", 24),
    C("partial64", 24),
    # the same prepares through the wide shapes under 'fast' and 'int8' (int8 falls back to the f64 families there)
    OPT("precision", "fast"), PREP("p2", SNR_A, 2, "fast"), C("est_all", 130), C("est_top3", 24), C("lp", 7),
    PREP("p4", SNR_A, 2, "fast"), C("est_all", 24), C("partial", 7),
    PREP("p7", SNR_C, 1, "big"), C("est_all", 7),
    OPT("precision", ("int8", 7)), PREP("p2", SNR_A, 2, "f64_4m"), C("est_all", 24), PREP("p4", SNR_A, 2, "f64_wide"),
    C("est_all", 7), PREP(None, SNR_A, 1, "int8"), C("est_all", 24),
    OPT("precision", "f64"),
    OPT("beta_first", 1, "beta_first_on"), PREP("p2", SNR_A, 1, "f64_4m"), C("est_all", 24), C("est_top3", 7), C("lp", 7),
    OPT("beta_first", 0, "beta_first_off"), PREP("p2", SNR_A, 1, "f64_4m"), C("est_all", 24), C("lp", 7),
    PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 130), C("partial64", 130),
    OPT("reserve_cus", 16, "reserve_0_16"), C("est_all", 130), C("partial64", 130), C("est_top3", 24),
    OPT("reserve_cus", 0, "reserve_16_0"), C("est_all", 130), C("partial_shifted", 130),
    # a prepare that fails with the reference's ValueError, then a valid set_params + prepare
    P("bad"), PREP(None, SNR_B, INF, "f64_3m", "refused_prepare_chol", fails=True),
    P("mean"), PREP(None, SNR_B, INF, "f64_3m", "after_refused_prepare"), C("est_all", 24), C("est_top3", 7), C("lp", 7),
    C("tables", 7),
])

# the lazy tables in both orders on a fresh prepare each; the batch history at one prepare
SCENARIOS["full40_lazy_orders"] = ("full40", "mean", [
    PREP("rect24", SNR_B, 2, "f64_3m"), *_lazy("lazy_all_top3_lp:f64_3m"),
    PREP("rect24", SNR_B, 2, "f64_3m"), *_lazy("lazy_lp_top3_all:f64_3m"),
    PREP("p4", SNR_A, 2, "f64_wide"), *_lazy("lazy_all_top3_lp:f64_wide"),
    PREP("p4", SNR_A, 2, "f64_wide"), *_lazy("lazy_lp_top3_all:f64_wide"),
    PREP("p7", SNR_C, 1, "big"), *_lazy("lazy_all_top3_lp:big", 7),
    PREP("p7", SNR_C, 1, "big"), *_lazy("lazy_lp_top3_all:big", 7),
    PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 130, "host", "batch_130_7_24"), C("est_all", 7, "dev"),
    C("est_all", 24, "host"), C("est_top3", 130, "dev"), C("est_top3", 7, "host"), C("est_top3", 24, "dev"),
    C("lp", 130), C("lp", 7), C("partial64", 130, "dev"), C("partial64", 7, "host"), C("partial64", 24, "dev"),
])

# N = 72: the padded-128 3M kernel and the two-pass path
SCENARIOS["full72"] = ("full72", "mean", [
    PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 130), C("est_top3", 24), C("partial64", 24), C("partial_shifted", 7),
    *_stale(),
    PREP("p2", SNR_B, 2, "f64_wide"), C("est_all", 130, "dev"), C("est_top1", 24), C("partial", 7), *_stale(7),
    P("zero"), PREP(None, SNR_B, 2, "f64_3m"), C("est_all", 24), C("est_p09", 7), C("partial64", 130), C("tables", 7),
    P("mean"), PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 7), C("lp", 24), C("estep", 24),
])


# (block-)circulant handles: the Fourier families, the dense replay, the stored A, structure detection
def _fourier(handle):
    dense_p2 = "f64_3m" if handle == "circ32" else "f64_4m"
    return (handle, "zero", [
        PREP(None, SNR_A, 1, "fourier"), C("est_all", 130), C("est_top3", 24), C("lp", 24), C("partial", 7),
        C("partial64", 24, "dev"), C("partial_shifted", 7),
        C("tables", 24, "host", "fourier_tables_replay"), C("est_all", 24), C("est_p09", 7),
        PREP(None, SNR_B, 2, "fourier", "fourier_after_replay"), C("est_all", 24),
        C("tables", 7, "host", "fourier_tables_replay_again"), C("est_top1", 24),
        P("mean"), PREP(None, SNR_A, 1, "fourier"), C("est_all", 130), C("lp", 7),
        C("assigned", 24, "host", "fourier_assigned"), C("ls", 7), C("est_top3", 24),
        PREP(None, SNR_B, 3, "fourier", "fourier_after_assigned", qtype="lloyd"), C("est_all", 24),
        C("cconst_max", 1), C("est_all", 7, "dev", "fourier_cconst_then_estimate"), C("est_top3", 24), C("partial64", 7),
        OPT("fourier_pilots", 1), PREP("p2", SNR_A, 1, "fourier_pilots", "fourier_to_pilots"), C("est_all", 130),
        C("est_top3", 24), C("lp", 24), C("partial", 7, raises=NotImplementedError), C("tables", 7), C("assigned", 7),
        C("est_p09", 24, "dev"),
        PREP("dense", SNR_B, 2, "f64_3m", "pilots_to_dense_A"), C("est_all", 24),
        C("est_top3", 7), C("tables", 7),
        PREP(None, SNR_A, 1, "fourier", "dense_A_to_identity"), C("est_all", 24), C("tables", 7), C("lp", 7),
        OPT("fourier_pilots", 0), PREP("p2", SNR_A, 1, dense_p2), C("est_all", 24), C("est_top3", 7), C("lp", 7),
        P("full_mean", "structure_flips_to_full"), PREP(None, SNR_A, 1, "f64_3m"), C("est_all", 24), C("est_top3", 7),
        C("tables", 7),
        P("zero", "structure_flips_back"), PREP(None, SNR_B, 1, "fourier"), C("est_all", 130), C("est_top3", 24),
        C("tables", 7), C("estep", 24),
        OPT("precision", ("int8", 7)), PREP(None, SNR_A, 1, "fourier"), C("est_all", 24), C("cconst_max", 1),
        OPT("precision", "fast"), PREP(None, SNR_A, 1, "fourier"), C("est_all", 7), C("tables", 7), C("est_all", 24),
    ])


SCENARIOS["circ32"] = _fourier("circ32")
SCENARIOS["bcirc64"] = _fourier("bcirc64")


# ---- the state a step runs in ------------------------------------------------------------------------------------------
DEFAULT_OPTIONS = (("precision", "f64"), ("beta_first", 0), ("fourier_pilots", 0), ("reserve_cus", 0))
Context = collections.namedtuple("Context", "handle params options prepare")


def contexts(scn):
    """Per step of a scenario: the Context in force when the step runs (for a prepare / params / option step: after
    it).  ``prepare`` is the last prepare step's index or None when a set_params or option change dropped it."""
    handle, pname, steps = SCENARIOS[scn]
    opts = dict(DEFAULT_OPTIONS)
    prep = None
    out = []
    for i, s in enumerate(steps):
        if s["op"] == "params":
            pname, prep = s["name"], None
        elif s["op"] == "option":
            opts[s["name"]] = s["value"]
            if s["name"] != "reserve_cus":  # the prepared tables stay valid
                prep = None
        elif s["op"] == "prepare":
            prep = None if s["fails"] else i
        elif s["name"] == "estep" and s["raises"] is None:
            prep = i  # DeviceEM.estep re-prepares: A = I, sigma^2 = 0, no quantisation
        out.append(Context(handle, pname, tuple(sorted(opts.items(), key=lambda kv: repr(kv[0]))), prep))
    return out


def prepare_args(scn, idx):
    """(A name, snr, n_bits, qtype) of the prepare step (or estep call) idx"""
    s = SCENARIOS[scn][2][idx]
    if s["op"] == "call":
        return (None, INF, INF, "uniform")
    return (s["A"], s["snr"], s["n_bits"], s["qtype"])


def call_steps(scn):
    """[(idx, step, context before the call)]: for an estep the prepare in force is its own"""
    ctx = contexts(scn)
    return [(i, s, ctx[i]) for i, s in enumerate(SCENARIOS[scn][2]) if s["op"] == "call"]


def family(scn, idx):
    """The kernel family named by the prepare in force at call step idx"""
    c = contexts(scn)[idx]
    s = SCENARIOS[scn][2][c.prepare]
    if s["op"] == "call":  # estep's own prepare: the channel-domain model
        hd = HANDLES[c.handle]
        if hd.cov != "full" and c.params != "full_mean":
            return "fourier"
        return "f64_3m"
    return s["kernel"]


# ---- inputs ------------------------------------------------------------------------------------------------------------
# Seeds of the steps whose first seed put a row closer than MARGIN to a selection boundary (the search that found them
# took the first salt with every margin above 1e-4): (scenario, step) -> salt
SALT = {("full40_shapes", 27): 28, ("full40_shapes", 47): 1, ("full40_shapes", 55): 3, ("full40_shapes", 70): 16,
        ("full40_quantisers_fast", 11): 1, ("full40_lazy_orders", 10): 5, ("full40_lazy_orders", 22): 2,
        ("bcirc64", 38): 1}


POOL = 160


@functools.lru_cache(maxsize=None)
def channel_pool(handle):
    """POOL SCM channels of a handle's N, drawn once (1.3 ms each); a step picks its rows and draws its noise by its
    own seed."""
    from quantized_channel_estimation_amd import inputs
    h, _ = inputs.scm_generate(POOL, 1, HANDLES[handle].N, np.random.default_rng(_seed(handle, "channels")), n_path=3)
    h = h[:, 0, :].astype(complex)
    h.flags.writeable = False
    return h


@functools.lru_cache(maxsize=None)
def inputs_of(scn, idx):
    """y (B, M) of call step idx at its prepare's own SNR and quantiser, component indices, the int8 debug component."""
    from quantized_channel_estimation_amd import inputs
    s = SCENARIOS[scn][2][idx]
    c = contexts(scn)[idx]
    hd = HANDLES[c.handle]
    Aname, snr, nb, qtype = prepare_args(scn, c.prepare)
    rng = np.random.default_rng(_seed(scn, idx, SALT.get((scn, idx), 0)))
    h = channel_pool(c.handle)[rng.choice(POOL, size=s["B"], replace=False)]
    if s["name"] == "estep":
        y = inputs.get_observation_nbit(h, 10.0, None, INF, rng=rng)
    else:
        qz = quantizer(snr, nb, qtype)
        y = inputs.get_observation_nbit(h, snr, matrix(c.handle, Aname), INF if nb == INF else int(nb), qz[0], qz[1],
                                        rng=rng)
    y = np.ascontiguousarray(y, dtype=np.complex128)
    comp = rng.integers(0, hd.K, size=s["B"]).astype(np.int64)
    k = int(rng.integers(0, hd.K))
    for a in (y, comp):
        a.flags.writeable = False
    return dict(y=y, comp=comp, k=k)


# ---- oracle ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_tables(handle, pname, Aname, snr, nb, qtype):
    means, covs, w = params(handle, pname)
    N = HANDLES[handle].N
    A = matrix(handle, Aname)
    A = np.eye(N, dtype=complex) if A is None else A
    if snr == INF:  # the channel-domain model of DeviceEM.estep: Cr = C, A_eff = I
        t = O.prepare(means, covs, A, 300.0, INF)
    else:
        t = O.prepare(means, covs, A, snr, INF if nb == INF else int(nb), qtype, quantizer(snr, nb, qtype))
    t["W"], t["b"] = O._filters(means, covs, t)
    t["cconst"] = -A.shape[0] * O.LOG_PI + 2 * np.real(O.log_det_cholesky(t["P"])) + np.log(w)
    return t


def oracle_tables(scn, idx):
    c = contexts(scn)[idx]
    return _oracle_tables(c.handle, c.params, *prepare_args(scn, c.prepare))


def shift_of(scn, idx):
    """The shift of a partial_shifted step: the oracle's largest c_k rounded down (a fresh handle gets the same)."""
    return float(np.floor(np.max(oracle_tables(scn, idx)["cconst"])))


def _weighted(t, w, y, wts):
    hk = np.einsum("knm,bm->bkn", t["W"], y) + t["b"][None]
    return np.einsum("bk,bkn->bn", wts, hk)


def selection_weights(proba, mode):
    """The oracle's selective-mode weights (oracle/qce_oracle.py estimate): top-n / cumulative-p, renormalised."""
    B, K = proba.shape
    w = np.zeros((B, K))
    order = np.argsort(proba, axis=1)[:, ::-1]
    if isinstance(mode, int):
        n = np.full(B, min(mode, K))
    else:
        cs = np.cumsum(np.take_along_axis(proba, order, axis=1), axis=1)
        n = np.array([np.searchsorted(cs[i], mode) + 1 for i in range(B)])
    for i in range(B):
        ks = order[i, :n[i]]
        w[i, ks] = proba[i, ks] / np.sum(proba[i, ks])
    return w


def oracle_of(scn, idx):
    """The FP64 oracle's result of call step idx: the keys of run_call's result that the oracle defines."""
    s = SCENARIOS[scn][2][idx]
    c = contexts(scn)[idx]
    _, _, w = params(c.handle, c.params)
    t = oracle_tables(scn, idx)
    d = inputs_of(scn, idx)
    y, name = d["y"], s["name"]
    out = {}
    if name in ("est_all", "partial", "partial64", "partial_shifted", "lp", "estep") or name in SELECTIVE:
        wlp = O.weighted_log_prob(y, t["means_y"], t["P"], w)
        proba = O.predict_proba(y, t["means_y"], t["P"], w)
    if name == "est_all" or name.startswith("partial"):
        out["h"] = _weighted(t, w, y, proba)
    elif name == "est_top1":
        out["h"] = _weighted(t, w, y, np.eye(len(w))[wlp.argmax(axis=1)])
    elif name in SELECTIVE:
        out["h"] = _weighted(t, w, y, selection_weights(proba, SELECTIVE[name]))
    elif name == "lp":
        out.update(lp=wlp, proba=proba, labels=wlp.argmax(axis=1))
    elif name == "estep":
        from scipy.special import logsumexp
        out.update(resp=proba, mean_lse=float(np.mean(logsumexp(wlp, axis=1))))
    elif name == "tables":
        out.update({k: t[k] for k in ("means_y", "Cy", "Cr", "P", "A_eff", "W", "b", "cconst")})
    elif name == "cconst_max":
        out["cconst_max"] = float(np.max(t["cconst"]))
    elif name == "assigned":
        out["h"] = np.einsum("bnm,bm->bn", t["W"][d["comp"]], y) + t["b"][d["comp"]]
    elif name in ("ls", "ls_general"):
        out["h"] = np.stack([np.linalg.lstsq(t["A_eff"][k], y[b], rcond=None)[0] for b, k in enumerate(d["comp"])])
    return out


def margins(scn, idx):
    """Smallest selection margins over the rows of a selective-mode (or log_prob) step: the gap between the n-th and
    (n+1)-th largest oracle probability, the distance of the cumulative sums from 0.9, the top-two lp gap."""
    s = SCENARIOS[scn][2][idx]
    c = contexts(scn)[idx]
    _, _, w = params(c.handle, c.params)
    t = oracle_tables(scn, idx)
    y = inputs_of(scn, idx)["y"]
    wlp = np.sort(O.weighted_log_prob(y, t["means_y"], t["P"], w), axis=1)[:, ::-1]
    pr = np.sort(O.predict_proba(y, t["means_y"], t["P"], w), axis=1)[:, ::-1]
    K = pr.shape[1]
    out = dict(lp_gap=float(np.min(wlp[:, 0] - wlp[:, 1])))
    if s["name"] == "est_top3" and K > 3:
        out["rank_gap"] = float(np.min(pr[:, 2] - pr[:, 3]))
    if s["name"] == "est_p09":
        out["cum_gap"] = float(np.min(np.abs(np.cumsum(pr, axis=1) - 0.9)))
    return out


# ---- running a step on a handle (GPU) ------------------------------------------------------------------------------------
def apply_option(dm, name, value):
    if name == "precision":
        if isinstance(value, tuple):
            dm.set_precision(value[0], slices=value[1])
        else:
            dm.set_precision(value)
    elif name == "beta_first":
        from quantized_channel_estimation_amd import _lib
        dm.set_option(_lib.OPT_BETA_FIRST, float(value))
    elif name == "fourier_pilots":
        dm.set_fourier_pilots(bool(value))
    elif name == "reserve_cus":
        dm.reserve_cus(int(value))
    else:
        raise KeyError(name)


def run_prepare(dm, handle, Aname, snr, nb, qtype):
    from quantized_channel_estimation_amd import _lib
    qz = quantizer(snr, nb, qtype)
    kind = _lib.QUANT_LLOYD if (qtype == "lloyd" and nb not in (1, INF)) else _lib.QUANT_UNIFORM
    thr, lab = (qz[0], qz[1]) if kind == _lib.QUANT_LLOYD else (None, None)
    dm.prepare(matrix(handle, Aname), snr, nb, kind, thr, lab)


def run_call(dm, scn, idx):
    """Make call step idx on `dm` and return its results as a dict of NumPy arrays / scalars."""
    import torch
    from quantized_channel_estimation_amd import _em, _lib
    s = SCENARIOS[scn][2][idx]
    c = contexts(scn)[idx]
    d = inputs_of(scn, idx)
    name, y = s["name"], d["y"]
    dev = s["io"] == "dev"
    yy = torch.from_numpy(np.array(y)).to(f"cuda:{dm.device}") if dev else y  # y is read-only: a copy
    host = lambda a: a.cpu().numpy() if dev else np.array(a)
    if name == "est_all" or name in SELECTIVE:
        mode = {"est_all": (_lib.MODE_ALL, 0.0), "est_top1": (_lib.MODE_TOPN, 1.0), "est_top3": (_lib.MODE_TOPN, 3.0),
                "est_p09": (_lib.MODE_CUMP, 0.9)}[name]
        return dict(h=host(dm.estimate(yy, *mode)))
    if name == "lp":
        lp, pr, lab = dm.log_prob(y, True, True, True)
        return dict(lp=lp, proba=pr, labels=lab)
    if name in ("partial", "partial64"):
        m, sm, acc = getattr(dm, name)(yy)
        return dict(m=host(m), s=host(sm), acc=host(acc).astype(np.float64))
    if name == "partial_shifted":
        return dict(packed=host(dm.partial_shifted(yy, shift_of(scn, idx))))
    if name == "tables":
        return dm.tables()
    if name == "cconst_max":
        return dict(cconst_max=dm.cconst_max())
    if name in ("assigned", "ls", "ls_general"):
        ls = {"assigned": False, "ls": True, "ls_general": "general"}[name]
        return dict(h=dm.estimate_assigned(y, d["comp"], ls=ls))
    if name == "i8_products":
        raw_l, raw_w, exps = dm.debug_i8_products(y, d["k"])
        return dict(raw_l=raw_l, raw_w=raw_w, exps=exps)
    if name == "estep":
        means, covs, w = params(c.handle, c.params)
        em = _em.DeviceEM(y, HANDLES[c.handle].K, "full", 0.0, False, device=dm.device)
        em._dm = dm  # the E-step of a fit on a model that has a history: set_params, prepare, qce_em_estep
        mean_lse = em.estep(means, covs, w)
        resp = em.R.cpu().numpy()
        em._dm = None
        return dict(resp=resp, mean_lse=mean_lse)
    raise KeyError(name)


def fresh_handle(scn, idx, with_prepare=True):
    """A fresh handle in the state call step idx runs in: created with the parameters in force, the options in force
    applied, the last prepare run."""
    from quantized_channel_estimation_amd import _lib
    c = contexts(scn)[idx]
    dm = _lib.DeviceModel(*params(c.handle, c.params))
    for name, value in c.options:
        if (name, value) not in DEFAULT_OPTIONS:
            apply_option(dm, name, value)
    s = SCENARIOS[scn][2][idx]
    if with_prepare and not (s["op"] == "call" and s["name"] == "estep"):
        run_prepare(dm, c.handle, *prepare_args(scn, c.prepare))
    return dm


def replay_fresh(scn, idx):
    """One step alone on a fresh handle: (result, kernel(), structure())"""
    dm = fresh_handle(scn, idx)
    try:
        res = run_call(dm, scn, idx)
        return res, dm.kernel(), dm.structure()
    finally:
        dm.close()


# ---- one level up: a scrambled script loop on one Gmm_nbit / Gmm_quant object ---------------------------------------------
# (snr, n_bits, quantiser, A, mode) in non-monotone order; before entry SCRIPT_EDIT_AT the means are edited in place
SCRIPT = [
    (-10.0, 1, "uniform", None, "all"), (-5.0, 3, "lloyd", "p2", 0.9), (-10.0, 2, "uniform", "rect24", 3),
    (-5.0, INF, "uniform", None, 1), (-14.0, 1, "uniform", "p7", "all"), (-10.0, 2, "uniform", "p4", 3),
    (-5.0, 1, "uniform", None, "all"), (-10.0, 2, "uniform", "rect24", 3), (-5.0, 1, "uniform", "p2", 0.9),
]
SCRIPT_EDIT_AT = 5
SCRIPT_B = 24
SCRIPT_SALT = {5: 3, 8: 1}  # as SALT


def script_params(j):
    means, covs, w = params("full40", "mean")
    if j >= SCRIPT_EDIT_AT:
        means = means.copy()
        means[0] *= 1.5
    return means, covs, w


@functools.lru_cache(maxsize=None)
def script_inputs(j):
    from quantized_channel_estimation_amd import inputs
    snr, nb, qtype, Aname, _ = SCRIPT[j]
    rng = np.random.default_rng(_seed("script", j, SCRIPT_SALT.get(j, 0)))
    h = channel_pool("full40")[rng.choice(POOL, size=SCRIPT_B, replace=False)]
    qz = quantizer(snr, nb, qtype)
    y = inputs.get_observation_nbit(h, snr, matrix("full40", Aname), nb, qz[0], qz[1], rng=rng)
    y = np.ascontiguousarray(y, dtype=np.complex128)
    y.flags.writeable = False
    return y


def script_oracle(j):
    """h of entry j, and the observation-domain proba / labels the object reports after it"""
    snr, nb, qtype, Aname, mode = SCRIPT[j]
    means, covs, w = script_params(j)
    y = script_inputs(j)
    A = matrix("full40", Aname)
    A = np.eye(40, dtype=complex) if A is None else A
    h, t = O.estimate(means, covs, w, y, snr, 40, A, mode, nb, qtype, quantizer(snr, nb, qtype), return_tables=True)
    wlp = O.weighted_log_prob(y, t["means_y"], t["P"], w)
    pr = O.predict_proba(y, t["means_y"], t["P"], w)
    return dict(h=h, proba=pr, labels=wlp.argmax(axis=1), wlp=wlp)


def script_margins(j):
    r = script_oracle(j)
    wlp = np.sort(r["wlp"], axis=1)[:, ::-1]
    pr = np.sort(r["proba"], axis=1)[:, ::-1]
    out = dict(lp_gap=float(np.min(wlp[:, 0] - wlp[:, 1])))
    if SCRIPT[j][4] == 3:
        out["rank_gap"] = float(np.min(pr[:, 2] - pr[:, 3]))
    if SCRIPT[j][4] == 0.9:
        out["cum_gap"] = float(np.min(np.abs(np.cumsum(pr, axis=1) - 0.9)))
    return out


def find_salts(target=1e-4, tries=400):
    """The SALT table for the scenario tables as they stand (run after editing them: step indices shift)."""
    out = {}
    saved = dict(SALT)
    SALT.clear()
    for scn in SCENARIOS:
        for i, s, _ in call_steps(scn):
            if s["raises"] is not None or not (s["name"] in SELECTIVE or s["name"] == "lp"):
                continue
            for salt in range(tries):
                SALT[(scn, i)] = salt
                inputs_of.cache_clear()
                if min(margins(scn, i).values()) > target:
                    break
            else:
                raise RuntimeError(f"no seed keeps {scn} step {i} away from its selection boundaries")
            if SALT.pop((scn, i)):
                out[(scn, i)] = salt
    SALT.update(saved)
    inputs_of.cache_clear()
    return out


if __name__ == "__main__":
    print("SALT =", find_salts())
