"""The handle-history scenarios (tests/handle_history.py) hold without a GPU: every required transition and kernel
family is in the tables, no row of a selective-mode step sits within 1e-6 of a selection boundary (so the GPU test
excludes no row), and a step's inputs and oracle result do not depend on the order steps are evaluated in."""
import numpy as np
import pytest

import handle_history as H


def _steps():
    for scn, (_, _, steps) in H.SCENARIOS.items():
        for i, s in enumerate(steps):
            yield scn, i, s


def test_every_transition_is_tagged():
    tags = [t for _, _, s in _steps() for t in s["tags"]]
    missing = [t for t in H.TRANSITIONS if t not in tags]
    assert not missing, missing
    unknown = sorted(set(tags) - set(H.TRANSITIONS))
    assert not unknown, unknown


def test_every_kernel_family_is_named():
    """... by a prepare that succeeds and is followed by an 'all'-mode estimate; 'none' is what kernel() reports
    after a set_params or an option change (the GPU test reads it there)."""
    named = set()
    for scn, (_, _, steps) in H.SCENARIOS.items():
        ctx = H.contexts(scn)
        for i, s in enumerate(steps):
            if s["op"] == "call" and s["name"] == "est_all" and s["raises"] is None:
                named.add(H.family(scn, i))
            if s["op"] in ("params", "option") and ctx[i].prepare is None:
                named.add("none")
    assert named == set(H.KERNEL_NAMES), set(H.KERNEL_NAMES) ^ named


def test_tags_sit_on_the_transition_they_name():
    """The data behind a few tags: the prepare a tag sits on differs from the prepare before it in the named way."""
    for scn, (handle, _, steps) in H.SCENARIOS.items():
        ctx = H.contexts(scn)
        preps = [i for i, s in enumerate(steps) if s["op"] == "prepare"]
        N = H.HANDLES[handle].N
        rows = lambda i: N if steps[i]["A"] is None else H.matrix(handle, steps[i]["A"]).shape[0]
        for a, b in zip(preps, preps[1:]):
            t = steps[b]["tags"]
            if "M_shrinks_in_pad" in t:
                assert rows(b) < rows(a) <= 64 and steps[a]["kernel"] == steps[b]["kernel"]
            if "M_grows_in_pad" in t:
                assert rows(a) < rows(b) <= 64
            if "M_grows_after_zero_mean" in t:
                assert rows(b) > rows(a) and ctx[a].params == ctx[b].params == "zero"
            for tag, (ka, kb) in {"3m_to_4m": ("f64_3m", "f64_4m"), "4m_to_wide": ("f64_4m", "f64_wide"),
                                  "wide_to_big": ("f64_wide", "big"), "big_to_3m": ("big", "f64_3m"),
                                  "fourier_to_pilots": ("fourier", "fourier_pilots")}.items():
                if tag in t:
                    assert (steps[a]["kernel"], steps[b]["kernel"]) == (ka, kb), (scn, b, tag)
            if t and not steps[b]["fails"] and any(x in t for x in ("3m_to_4m", "4m_to_wide", "wide_to_big",
                                                                    "M_shrinks_in_pad", "M_grows_in_pad")):
                # the earlier prepare built every lazy table: a selective mode, a log_prob, an estimate_assigned
                before = [s["name"] for s in steps[a:b] if s["op"] == "call" and s["raises"] is None]
                assert {"lp", "assigned"} <= set(before) and set(before) & set(H.SELECTIVE), (scn, b)
                assert steps[a]["snr"] != steps[b]["snr"], (scn, b)
        batches = {s["B"] for s in steps if s["op"] == "call"}
        assert batches <= {1, 7, 24, 130}


@pytest.mark.parametrize("scn", list(H.SCENARIOS))
def test_no_row_near_a_selection_boundary(scn):
    """Zero excluded rows: every margin of every selective-mode and log_prob step exceeds 1e-6."""
    worst = {}
    for i, s, _ in H.call_steps(scn):
        if s["raises"] is None and (s["name"] in H.SELECTIVE or s["name"] == "lp"):
            for k, v in H.margins(scn, i).items():
                assert v > H.MARGIN, (scn, i, s["name"], k, v)
                worst[k] = min(v, worst.get(k, np.inf))
    print(scn, {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst


def test_script_loop_rows_are_away_from_selection_boundaries():
    for j in range(len(H.SCRIPT)):
        for k, v in H.script_margins(j).items():
            assert v > H.MARGIN, (j, k, v)
    modes = [e[4] for e in H.SCRIPT]
    assert {"all", 1, 3, 0.9} <= set(modes) and 0 < H.SCRIPT_EDIT_AT < len(H.SCRIPT)
    snrs = [e[0] for e in H.SCRIPT]
    assert snrs != sorted(snrs) and snrs != sorted(snrs, reverse=True)


def test_oracle_results_do_not_depend_on_evaluation_order():
    scn = "full40_quantisers_f64"
    idx = [i for i, s, _ in H.call_steps(scn) if s["raises"] is None]

    def evaluate(order):
        H.inputs_of.cache_clear()
        H._oracle_tables.cache_clear()
        return {i: (H.inputs_of(scn, i), H.oracle_of(scn, i)) for i in order}

    fwd, rev = evaluate(idx), evaluate(idx[::-1])
    for i in idx:
        assert np.array_equal(fwd[i][0]["y"], rev[i][0]["y"]) and np.array_equal(fwd[i][0]["comp"], rev[i][0]["comp"])
        assert fwd[i][1].keys() == rev[i][1].keys() and fwd[i][1]
        for k in fwd[i][1]:
            assert np.array_equal(fwd[i][1][k], rev[i][1][k]), (i, k)


def test_contexts_follow_the_steps():
    """A set_params or an option other than reserve_cus drops the prepare; reserve_cus keeps it; a failed prepare
    leaves none; an estep is its own prepare."""
    for scn, (_, _, steps) in H.SCENARIOS.items():
        ctx = H.contexts(scn)
        for i, s in enumerate(steps):
            if s["op"] == "params" or (s["op"] == "option" and s["name"] != "reserve_cus"):
                assert ctx[i].prepare is None
            if s["op"] == "option" and s["name"] == "reserve_cus":
                assert ctx[i].prepare == ctx[i - 1].prepare is not None
            if s["op"] == "prepare":
                assert ctx[i].prepare == (None if s["fails"] else i)
            if s["op"] == "call":
                assert ctx[i].prepare is not None, (scn, i)  # every call has a prepare to read
