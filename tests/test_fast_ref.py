"""CPU checks of tests/fast_ref.py, the arithmetic model behind the bars of tests/test_gpu_fast.py: over the whole
case matrix the model is finite and its derived bar stays inside the project's 1e-5 bar; its own error is pinned at
two cases; and a model with one a_lo product or one slice scale wrong leaves the bars by far more than their factor,
so a kernel with that defect cannot pass them."""
import numpy as np
import pytest

import fast_ref as R

# e_model_fro, e_model_row of the model as committed (an edit of the model shows up here)
PINNED = {
    (R.case(3, 64, 64, 300, 1, False), "h2"): (2.25614e-07, 2.19410e-06),
    (R.case(3, 28, 12, 300, np.inf, True), "h2"): (2.37685e-07, 2.94467e-06),
}


def _id(p):
    c, tables, mode = p
    return f"{tables}-{mode}-K{c.K}-{c.M}x{c.N}-B{c.B}-b{c.n_bits}-m{int(c.mean)}-s{c.scale:g}"


@pytest.mark.parametrize("p", R.all_cases(), ids=_id)
def test_model_is_finite_and_inside_the_project_bar(p):
    c, tables, mode = p
    ref = R.reference(c, tables, mode)
    print(_id(p), f"e_model_fro {ref['e_model_fro']:.3e} e_model_row {ref['e_model_row']:.3e}")
    assert np.isfinite(ref["h"]).all()
    assert R.F * ref["e_model_fro"] <= R.H_TOL, ref["e_model_fro"]


@pytest.mark.parametrize("key", list(PINNED), ids=lambda k: _id((k[0], k[1], "all")))
def test_model_error_is_pinned(key):
    ref = R.reference(*key)
    fro, row = PINNED[key]
    assert ref["e_model_fro"] == pytest.approx(fro, rel=1e-3)
    assert ref["e_model_row"] == pytest.approx(row, rel=1e-3)


@pytest.mark.parametrize("mutation", [dict(drop_lo=True), dict(bad_slice=1)], ids=["a_lo dropped", "slice scale"])
def test_bars_discriminate(mutation):
    """A kernel that drops the a_lo products, or applies a wrong scale to one 32-row slice, computes what the mutated
    model computes: far outside F x the model's error, whole batch and worst row."""
    c = R.case(3, 64, 64, 300, 1, False)
    ref = R.reference(c)
    bad = R.model(c, **mutation)
    fro_bar, row_bar = R.bars(ref)
    assert bad["e_model_fro"] > 10 * fro_bar, (bad["e_model_fro"], fro_bar)
    assert bad["e_model_row"] > 10 * row_bar, (bad["e_model_row"], row_bar)
