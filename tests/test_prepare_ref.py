"""CPU checks of the extended-precision prepare reference (tests/prepare_ref.py), without a GPU:

  * against the reference project's own tables recorded in tests/golden/model_*.npz, at the bounds the kernels are held
    to -- this pins the restatement to the reference where its outputs are recorded;
  * against the FP64 NumPy oracle on every case of the GPU matrix: e_oracle per table and case is printed and must
    itself stay inside the bound, component by component (e_oracle is a whole-table figure) -- a correct FP64
    computation can meet the bounds of tests/test_gpu_prepare.py;
  * every non-PD input of that file makes both the long double Cholesky loop and the oracle raise.
"""
import numpy as np
import pytest

import prepare_ref as R
from conftest import MODELS, case_args


def _golden_cases(golden_models):
    for mname in MODELS:
        fx = golden_models[mname]
        for tag in fx["cases"]:
            tag = str(tag)
            if f"{tag}__Cy" in fx:
                yield mname, fx, tag


def test_reference_matches_golden_tables(golden_models):
    """The fixtures record Cy, Cr, P, A_eff of components 0, 1, means_y and lp of all (the reference's own FP64
    results).  Bound as in prepare_ref: the fixture is an FP64 computation like the oracle, so its error against the
    long double tables is held to max(F * e_oracle, G M u kappa) with e_oracle measured on the same inputs."""
    from oracle import qce_oracle as O
    n = 0
    for mname, fx, tag in _golden_cases(golden_models):
        y, snr, N, A, n_bits, qtype, quantizer = case_args(fx, tag)
        means, covs, w = fx["means_cplx"], fx["covs_cplx"], fx["weights"]
        K, M = covs.shape[0], A.shape[0]
        t = R.prepare(means, covs, w, A, snr, n_bits, qtype, quantizer[0], quantizer[1])
        t["lp"] = R.log_prob(t, y)
        o = O.prepare(means, covs, A, snr, n_bits, qtype, quantizer)
        o["lp"] = O.weighted_log_prob(y, o["means_y"], o["P"], w)
        kappa = max(np.linalg.cond(t["Cr"][k].astype(complex)) for k in range(K))
        for tb in ("Cy", "Cr", "P", "A_eff", "means_y", "lp"):
            rows = slice(None) if tb in ("means_y", "lp") else slice(0, 2)
            ref = t[tb][rows]
            e_fix = R.error(tb, fx[f"{tag}__{tb}"], ref)
            e_orc = R.error(tb, o[tb][rows], ref)
            bound = max(R.F * e_orc, R.G * M * R.U * (kappa if tb in R.KAPPA_TABLES else 1.0))
            print(f"{mname}/{tag:8s} {tb:8s} fixture {e_fix:.2e}  e_oracle {e_orc:.2e}  bound {bound:.2e}")
            assert e_fix <= bound, (mname, tag, tb, e_fix, bound)
        n += 1
    assert n >= 6


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_meets_the_bounds(name):
    """e_oracle[table, case], printed; a correct FP64 computation stays inside the floor G M u kappa_t or -- where the
    inputs amplify (arcsine law near |rho| = 1, 1 bit with a non-identity A) -- defines the bound through F."""
    c, ref, eo = R.case(name), R.reference(name), R.oracle_errors(name)
    o = R.oracle_tables(name)
    for tb in R.TABLES + ("lp",):
        worst = max(R.error(tb, R.component(tb, o[tb], k), R.component(tb, ref[tb], k)) / R.bound(name, tb, k)
                    for k in range(c["K"]))
        print(f"{name:22s} M={c['M']:3d} {tb:8s} e_oracle {eo[tb]:.2e}  floor {R.floor(name, tb, 0):.2e}  "
              f"kappa {ref['kappa'].max():.1e}  worst component / bound {worst:.3f}")
        assert worst <= 1.0, (name, tb, worst)


def test_other_quantiser_kind_and_asymptotic_step():
    """The two branches no matrix case of the oracle comparison names by itself: an unknown multi-bit quantiser type
    (gain 0: Cr = diag(Cy), means_y = 0, W = 0) and the step 4 sqrt(b) 2^-b above 8 bits."""
    from oracle import qce_oracle as O
    c = R.case("n16_inf_mu")
    t = R.prepare(c["means"], c["covs"], c["w"], None, 5.0, 3, "other")
    o = O.prepare(c["means"], c["covs"], np.eye(16), 5.0, 3, "foo")
    assert not t["gain"].any() and not t["means_y"].any() and not t["W"].any()
    for tb in ("Cy", "Cr", "P"):
        e = R.error(tb, o[tb], t[tb])
        print(f"other kind {tb:3s} e_oracle {e:.2e}")
        assert e <= R.G * 16 * R.U
    assert R.error("b", c["means"], t["b"]) == 0.0
    for nb in (9, 12):
        assert abs(float(R.uniform_step(5.0, nb)) - O.uniform_step(5.0, nb)) <= 4 * R.U * O.uniform_step(5.0, nb)


@pytest.mark.parametrize("M", R.NONPD_M)
def test_nonpd_inputs_raise_in_both(M):
    from oracle import qce_oracle as O
    means, covs, w = R.nonpd_mixture(M)
    for k in (0, 1):
        R.cholesky_lower(covs[k].astype(R.CLD))
        O.precision_cholesky(covs[k:k + 1])
    with pytest.raises(ValueError) as ei:
        R.prepare(means, covs, w, None, 300.0, np.inf)
    assert str(ei.value) == O.CHOL_ERROR
    with pytest.raises(ValueError) as ei:
        O.prepare(means, covs, np.eye(M), 300.0, np.inf)
    assert str(ei.value) == O.CHOL_ERROR
    # every leading minor but the last is positive: the loop fails at the last pivot only
    S = covs[2].astype(R.CLD)
    R.cholesky_lower(S[:M - 1, :M - 1])
