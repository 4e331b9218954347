"""Child-process helper of tests/test_gpu_prepare.py: the process-wide A/B switches of libqce.so (QCE_CHOL,
QCE_CHOL_PAIRS, QCE_CHOL_THREADS, QCE_ZGEMM) are read once per process, so each setting gets a fresh one.

    python tests/prepare_dump.py OUT.npz [--gemm]

prepares the six dense A = I cases with M <= 64 (with --gemm also the two dense-A cases) and the M = 33 non-PD
mixture under whatever environment it was started with and writes every table and lp as `case__table` to OUT.npz;
`nonpd33` records whether the non-PD mixture raised the Cholesky error.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def prepare_case(dm, name):
    """Prepare DeviceModel `dm` for a case of prepare_ref.CASES."""
    import prepare_ref as R
    from quantized_channel_estimation_amd import _lib
    c = R.case(name)
    lloyd = c["kind"] == "lloyd" and c["n_bits"] not in (1, np.inf)
    dm.prepare(c["A"], c["snr"], float(c["n_bits"]), _lib.QUANT_LLOYD if lloyd else _lib.QUANT_UNIFORM,
               c["thr"] if lloyd else None, c["lab"] if lloyd else None)


def device_model(name):
    import prepare_ref as R
    from quantized_channel_estimation_amd import _lib
    c = R.case(name)
    dm = _lib.DeviceModel(c["means"], c["covs"], c["w"])
    if c["beta_first"]:
        dm.set_option(_lib.OPT_BETA_FIRST, 1)
    return dm


def main(argv):
    import prepare_ref as R
    from quantized_channel_estimation_amd import _lib
    out_path = argv[1]
    names = R.SMALL + (R.SMALL_GEMM if "--gemm" in argv[2:] else ())
    out = {}
    for name in names:
        dm = device_model(name)
        prepare_case(dm, name)
        t = dm.tables()
        t["lp"] = dm.log_prob(R.case(name)["X"])[0]
        out.update({f"{name}__{k}": v for k, v in t.items()})
        out[f"{name}__family"] = np.array(dm.kernel())
        dm.close()
    means, covs, w = R.nonpd_mixture(33)
    dm = _lib.DeviceModel(means, covs, w)
    dm.prepare(None, 300.0, float("inf"))
    try:
        dm.estimate(R.case("ok33")["X"])
        out["nonpd33"] = np.array("no error")
    except ValueError as e:
        out["nonpd33"] = np.array(str(e))
    dm.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv)
