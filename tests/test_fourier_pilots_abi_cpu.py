"""The Fourier-path-with-pilots option on the CPU: the Python constants equal the defines of include/qce.h, and the
option is plain state of the estimator object (no device needed to set or pickle it)."""
import os
import pickle
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    txt = open(os.path.join(ROOT, "include", "qce.h")).read()
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", txt, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_constants_equal_the_header():
    from quantized_channel_estimation_amd import _lib
    assert _lib.OPT_FOURIER_PILOTS == _define("QCE_OPT_FOURIER_PILOTS") == 5
    assert _define("QCE_KERNEL_FOURIER_PILOTS") == 8
    assert _lib.DeviceModel.KERNELS[_define("QCE_KERNEL_FOURIER_PILOTS")] == "fourier_pilots"
    # the other options and kernel ids keep their values
    for name in ("BETA_FIRST", "PRECISION", "RESERVE_CUS", "INT8_SLICES"):
        assert getattr(_lib, "OPT_" + name) == _define("QCE_OPT_" + name)
    for kid, kname in _lib.DeviceModel.KERNELS.items():
        assert _define("QCE_KERNEL_" + kname.upper()) == kid


def test_option_pickles_without_a_device():
    from quantized_channel_estimation_amd import Gmm_nbit, Gmm_quant
    for cls in (Gmm_nbit, Gmm_quant):
        g = cls(n_components=3, fourier_pilots=True)
        assert g.fourier_pilots is True and g._dev is None
        g2 = pickle.loads(pickle.dumps(g))
        assert g2.fourier_pilots is True and g2._dev is None
        assert cls(n_components=3).fourier_pilots is False
    # an object pickled before the option existed has no such attribute: it reads as off
    g = Gmm_nbit(n_components=2)
    d = g.__getstate__()
    d.pop("fourier_pilots")
    old = Gmm_nbit.__new__(Gmm_nbit)
    old.__setstate__(d)
    assert not getattr(old, "fourier_pilots", False)
