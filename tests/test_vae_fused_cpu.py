"""qce_vae_net_create refuses before any device call (include/qce.h; csrc/qce_capi_vae_net.hip), so every refusal can
be checked without a GPU: the status code, and a message in qce_last_error."""
import ctypes

import numpy as np
import pytest

from quantized_channel_estimation_amd import _lib


def _widths(N, P, L, nl, npc):
    return [np.linspace(P, 1, npc + 1, dtype=int), np.linspace(2 * N, 2 * L, nl + 1, dtype=int),
            np.linspace(L, N, nl + 1, dtype=int)]


def _count(parts):
    return int(sum(int(w[i + 1]) * int(w[i]) + int(w[i + 1]) for w in parts for i in range(len(w) - 1)))


def _create(N=16, P=1, L=4, nl=2, npc=0, genie=0, parts=None, n_weights=None, null=None):
    """(status, message) of one qce_vae_net_create on zero weights."""
    lib = _lib.load()
    parts = _widths(N, P, L, nl, npc) if parts is None else parts
    widths = np.concatenate(parts).astype(np.int32)
    n = _count(parts) if n_weights is None else n_weights
    weights = np.zeros(max(n, 1), np.float32)
    out = ctypes.c_void_p()
    rc = lib.qce_vae_net_create(N, P, L, nl, npc, genie, None if null == "widths" else _lib.ptr(widths),
                                None if null == "weights" else _lib.ptr(weights), n, _lib.IO_HOST, 0,
                                None if null == "out" else ctypes.byref(out))
    assert rc != _lib.QCE_OK and not out.value
    return rc, lib.qce_last_error().decode()


@pytest.mark.parametrize("kw", [dict(N=48), dict(N=8), dict(N=512), dict(P=5, npc=2), dict(L=0), dict(L=129, N=256),
                                dict(nl=0), dict(nl=9), dict(P=4, npc=5)],
                         ids=["N48", "N8", "N512", "P5", "L0", "L129", "nl0", "nl9", "npc5"])
def test_not_implemented_shapes(kw):
    rc, msg = _create(**kw)
    assert rc == _lib.QCE_ENOTIMPL, msg
    assert msg.startswith("vae_net_create: ")


def test_width_above_512_is_not_implemented():
    parts = _widths(64, 1, 16, 2, 0)
    parts[1][1] = 600
    rc, msg = _create(N=64, L=16, parts=parts)
    assert rc == _lib.QCE_ENOTIMPL and "512" in msg


@pytest.mark.parametrize("which", ["conv0", "conv_last", "enc0", "enc_last", "dec0", "dec_last"])
def test_inconsistent_widths(which):
    N, P, L, nl, npc = 16, 2, 4, 2, 1
    parts = _widths(N, P, L, nl, npc)
    part, idx = {"conv0": (0, 0), "conv_last": (0, -1), "enc0": (1, 0), "enc_last": (1, -1), "dec0": (2, 0),
                 "dec_last": (2, -1)}[which]
    parts[part][idx] += 1
    rc, msg = _create(N=N, P=P, L=L, nl=nl, npc=npc, parts=parts)
    assert rc == _lib.QCE_EARG, msg
    assert "inconsistent widths" in msg


def test_pilots_without_convs():
    rc, msg = _create(P=2, npc=0)
    assert rc == _lib.QCE_EARG and "n_pilot_convs" in msg


def test_weight_count():
    n = _count(_widths(16, 1, 4, 2, 0))
    for wrong in (n - 1, n + 1, 0):
        rc, msg = _create(n_weights=wrong)
        assert rc == _lib.QCE_EARG and str(n) in msg, msg


@pytest.mark.parametrize("null", ["widths", "weights", "out"])
def test_null_pointers(null):
    rc, msg = _create(null=null)
    assert rc == _lib.QCE_EARG and "null" in msg


def test_destroy_null_is_a_no_op():
    assert _lib.load().qce_vae_net_destroy(None) == _lib.QCE_OK


def test_forward_refuses_a_null_handle():
    rc = _lib.load().qce_vae_net_forward(None, None, 1, 0, None, None, None, None, 0.0, 1.0, None, _lib.IO_HOST, None)
    assert rc == _lib.QCE_EARG
