"""Float64 NumPy restatement of one VAE training step (reference estimators/vae.py:108-123: DNN_VAE.forward, vae_loss,
backward, Adam): the arbiter of tests/test_gpu_vae_step.py and the subject of tests/test_vae_step_ref_cpu.py.

The network is written with plain matrix products on whole (B, width) arrays; the loss and its gradients with respect to
the encoder and decoder outputs come from tests/vae_train_ref.py; the backward pass is the chain rule written out layer
by layer.  It shares no code and no summation order with csrc/qce_vae_step.hip.

``w``: {state-dict name: array}; ``x`` (n, P, 2N) (or (n, 2N)); ``t`` (T, 2N); row b uses row ``index[b]`` of x, t and
``snr_db`` (or row b); ``eps`` (B, L).
"""
import numpy as np

import vae_train_ref as R


def _count(w, prefix):
    return sum(1 for k in w if k.startswith(prefix) and k.endswith(".weight"))


def forward(w, x, eps, mode):
    """(enc (B, 2L), dec (B, N), cache for ``backward``) in float64."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    a = np.asarray(x, dtype=np.float64)
    cache = {"w": w, "conv": [], "enc": [], "dec": []}
    nconv = 0 if mode == "genie" else _count(w, "pre_pilot.conv")
    if a.ndim == 3 and nconv == 0:
        a = a[:, 0, :]
    for i in range(nconv):  # kernel size 1: a channel mix per position
        cw, cb = w[f"pre_pilot.conv{i}.weight"][:, :, 0], w[f"pre_pilot.conv{i}.bias"]
        out = np.maximum(np.einsum("oc,bcq->boq", cw, a) + cb[None, :, None], 0.0)
        cache["conv"].append((a, out))
        a = out
    if nconv:
        a = a[:, 0, :]
    nl = _count(w, "enc.linear")
    for i in range(nl):
        out = a @ w[f"enc.linear{i}.weight"].T + w[f"enc.linear{i}.bias"]
        if i < nl - 1:
            out = np.maximum(out, 0.0)
        cache["enc"].append((a, out))
        a = out
    enc = a
    L = enc.shape[1] // 2
    eps = np.asarray(eps, dtype=np.float64)
    a = enc[:, :L] + np.exp(enc[:, L:]) * eps
    for i in range(nl):
        out = a @ w[f"dec.linear{i}.weight"].T + w[f"dec.linear{i}.bias"]
        if i < nl - 1:
            out = np.maximum(out, 0.0)
        cache["dec"].append((a, out))
        a = out
    cache["eps"] = eps
    return enc, a, cache


def _mlp_backward(w, name, layers, g, grads):
    """Back through the linear layers ``layers`` = [(input, output)]; g: the gradient of the last output."""
    nl = len(layers)
    for i in range(nl - 1, -1, -1):
        a, out = layers[i]
        if i < nl - 1:
            g = g * (out > 0)
        grads[f"{name}.linear{i}.weight"] = g.T @ a
        grads[f"{name}.linear{i}.bias"] = g.sum(axis=0)
        g = g @ w[f"{name}.linear{i}.weight"]
    return g


def loss_and_grads(w, x, t, eps, mode, n_bits=1, snr_db=None, index=None):
    """(loss, rows (B,), {name: d loss / d parameter}) in float64."""
    x = np.asarray(x, dtype=np.float64)
    if index is not None:
        x = x[np.asarray(index).astype(np.int64)]
    enc, dec, cache = forward(w, x, eps, mode)
    wd = cache["w"]
    rows = R.elbo_rows(enc, dec, t, mode, n_bits, snr_db, index)
    g_enc, g_dec = R.loss_grads(enc, dec, t, mode, n_bits, snr_db, index)
    grads = {}
    g_z = _mlp_backward(wd, "dec", cache["dec"], g_dec, grads)
    g = g_enc + R.reparameterize_bwd(enc, cache["eps"], g_z)
    g = _mlp_backward(wd, "enc", cache["enc"], g, grads)
    if cache["conv"]:
        g = g[:, None, :]
        for i in range(len(cache["conv"]) - 1, -1, -1):
            a, out = cache["conv"][i]
            g = g * (out > 0)
            grads[f"pre_pilot.conv{i}.weight"] = np.einsum("boq,bcq->oc", g, a)[:, :, None]
            grads[f"pre_pilot.conv{i}.bias"] = g.sum(axis=(0, 2))
            g = np.einsum("oc,boq->bcq", wd[f"pre_pilot.conv{i}.weight"][:, :, 0], g)
    for k in wd:  # parameters the forward does not use (a genie network's convolutions)
        grads.setdefault(k, np.zeros_like(wd[k]))
    return -float(np.mean(rows)), rows, {k: grads[k] for k in wd}


def adam(w, m, v, g, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step of torch.optim.Adam (defaults: no weight decay, no amsgrad) in float64 on {name: array} dicts; ``step``
    is the count before this step.  Returns (w, m, v, step + 1)."""
    t = step + 1
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    w2, m2, v2 = {}, {}, {}
    for k in w:
        gk = np.asarray(g[k], dtype=np.float64)
        m2[k] = beta1 * np.asarray(m[k], dtype=np.float64) + (1 - beta1) * gk
        v2[k] = beta2 * np.asarray(v[k], dtype=np.float64) + (1 - beta2) * gk * gk
        w2[k] = np.asarray(w[k], dtype=np.float64) - lr / bc1 * m2[k] / (np.sqrt(v2[k]) / np.sqrt(bc2) + eps)
    return w2, m2, v2, t
