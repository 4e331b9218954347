"""Generate tests/golden/vae_train.npz and vae_train_meta.json: golden vectors for the training side of the VAE
estimator (reference estimators/vae.py: DNN_VAE.vae_loss, DNN_VAE.forward, VAE_nbit.train).

Runs ONLY in the build container (reference imported read-only, no bytecode written), on the CPU.

Loss cases.  The reference model's ``forward`` is replaced by one that returns given float32 leaf tensors
(enc = [mu | log_var_enc], dec = log_var_dec), so ``vae_loss`` and its autograd run on known inputs:

  <tag>__enc, __dec, __t, __snr      the inputs (snr in dB, 'real' only)
  <tag>__loss32, __genc32, __gdec32  the reference in float32 (as it trains)
  <tag>__loss64, __genc64, __gdec64  the same run with every tensor widened to float64

and in the meta file e32 = the reference's own float32-vs-float64 difference, separately for the loss (relative), the
enc gradient and the dec gradient (relative Frobenius).

Network cases.  A seeded reference DNN_VAE, one batch of B = 6; eps is recovered by re-seeding torch before the call
(``forward`` draws it with the first torch.randn after the seed):

  <tag>__w__<name>       the parameters (float32)
  <tag>__x, __t, __snr   encoder input, target, SNRs;  <tag>__eps the draw
  <tag>__loss32, <tag>__g32__<name>, <tag>__g64__<name>   loss and .grad of every parameter, float32 model and .double()

with e32 per parameter tensor in the meta file.

Quirk: the type and message of the exception VAE_nbit.train raises without h_test.

Usage:  python -B tests/golden/make_golden_vae_train.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# tag, mode, n_bits, N, L, B
LOSS_CASES = [
    ("noisy_b1_n16", "noisy", 1, 16, 3, 5),
    ("genie_b1_n64", "genie", 1, 64, 16, 7),
    ("real_b1_n16", "real", 1, 16, 4, 7),
    ("real_b3_n64", "real", 3, 64, 16, 7),
    ("real_b2_n256", "real", 2, 256, 64, 5),
    ("real_inf_n64", "real", float("inf"), 64, 16, 7),
]
# tag, mode, n_bits, N, L, P, n_pilot_convs, n_layers, seed
NET_CASES = [
    ("net_noisy_n16p2", "noisy", 1, 16, 4, 2, 1, 3, 23),
    ("net_real_n64", "real", 3, 64, 16, 1, 0, 2, 22),
]
NET_B = 6
SNRS = [-10, -5, 0, 5, 10, 15, 20]


def main():
    import warnings
    import numpy as np
    import torch
    from make_golden import _import_reference
    _import_reference()
    from estimators import vae as V
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    dev = torch.device("cpu")
    out, meta = {}, {"loss_cases": {}, "net_cases": {}, "quirks": {}}

    def make_params(mode, nb, N, L, P=1, npc=0, nl=2, **kw):
        p = dict(n_antennas=N, n_pilots=P, latent_dim=L, n_layers=nl, n_pilot_convs=npc, vae_mode=mode, fft_pre=True,
                 zeromean=True, apply_batchnorm=False, n_bits=nb, quantizer_type="uniform", device=dev, filters_max=32,
                 lr=1e-3, batch_size=NET_B)
        p.update(kw)
        return p

    def rel(a, b):
        return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))

    for ci, (tag, mode, nb, N, L, B) in enumerate(LOSS_CASES):
        rng = np.random.default_rng(500 + ci)
        enc = (0.5 * rng.standard_normal((B, 2 * L))).astype(np.float32)
        dec = rng.standard_normal((B, N)).astype(np.float32)
        t = (np.sqrt(0.5) * rng.standard_normal((B, 2 * N))).astype(np.float32)
        snr = rng.choice(SNRS, B).astype(np.float64)
        model = V.DNN_VAE(make_params(mode, nb, N, L))
        res = {}
        for name, dt in (("32", torch.float32), ("64", torch.float64)):
            e = torch.tensor(enc, dtype=dt, requires_grad=True)
            d = torch.tensor(dec, dtype=dt, requires_grad=True)
            tt = torch.tensor(t, dtype=dt)
            sl = torch.tensor(snr, dtype=dt)
            model.forward = lambda x, e=e, d=d: (e[:, :L], e[:, L:], None, d)
            if mode == "real":
                loss = model.vae_loss(None, tt, mode=mode, snr_list=sl)
            else:
                loss = model.vae_loss(tt, None, mode=mode)
            loss.backward()
            res[name] = (loss.detach().numpy().copy(), e.grad.numpy().copy(), d.grad.numpy().copy())
        p = tag + "__"
        out[p + "enc"], out[p + "dec"], out[p + "t"] = enc, dec, t
        if mode == "real":
            out[p + "snr"] = snr
        for name in ("32", "64"):
            out[p + "loss" + name], out[p + "genc" + name], out[p + "gdec" + name] = res[name]
        l32, l64 = float(res["32"][0]), float(res["64"][0])
        meta["loss_cases"][tag] = dict(mode=mode, n_bits=("inf" if nb == np.inf else nb), N=N, L=L, B=B, loss=l64,
                                       e32=dict(loss=abs(l32 - l64) / abs(l64), enc=rel(res["32"][1], res["64"][1]),
                                                dec=rel(res["32"][2], res["64"][2])))
        print(tag, "loss %.6g" % l64, meta["loss_cases"][tag]["e32"])

    for ci, (tag, mode, nb, N, L, P, npc, nl, seed) in enumerate(NET_CASES):
        params = make_params(mode, nb, N, L, P, npc, nl)
        torch.manual_seed(seed)
        model = V.DNN_VAE(params)
        rng = np.random.default_rng(600 + ci)
        t = (np.sqrt(0.5) * rng.standard_normal((NET_B, 2 * N))).astype(np.float32)
        snr = rng.choice(SNRS, NET_B).astype(np.float64)
        if mode == "real":
            x = t
        else:
            x = (np.sqrt(0.5) * rng.standard_normal((NET_B, P, 2 * N))).astype(np.float32)
        p = tag + "__"
        sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
        for k, v in sd.items():
            out[p + "w__" + k] = v
        out[p + "x"], out[p + "t"] = x, t
        if mode == "real":
            out[p + "snr"] = snr
        torch.manual_seed(1000 + seed)
        out[p + "eps"] = torch.randn((NET_B, L)).numpy().copy()
        grads = {}
        for name, dt in (("32", torch.float32), ("64", torch.float64)):
            m = V.DNN_VAE(params)
            m.load_state_dict({k: torch.tensor(v) for k, v in sd.items()})
            m = m.to(dt)
            xx, tt, sl = torch.tensor(x, dtype=dt), torch.tensor(t, dtype=dt), torch.tensor(snr, dtype=dt)
            torch.manual_seed(1000 + seed)
            if mode == "real":
                loss = m.vae_loss(None, xx, mode=mode, snr_list=sl)
            else:
                loss = m.vae_loss(tt, xx, mode=mode)
            loss.backward()
            grads[name] = (float(loss), {k: v.grad.numpy().copy() for k, v in m.named_parameters()})
        out[p + "loss32"] = np.float32(grads["32"][0])
        e32 = {}
        for k in grads["32"][1]:
            out[p + "g32__" + k] = grads["32"][1][k]
            out[p + "g64__" + k] = grads["64"][1][k]
            e32[k] = rel(grads["32"][1][k], grads["64"][1][k])
            assert np.any(grads["64"][1][k] != 0), (tag, k)  # a dead pilot ReLU would leave nothing to compare
        meta["net_cases"][tag] = dict(mode=mode, n_bits=nb, N=N, L=L, P=P, n_pilot_convs=npc, n_layers=nl, B=NET_B,
                                      loss=grads["64"][0], e32_loss=abs(grads["32"][0] - grads["64"][0]) / abs(grads["64"][0]),
                                      e32=e32)
        print(tag, "loss %.6g" % grads["64"][0], "e32 max %.3g" % max(e32.values()))

    # VAE_nbit.train without h_test: the first validation pass fails
    N = 16
    params = make_params("genie", 1, N, 4, epochs=1, snr_scale=False, snrs=[0], sim_id="x", model_type="x", n_paths=1,
                         n_train=12)
    params["A"] = np.eye(N)
    rng = np.random.default_rng(700)
    h = (rng.standard_normal((12, N)) + 1j * rng.standard_normal((12, N))) * np.sqrt(0.5)
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())
    try:
        torch.manual_seed(3)
        V.VAE_nbit(params).train(h, None, [0])
        meta["quirks"]["h_test_none"] = {"type": "ok", "message": ""}
    except Exception as e:  # noqa: BLE001 - the point is to record whatever the reference raises
        meta["quirks"]["h_test_none"] = {"type": type(e).__name__, "message": str(e)}
    finally:
        os.chdir(cwd)
    print(meta["quirks"])

    np.savez_compressed(os.path.join(HERE, "vae_train.npz"), **out)
    with open(os.path.join(HERE, "vae_train_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote vae_train.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "vae_train.npz")))


if __name__ == "__main__":
    main()
