"""Generate tests/golden/vae.npz and vae_meta.json: golden vectors for the VAE-parameterised Bussgang estimator
(reference estimators/vae.py: DNN_VAE.forward_nosamp, convert_dec_outputs, lmmse, VAE_nbit.eval).

Runs ONLY in the build container (reference imported read-only, no bytecode written).  Per case it builds the
reference's DNN_VAE under torch.manual_seed, rounds its weights to a coarse grid of float16-representable values (they
are stored as float16 and compress well; the reference runs on exactly the stored values), multiplies the last decoder layer
by 12 (fresh weights give log-variances within +-0.2, a spectrum too flat to test anything; with the factor the
range is about +-2.5), prepares the inputs as VAE_nbit.eval does and records

  lv        float32 log-variances of forward_nosamp
  hhat      convert_dec_outputs + lmmse on those log-variances widened to float64 (the kernel's contract:
            exp() in float64)
  hhat_eval the same two calls exactly as VAE_nbit.eval makes them (float32 log-variances, so exp() in float32)
  mse       sum |hhat_eval - h|^2 / h.size, VAE_nbit.eval's MSE arithmetic (:211, :227)

and in the meta file lam_min (smallest eigenvalue of Cr over the samples, from the reference's pinv(Cr)) and e32
(relative difference of hhat_eval to the same weights run in float64), plus the quirk cases' exceptions.

Usage:  python -B tests/golden/make_golden_vae.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# tag, N, P, bits, snr, mode, fft_pre, B, n_layers, net (cases of one net share their weights)
CASES = [
    ("b1", 16, 1, 1, 5.0, "noisy", True, 37, 4, "n16p1"),
    ("b1_p2", 16, 2, 1, 20.0, "noisy", False, 37, 4, "n16p2"),
    ("b2u", 64, 1, 2, -10.0, "real", True, 37, 4, "n64p1"),
    ("inf", 64, 1, float("inf"), 10.0, "genie", True, 37, 4, "n64p1"),
    ("b3u_p4", 64, 4, 3, 0.0, "noisy", True, 37, 4, "n64p4"),
    ("b1_64", 64, 1, 1, 20.0, "noisy", True, 37, 4, "n64p1"),
    ("b2u_128", 128, 1, 2, 5.0, "noisy", True, 5, 2, "n128p1"),
    ("b1_256", 256, 2, 1, 5.0, "noisy", True, 3, 2, "n256p2"),
]
SEEDS = {"n16p1": 11, "n16p2": 12, "n64p1": 13, "n64p4": 14, "n128p1": 15, "n256p2": 16}


def main():
    import warnings
    import numpy as np
    import torch
    from make_golden import _import_reference
    R = _import_reference()
    ut = R["ut"]
    from estimators import vae as V
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    _load = torch.load
    torch.load = lambda *a, **k: _load(*a, **{**k, "weights_only": False})  # shim: the checkpoint carries params
    dev = torch.device("cpu")
    tmp = tempfile.mkdtemp()
    out, meta = {}, {"cases": {}, "quirks": {}}
    nets = {}

    def make_params(N, P, nb, snr, mode, fft_pre, nl, **kw):
        p = dict(n_antennas=N, n_pilots=P, latent_dim=max(N // 4, 1) if N < 128 else 8, n_layers=nl,
                 n_pilot_convs=max(0, P // 2), vae_mode=mode, fft_pre=fft_pre, zeromean=True, apply_batchnorm=False,
                 n_bits=nb, quantizer_type="uniform", quantizer=ut.get_quantizer([snr], nb, "uniform"),
                 A=ut.get_pilot_matrix(N, P, nb, "angle_amp"), eval_rate=False, device=dev, filters_max=32, lr=1e-3,
                 batch_size=100, file_vae="")
        p.update(kw)
        return p

    def make_net(params, net):
        torch.manual_seed(SEEDS[net])
        model = V.DNN_VAE(params)
        sd = model.state_dict()
        last = f"dec.linear{params['n_layers'] - 1}."
        for k in sd:
            w = sd[k] * 12 if k.startswith(last) else sd[k]
            grid = 2.0 ** (8 if params["n_antennas"] >= 128 else 10)  # a coarse grid compresses well
            sd[k] = (torch.round(w * grid) / grid).half().float()
        model.load_state_dict(sd)
        return model

    def prep(params, h, y):
        N, P = params["n_antennas"], params["n_pilots"]
        hf = ut.cplx2real(np.fft.fft(h, axis=1) / np.sqrt(N), axis=1)
        yf = np.transpose(np.reshape(y, (-1, N, P), "F"), [0, 2, 1])
        if params["fft_pre"]:
            yf = np.fft.fft(yf, axis=-1) / np.sqrt(N)
        yf = ut.cplx2real(yf, axis=-1)
        return torch.as_tensor(hf).float(), torch.as_tensor(yf).float()

    def run(model, params, h, y, snr, widen, dtype=torch.float32, **conv_kw):
        N = params["n_antennas"]
        hf, yf = prep(params, h, y)
        F = torch.fft.fft(torch.eye(N, dtype=torch.complex128)) / np.sqrt(N)
        A_t = torch.as_tensor(params["A"], dtype=torch.complex128)
        with torch.no_grad():
            x = (hf if params["vae_mode"] == "genie" else yf).to(dtype)
            mu, var = model.forward_nosamp(x)
            lv = var.clone()
            kw = dict(quantizer_type=params["quantizer_type"], zeromean=params["zeromean"])
            kw.update(conv_kw)
            mu_h, mu_y, Ch, Cy_inv = V.convert_dec_outputs(mu, var.double() if widen else var, F, 10 ** (-snr / 10), N,
                                                           A_t, params["n_bits"], dev, params["quantizer"][snr], **kw)
            hh = V.lmmse(torch.as_tensor(y, dtype=torch.complex128), mu_h, mu_y, Ch, Cy_inv)
        lam = 1.0 / float(torch.linalg.eigvalsh(Cy_inv).max())
        return lv.numpy(), hh.numpy(), lam

    def ref_eval(model, params, h, y, snr, h_train):
        path = os.path.join(tmp, "ck.pt")
        torch.save({"model": model.state_dict(), "params": params}, path)
        p = dict(params, file_vae=path)
        return V.VAE_nbit(p).eval(h, y, snr, h_train)

    def record(name, fn):
        try:
            res = fn()
            meta["quirks"][name] = {"type": "ok", "message": "", "value": res}
        except Exception as e:  # noqa: BLE001 - the point is to record whatever the reference raises
            meta["quirks"][name] = {"type": type(e).__name__, "message": str(e)}

    tags = []
    for ci, (tag, N, P, nb, snr, mode, fft_pre, B, nl, net) in enumerate(CASES):
        params = make_params(N, P, nb, snr, mode, fft_pre, nl)
        if net not in nets:
            nets[net] = make_net(params, net)
            for k, v in nets[net].state_dict().items():
                out[f"{net}__{k}"] = v.numpy().astype(np.float16)
        model = nets[net]
        model.params = params  # forward_nosamp reads vae_mode from the module's params
        scm = R["SCMMulti"](path_sigma=2.0, n_path=3)
        h, _ = scm.generate_channel(B, 1, N, np.random.default_rng(100 + ci))
        h = np.squeeze(h)  # complex64, stored as such; the reference casts to complex128
        rng = np.random.default_rng(200 + ci)
        A = params["A"]
        y0 = (A @ h.astype(complex).T).T
        w = (rng.standard_normal(y0.shape) + 1j * rng.standard_normal(y0.shape)) * np.sqrt(0.5)
        y = y0 + 10 ** (-snr / 20) * w
        if nb != np.inf:
            q = params["quantizer"][snr]
            y = ut.quant(y, nb, q[0], q[1])
        h128 = h.astype(complex)
        lv, hhat, lam = run(model, params, h128, y, snr, widen=True)
        lv2, hhat_eval, _ = run(model, params, h128, y, snr, widen=False)
        assert np.array_equal(lv, lv2)
        m64 = V.DNN_VAE(params).double()
        m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
        _, h64, _ = run(m64, params, h128, y, snr, widen=False, dtype=torch.float64)
        e32 = float(np.linalg.norm(hhat_eval - h64) / np.linalg.norm(h64))
        assert lam >= 0.1, (tag, lam)
        mse = float(np.sum(np.abs(hhat_eval - h128) ** 2) / h128.size)  # vae.py:211, :227
        p = tag + "__"
        out[p + "h"], out[p + "y"], out[p + "lv"] = h, y, lv
        out[p + "hhat"], out[p + "hhat_eval"] = hhat, hhat_eval
        out[p + "x"] = np.asarray(A[::N, 0], dtype=complex)
        meta["cases"][tag] = dict(N=N, P=P, n_bits=("inf" if nb == np.inf else nb), snr=snr, mode=mode,
                                  fft_pre=fft_pre, B=B, n_layers=nl, latent_dim=params["latent_dim"], net=net,
                                  lam_min=lam, e32=e32, mse=float(mse),
                                  lv_range=[float(lv.min()), float(lv.max())])
        print(tag, "lam_min %.3g e32 %.3g mse %.6g lv [%.2f, %.2f] widened-vs-eval %.3g" % (
            lam, e32, mse, lv.min(), lv.max(), np.linalg.norm(hhat - hhat_eval) / np.linalg.norm(hhat)))
        tags.append(tag)

        if tag in ("b1", "b2u"):
            scm_t, _ = scm.generate_channel(100, 1, N, np.random.default_rng(300 + ci))
            h_tr = np.squeeze(scm_t)
            out[p + "h_train"] = h_tr
            record("rate_" + tag, lambda: list(map(float, ref_eval(model, dict(params, eval_rate=True), h128, y, snr,
                                                                     h_tr.astype(complex))[:2])))
        if tag == "b1":
            record("eval_rate_false", lambda: float(ref_eval(model, params, h128, y, snr, h128)[0]))
            h51 = np.concatenate([h128, h128[:14]])
            y51 = np.concatenate([y, y[:14]])
            record("batch51", lambda: float(ref_eval(model, dict(params, eval_rate=True), h51, y51, snr, h128)[0]))
            pz = make_params(N, P, nb, snr, mode, fft_pre, nl, zeromean=False)
            mz = make_net(pz, net)
            record("zeromean_false", lambda: run(mz, pz, h128, y, snr, widen=False)[2])
            pl = make_params(N, P, 3, snr, mode, fft_pre, nl, quantizer_type="lloyd",
                             quantizer=ut.get_quantizer([snr], 3, "lloyd"))
            pl["n_bits"] = 3
            record("lloyd_3bit", lambda: run(model, pl, h128, y, snr, widen=False)[2])
            model.params = params
    out["tags"] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, "vae.npz"), **out)
    with open(os.path.join(HERE, "vae_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote vae.npz (%d bytes):" % os.path.getsize(os.path.join(HERE, "vae.npz")), tags)
    for k, v in meta["quirks"].items():
        print(k, v)


if __name__ == "__main__":
    main()
