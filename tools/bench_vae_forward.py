"""Call time of VAE_nbit.estimate_from_y with the network in torch (fused=False: torch.fft, cat, cast, conv1d,
F.linear, then k_vae) against the network inside libqce.so (fused=True: k_vae_net, then k_vae), on the fixture
networks of tests/golden/vae.npz with seeded quantised observations.

  python tools/bench_vae_forward.py [--B 10000] [--windows 7] [--calls 50] [--warmup 5] [--only NET] [--variant V]

Device tensors in and out.  One process; per network both variants are warmed up, then timed in alternating windows
of `calls` calls each, a host clock around a window that ends in a device synchronise (every call itself ends with
the 4-byte status read of k_vae).  Reported per variant: the median and the spread of the windows' mean call time.
The two estimates are compared on the same inputs (relative Frobenius difference).  One JSON line per network.
`--only` / `--variant` / `--calls` with `--windows 1` give the short single-variant run a kernel trace wants.
Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# network in the fixture -> (case that carries its hyper-parameters, n_bits timed, SNR)
NETS = {"n64p1": ("b1_64", 1, 5.0), "n64p4": ("b3u_p4", 3, 0.0), "n256p2": ("b1_256", 1, 5.0)}


def estimator(fx, meta, net):
    from quantized_channel_estimation_amd import VAE_nbit, inputs
    tag, nb, snr = NETS[net]
    c = meta["cases"][tag]
    x = fx[tag + "__x"]
    params = dict(n_antennas=c["N"], n_pilots=c["P"], latent_dim=c["latent_dim"], n_layers=c["n_layers"],
                  n_pilot_convs=max(0, c["P"] // 2), vae_mode="noisy", fft_pre=c["fft_pre"], zeromean=True,
                  apply_batchnorm=False, n_bits=nb, quantizer_type="uniform",
                  quantizer=inputs.get_quantizer([snr], nb, "uniform"), A=np.kron(x[:, None], np.eye(c["N"])),
                  eval_rate=True, device=0)
    w = {k[len(net) + 2:]: fx[k].astype(np.float32) for k in fx.files if k.startswith(net + "__")}
    return VAE_nbit(params).load_state_dict(w), c, nb, snr


def observations(c, nb, B, seed):
    rng = np.random.default_rng(seed)
    lev = np.array([-1.0, 1.0]) / np.sqrt(2) if nb == 1 else (np.arange(2 ** nb) - (2 ** nb - 1) / 2) * 0.5
    return rng.choice(lev, (B, c["P"] * c["N"])) + 1j * rng.choice(lev, (B, c["P"] * c["N"]))


def window(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=sorted(NETS))
    ap.add_argument("--variant", choices=["unfused", "fused"])
    a = ap.parse_args()
    import torch
    from quantized_channel_estimation_amd import _lib
    if _lib.device_count() == 0:
        raise SystemExit("bench_vae_forward: no GPU visible")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "vae.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "vae_meta.json")) as fh:
        meta = json.load(fh)
    for net in ([a.only] if a.only else list(NETS)):
        est, c, nb, snr = estimator(fx, meta, net)
        y = torch.as_tensor(observations(c, nb, a.B, 7), device="cuda")
        fns = {"unfused": lambda: est.estimate_from_y(y, snr), "fused": lambda: est.estimate_from_y(y, snr, fused=True)}
        if a.variant:
            fns = {a.variant: fns[a.variant]}
        out = {}
        for name, fn in fns.items():
            for _ in range(max(1, a.warmup)):
                out[name] = fn()
        ms = {name: [] for name in fns}
        for _ in range(a.windows):  # alternating windows: both variants see the same machine
            for name, fn in fns.items():
                ms[name].append(window(fn, a.calls))
        line = dict(net=net, N=c["N"], P=c["P"], n_bits=nb, B=a.B, windows=a.windows, calls_per_window=a.calls)
        for name, v in ms.items():
            line[name + "_call_ms_median"] = round(float(np.median(v)), 4)
            line[name + "_call_ms_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
            line[name + "_est_per_s"] = round(a.B / (float(np.median(v)) * 1e-3), 1)
        if len(fns) == 2:
            line["fused_over_unfused_time"] = round(line["fused_call_ms_median"] / line["unfused_call_ms_median"], 4)
            d = out["fused"] - out["unfused"]
            line["rel_diff"] = float(torch.linalg.norm(d) / torch.linalg.norm(out["unfused"]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
