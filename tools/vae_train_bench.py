"""One VAE training step with the fused loss (vae.reparameterize + vae.elbo_loss, csrc/qce_vae_train.hip) against the
same step with the loss and the reparameterisation composed of torch operations under autograd -- the route a user of
this package had before: ``composed_loss`` below, the formulas of DESIGN.md's "VAE training" section in float32 with
ordinary broadcasting (the gain sum is one broadcast exp over the quantiser's levels).

A third variant, ``step``, is the fused training step of ``VAE_nbit.train(fused=True)`` (csrc/qce_vae_step.hip): the
batch draw stays torch's, everything else is two kernels of libqce.so on weights and Adam state the library holds, and
the host reads the losses once per window (the loop's once per epoch) instead of once per step.

Settings: N = 64, L = 16, n_layers = 4, batch 200, P = 1; 'noisy' 1 bit and 'real' 3 bit.  The first two variants share
the layers (torch.nn.functional, float32), the weights' initial values, Adam, the batch draw and the index_select of
the encoder input; they differ in what lies between and around the layers.

Timing: after a warm-up, windows of at least 0.5 s; the two variants alternate and the median of 5 windows each is
reported.  ``device_us``: HIP events around a window of steps with no host read inside (what the device needs per
step); ``step_us``: the host clock around a window of whole steps including the skip rule's read of the loss (what
``VAE_nbit.train`` pays per step).

    python tools/vae_train_bench.py --out profiles/vae_train_bench.json

Launch counts: ``--trace VARIANT --mode MODE --steps K`` runs K plain steps and nothing else, for a kernel trace of
its own, one per (mode, variant, K) with K = 10 and 30:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/MODE_VARIANT_K -- \
        python tools/vae_train_bench.py --trace VARIANT --mode MODE --steps K

``--launches DIR --out FILE`` then counts the rows of each run's ``*kernel_trace.csv`` (one row per launch) and writes
launches per step = (rows at K = 30 - rows at K = 10) / 20, which cancels start-up and data preparation (and the same
for the rows of libqce.so's own kernels, whose names begin with k_).  ``--out``
replaces the lines of the kind it measured and keeps the others, so timing and launch counts share one file.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, L, LAYERS, BATCH, N_TRAIN = 64, 16, 4, 200, 8000
SNRS = [-10, -5, 0, 5, 10, 15, 20]
MODES = {"noisy": 1, "real": 3}
VARIANTS = ("fused", "composed", "step")


_LEVELS = {}


def _level_squares(n_bits, device):
    """m_i^2 for the 2^b - 1 terms of the gain sum, m_i = i - 2^(b-1), as a (1, 2^b - 1) float32 tensor."""
    import torch
    key = (n_bits, str(device))
    if key not in _LEVELS:
        m = torch.arange(1, 2 ** n_bits, device=device, dtype=torch.float32) - 2.0 ** (n_bits - 1)
        _LEVELS[key] = (m * m)[None, :]
    return _LEVELS[key]


def composed_loss(mu, s, dec, target, mode, n_bits, snr):
    """-mean_b of the row ELBO of DESIGN.md ("VAE training", Formulas) in float32 torch operations with ordinary
    broadcasting: a = tr^2 + ti^2; 'real': c = exp(-v) + s2, cbar, g, beta, c' and sum(-log c' - a / c'); otherwise
    sum(v - exp(v) a); plus the KL part."""
    import torch
    n = dec.shape[1]
    a = target[:, :n] ** 2 + target[:, n:] ** 2
    if mode == "real":
        from quantized_channel_estimation_amd.inputs import MAX_UNIFORM_STEP
        s2 = torch.pow(10.0, -snr / 10)[:, None]
        c = torch.exp(-dec) + s2
        cbar = c.mean(dim=1, keepdim=True)
        delta = torch.sqrt((1 + s2) / 2) * MAX_UNIFORM_STEP[n_bits]
        terms = torch.exp(-(delta * delta / cbar) * _level_squares(n_bits, dec.device))
        g = delta / float(np.sqrt(np.pi)) * torch.rsqrt(cbar) * terms.sum(dim=1, keepdim=True)
        beta = (g * g).clamp(0, 1)
        cp = beta * c + (1 - beta) * cbar
        row = -(torch.log(cp) + a / cp).sum(dim=1)
    else:
        row = (dec - torch.exp(dec) * a).sum(dim=1)
    row = row + (s - 0.5 * mu * mu - 0.5 * torch.exp(2 * s)).sum(dim=1)
    return -row.mean()


class Stepper:
    """One model, its data and its optimiser; ``step(read)`` is one training step of the chosen variant."""

    def __init__(self, mode, variant, seed=0):
        import torch
        from quantized_channel_estimation_amd import inputs, scm, vae
        self.torch, self.vae, self.mode, self.variant = torch, vae, mode, variant
        nb = MODES[mode]
        self.nb = nb
        p = dict(n_antennas=N, n_pilots=1, latent_dim=L, n_layers=LAYERS, n_pilot_convs=0, vae_mode=mode, fft_pre=True,
                 zeromean=True, apply_batchnorm=False, n_bits=nb, quantizer_type="uniform",
                 quantizer=inputs.get_quantizer(SNRS, nb, "uniform"), A=None, device=0, lr=1e-3, batch_size=BATCH)
        self.est = vae.VAE_nbit(p)
        self.dev = self.est._device()
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(seed)
        self.est._init_weights(self.gen)
        self.opti = torch.optim.Adam(list(self.est._w.values()), lr=p["lr"])
        h, _ = scm.SCMMulti(path_sigma=2.0, n_path=3).generate_channel(N_TRAIN, 1, N, seed=seed + 1, out="device")
        h = h[:, 0, :].to(torch.complex128).contiguous()
        from quantized_channel_estimation_amd import observe
        self.x, t, self.snr = self.est._train_data(h, SNRS, seed, 0)
        self.t = t if t is not None else observe.encoder_features(h, N, True).reshape(-1, 2 * N)  # 'noisy': the channel
        self.snr32 = None if self.snr is None else self.snr.float()
        self.drawn = 0
        self.slot = 0  # 'step': entries of the trainer's loss record written since the last read

    def end_window(self, read):
        """'step': the one host read of a window of steps (the losses and skip flags of the steps since the last)."""
        if self.variant == "step":
            if read and self.slot:
                self.est._fused_read(min(self.slot, self.vae.FUSED_STEP_SLOTS))
            self.slot = 0

    def step(self, read):
        torch, est = self.torch, self.est
        if self.variant == "step":
            idx = torch.randperm(N_TRAIN, generator=self.gen, device=self.dev)[:BATCH].to(torch.int32)
            est._fused_step(self.x, self.t, snr_db=self.snr, index=idx, seed=0, row_offset=self.drawn,
                            slot=self.slot % self.vae.FUSED_STEP_SLOTS, max_batch=BATCH)
            self.drawn += BATCH
            self.slot += 1
            return
        self.opti.zero_grad()
        idx = torch.randperm(N_TRAIN, generator=self.gen, device=self.dev)[:BATCH]
        xb = self.x.index_select(0, idx)
        if self.variant == "fused":
            enc, dec = est.forward(xb, seed=0, row_offset=self.drawn)
            self.drawn += BATCH
            loss = self.vae.elbo_loss(enc, dec, self.t, mode=self.mode, n_bits=self.nb, snr_db=self.snr,
                                      index=idx.to(torch.int32))
        else:
            enc = est._encode(xb, sums=True)
            mu, s = enc[:, :L], enc[:, L:]
            z = mu + torch.exp(s) * torch.randn(mu.shape, device=self.dev, generator=self.gen)
            dec = est._decode(z)
            snr = None if self.snr32 is None else self.snr32.index_select(0, idx)
            loss = composed_loss(mu, s, dec, self.t.index_select(0, idx), self.mode, self.nb, snr)
        if read:
            val = float(loss.detach())
            if np.isnan(val) or val > 1000:
                return
        loss.backward()
        self.opti.step()


def window(st, n, read):
    """Per-step microseconds of n steps: HIP events without the host read, the host clock with it."""
    torch = st.torch
    torch.cuda.synchronize()
    if read:
        t0 = time.perf_counter()
        for _ in range(n):
            st.step(True)
        st.end_window(True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        st.step(False)
    e1.record()
    torch.cuda.synchronize()
    st.end_window(False)
    return e0.elapsed_time(e1) * 1e3 / n


def write_lines(path, kind, lines):
    """Replace the lines of ``kind`` in the JSON-lines file ``path`` and keep every other line."""
    keep = []
    if os.path.exists(path):
        with open(path) as fh:
            keep = [json.loads(t) for t in fh if t.strip()]
    keep = [k for k in keep if k.get("bench") != kind]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        for line in keep + lines:
            fh.write(json.dumps(line) + "\n")


def count_launches(root, ks=(10, 30)):
    """Launches per step from the kernel traces under root/MODE_VARIANT_K (see the module docstring)."""
    import csv
    import glob
    import re
    out = []
    for mode in MODES:
        for v in VARIANTS:
            n, lib = {}, {}
            if not any(os.path.isdir(os.path.join(root, f"{mode}_{v}_{k}")) for k in ks):
                continue  # a variant that was not traced
            for k in ks:
                f = glob.glob(os.path.join(root, f"{mode}_{v}_{k}", "**", "*kernel_trace.csv"), recursive=True)
                if len(f) != 1:
                    raise SystemExit(f"expected one kernel trace under {root}/{mode}_{v}_{k}, found {len(f)}")
                with open(f[0]) as fh:
                    names = [r.get("Kernel_Name", "") for r in csv.DictReader(fh)]
                n[k] = len(names)
                lib[k] = sum(1 for name in names if re.search(r"\bk_[a-z0-9_]+", name))  # libqce.so's kernels: k_*
            out.append(dict(bench="vae_train_launches", mode=mode, variant=v, N=N, L=L, n_layers=LAYERS, batch=BATCH,
                            **{f"launches_{k}_steps": n[k] for k in ks},
                            launches_per_step=(n[ks[1]] - n[ks[0]]) / (ks[1] - ks[0]),
                            library_launches_per_step=(lib[ks[1]] - lib[ks[0]]) / (ks[1] - ks[0])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", choices=VARIANTS, default=None)
    ap.add_argument("--mode", choices=tuple(MODES), default="noisy")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", default=None, help="directory of kernel-trace runs MODE_VARIANT_K to count")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.5)
    a = ap.parse_args()
    if a.launches:
        lines = count_launches(a.launches)
        for line in lines:
            print(json.dumps(line), flush=True)
        if a.out:
            write_lines(a.out, "vae_train_launches", lines)
        return
    import torch
    if a.trace:
        st = Stepper(a.mode, a.trace)
        for _ in range(a.steps):
            st.step(False)
        st.end_window(False)
        torch.cuda.synchronize()
        return
    lines = []
    for mode in MODES:
        sts = {v: Stepper(mode, v) for v in VARIANTS}
        n = {}
        for v, st in sts.items():
            for _ in range(30):
                st.step(True)
            st.end_window(True)
            n[v] = max(10, int(np.ceil(a.window_seconds * 1e6 / window(st, 50, True))))
        res = {v: {"device_us": [], "step_us": []} for v in sts}
        for _ in range(a.windows):
            for v, st in sts.items():  # the variants alternate
                res[v]["device_us"].append(window(st, n[v], False))
                res[v]["step_us"].append(window(st, n[v], True))
        for v in sts:
            line = dict(bench="vae_train_step", device=torch.cuda.get_device_name(0), mode=mode, n_bits=MODES[mode],
                        variant=v, N=N, L=L, n_layers=LAYERS, batch=BATCH, steps_per_window=n[v], windows=a.windows,
                        device_us=statistics.median(res[v]["device_us"]), step_us=statistics.median(res[v]["step_us"]),
                        device_us_windows=res[v]["device_us"], step_us_windows=res[v]["step_us"])
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        write_lines(a.out, "vae_train_step", lines)


if __name__ == "__main__":
    main()
