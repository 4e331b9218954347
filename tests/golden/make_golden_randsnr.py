"""Generate tests/golden/randsnr.npz: golden vectors for the random-SNR observation helpers
(reference utils.py:254-268 get_observation_nbit_randSNR) and the VAE encoder features built from them
(estimators/vae.py:46-53).

Runs ONLY in the build container, where the reference checkout exists at /root/reference (imported read-only, no
bytecode written).  The reference draws each row's SNR from numpy's global generator (np.random.choice) and each
row's noise from the default generator of ``crandn`` (utils.py:13).  Both are replayed, harness side:
``np.random.seed`` before the call and again before re-drawing the choices as indices, and a seeded generator put in
place of crandn's default, then a second identically seeded generator drawn row by row.  The script asserts that
the replay reproduces the reference's y and snr_list bit for bit before it stores anything.

Stored: h, snrs, and per case the pilot matrix A (or none), the probabilities p (or none), the stacked per-SNR
tables, the replayed snr_index and noise w, the reference's y and snr_list, and the float32 features computed from
y as vae.py:48-52 does (numpy fft, cplx2real, float32).  The draws use the same two seeds in every case, so w depends
only on M and snr_index only on p; both are stored once per value.

Usage:  python -B tests/golden/make_golden_randsnr.py
"""
import os
import sys

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED_CHOICE, SEED_NOISE = 10, 2024  # 10: the first seed whose 96 choices hold every SNR 12 times under both p


def main():
    if not os.path.isdir(REF):
        raise SystemExit("make_golden_randsnr.py: /root/reference is absent; the fixture is committed")
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import numpy as np
    np.infty = np.inf
    from modules import utils

    out = {}
    rng = np.random.default_rng(91)
    B, N = 96, 16
    snrs = [-10, 0, 5, 20]
    h = (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))) * np.sqrt(0.5)
    A2 = np.asarray(utils.get_pilot_matrix(N, 2, 1, "angle_amp"), complex)
    probs = {"pu": None, "pw": [.1, .2, .3, .4]}
    mats = {"I": None, "A2": A2}
    bits = {"b1": (1, "uniform"), "b2u": (2, "uniform"), "b3l": (3, "lloyd"), "inf": (np.inf, "uniform")}

    tags = []
    for ptag, p in probs.items():
        np.random.seed(SEED_CHOICE)
        idx = np.array([np.random.choice(len(snrs), p=p) if p is not None else np.random.choice(len(snrs))
                        for _ in range(B)])
        assert np.bincount(idx, minlength=len(snrs)).min() >= 12, np.bincount(idx)
        out[f"idx__{ptag}"] = idx.astype(np.int32)
        out[f"p__{ptag}"] = np.zeros(0) if p is None else np.asarray(p, float)
    for atag, A in mats.items():
        M = N if A is None else A.shape[0]
        r2 = np.random.default_rng(SEED_NOISE)
        out[f"w__{atag}"] = np.stack([utils.crandn(M, rng=r2) for _ in range(B)])  # row by row, as the reference draws
        out[f"A__{atag}"] = np.zeros((0, 0), complex) if A is None else A
    for btag, (nb, qtype) in bits.items():
        quantizer = utils.get_quantizer(snrs, nb, qtype)
        if nb not in (1, np.inf):
            out[f"thr__{btag}"] = np.stack([np.asarray(quantizer[s][0], float) for s in snrs])
            out[f"lab__{btag}"] = np.stack([np.asarray(quantizer[s][1], float) for s in snrs])
        out[f"n_bits__{btag}"] = np.float64(nb)
        for atag, A in mats.items():
            for ptag, p in probs.items():
                np.random.seed(SEED_CHOICE)
                utils.crandn.__kwdefaults__ = {"rng": np.random.default_rng(SEED_NOISE)}
                y, snr_list = utils.get_observation_nbit_randSNR(h.copy(), snrs, A, nb, quantizer, snr_scaling=p)
                idx, w = out[f"idx__{ptag}"], out[f"w__{atag}"]
                assert np.array_equal(snr_list, np.asarray(snrs, float)[idx])
                # the replay: the reference's own steps with the stored draws
                Ah = np.squeeze(np.matmul(np.eye(N) if A is None else A, np.expand_dims(h, 2)))
                for i in range(B):
                    Ah[i] += 10 ** (-snr_list[i] / 20) * w[i]
                    if nb != np.inf:
                        Ah[i] = utils.quant(Ah[i], nb, quantizer[snrs[idx[i]]][0], quantizer[snrs[idx[i]]][1])
                assert np.array_equal(Ah, y), (btag, atag, ptag)
                P = y.shape[1] // N
                r = np.reshape(y, (-1, N, P), "F")
                r = np.transpose(r, [0, 2, 1])
                r = np.fft.fft(r, axis=-1) / np.sqrt(r.shape[-1])
                feat = utils.cplx2real(r, axis=-1).astype(np.float32)
                tag = f"{btag}_{atag}_{ptag}"
                out[f"y__{tag}"] = np.asarray(y)
                out[f"snr_list__{tag}"] = np.asarray(snr_list, float)
                out[f"feat__{tag}"] = feat
                tags.append(tag)
    out["h"] = h
    out["snrs"] = np.asarray(snrs)
    out["tags"] = np.array(tags)
    path = os.path.join(HERE, "randsnr.npz")
    np.savez_compressed(path, **out)
    print("wrote randsnr.npz:", len(tags), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
