"""A/B of two library builds on the bench command itself: `bench.py ARGS` run alternately with each library (QCE_LIB),
ROUNDS times each on the same GPU in one session.  One JSON line per run (ms_per_step, roofline.kernel_ms, value,
parity, mse), then one summary line with each build's median and (max - min) spread of ms_per_step and the verdict:
the second build wins only if its median is lower than the first's by more than three times the larger spread.
python tools/bench_ab.py [--rounds 5] [--out FILE.jsonl] parent:PATH/libqce_parent.so child:PATH/libqce.so -- [bench args]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    argv = sys.argv[1:]
    bargs = []
    if "--" in argv:
        i = argv.index("--")
        argv, bargs = argv[:i], argv[i + 1:]
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("variants", nargs=2)
    a = ap.parse_args(argv)
    out = open(a.out, "a") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    runs = {}
    for rnd in range(a.rounds):
        for v in a.variants:
            name, lib = v.split(":", 1)
            env = dict(os.environ, QCE_LIB=os.path.abspath(os.path.join(ROOT, lib)))
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bargs, env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:
                emit({"variant": name, "round": rnd, "error": p.stderr[-1500:]})
                return 1
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            rec = {"label": a.label, "variant": name, "round": rnd, "bench_args": " ".join(bargs),
                   "ms_per_step": r["ms_per_step"], "kernel_ms": (r.get("roofline") or {}).get("kernel_ms"),
                   "value": r["value"], "mse": r.get("mse"),
                   "parity_rel_fro": (r.get("parity") or {}).get("rel_fro")}
            runs.setdefault(name, []).append(rec)
            emit(rec)
    (n0, r0), (n1, r1) = list(runs.items())
    ms0, ms1 = np.array([x["ms_per_step"] for x in r0]), np.array([x["ms_per_step"] for x in r1])
    sp = max(ms0.max() - ms0.min(), ms1.max() - ms1.min())
    gain = float(np.median(ms0) - np.median(ms1))
    emit({"label": a.label, "summary": True, "bench_args": " ".join(bargs), "rounds": a.rounds,
          n0: {"median_ms_per_step": float(np.median(ms0)), "spread": float(ms0.max() - ms0.min())},
          n1: {"median_ms_per_step": float(np.median(ms1)), "spread": float(ms1.max() - ms1.min())},
          "gain_ms": gain, "gain_rel": gain / float(np.median(ms0)), "margin_ms": 3 * float(sp),
          "verdict": f"{n1} faster" if gain > 3 * sp else (f"{n1} slower" if -gain > sp else "no difference beyond noise")})
    return 0


if __name__ == "__main__":
    sys.exit(main())
