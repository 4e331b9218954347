"""Instruction histogram of the hot loops of one kernel in a gfx950 assembly file (hipcc -save-temps).
A loop is a backward branch; the loops with at least MIN v_mfma are reported (the component loops of the FP64
estimate kernels), each with its per-opcode counts, its non-MFMA VALU total and its s_waitcnt vmcnt lines.
python tools/loop_hist.py FILE.s KERNEL_SUBSTRING [MIN]"""
import collections
import re
import sys

path, pat = sys.argv[1], sys.argv[2]
min_mfma = int(sys.argv[3]) if len(sys.argv) > 3 else 20
lines = open(path).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"^\S+:", l) and pat in l.split(":")[0])
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
body = lines[start:end + 1]
labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\S+):", l))}
print(f"{lines[start].split(':')[0][:60]}: {len(body)} lines")
loops = {}  # head label -> last backward branch to it
for i, l in enumerate(body):
    m = re.match(r"\s+s_cbranch_\S+\s+(\.LBB\S+)", l) or re.match(r"\s+s_branch\s+(\.LBB\S+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops[m.group(1)] = i


def mfmas(a, b):
    return sum(1 for x in body[a:b + 1] if x.split() and x.split()[0].startswith("v_mfma"))


cand = {k: (labels[k], e) for k, e in loops.items() if mfmas(labels[k], e) >= min_mfma}
# innermost only: drop a loop that contains another reported one
inner = {k: v for k, v in cand.items()
         if not any(o != k and v[0] <= w[0] and w[1] <= v[1] and (w[1] - w[0]) < (v[1] - v[0]) for o, w in cand.items())}
for name, (a, i) in sorted(inner.items(), key=lambda kv: kv[1]):
    seg = [x.split(";")[0].split() for x in body[a:i + 1]]
    ops = [x[0] for x in seg if x and not x[0].endswith(":") and not x[0].startswith(".")]
    c = collections.Counter(ops)
    nm = sum(v for k, v in c.items() if k.startswith("v_mfma"))
    if nm < min_mfma:
        continue
    valu = sum(v for k, v in c.items() if k.startswith("v_") and not k.startswith("v_mfma"))
    print(f"loop {name} lines {a}..{i}: {len(ops)} instructions, {nm} MFMA, {valu} other VALU")
    print("  " + ", ".join(f"{k} {v}" for k, v in sorted(c.items(), key=lambda kv: -kv[1])))
    waits = collections.Counter(" ".join(x) for x in seg if x and x[0] == "s_waitcnt" and "vmcnt" in " ".join(x))
    print("  vmcnt waits: " + ", ".join(f"{k} x{v}" for k, v in waits.items()))
