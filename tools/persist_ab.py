"""Class-by-class A/B of two builds from their bench launch logs (`python bench.py --dump-gemm-launches FILE`, several repetitions per
side, interleaved on one GPU): mean launch duration per GEMM class and repetition, the parent's spread (max - min of its repetitions)
and whether the new mean is below the parent's by more than 3 x that spread — the bar a class has to clear to move to another kernel.

    python tools/persist_ab.py 'DIR/launches_parent_*.json' 'DIR/launches_new_*.json' [--only-variant 8]
"""
import argparse
import collections
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_classes import classify, header_flags  # noqa: E402


def per_class(path):
    d = json.load(open(path))
    acc = collections.OrderedDict()
    for row in d["launches"]:
        ms, meta = row[0], row[1:]
        e = acc.setdefault(tuple(meta[:5]), [0, 0.0, set()])
        e[0] += 1
        e[1] += ms
        e[2].add(meta[5])
    return d["profiled_steps"], acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent"), ap.add_argument("new")
    ap.add_argument("--only-variant", type=int, default=None, help="only the classes the new build ran on this kernel variant")
    a = ap.parse_args()
    H = header_flags()
    sides = []
    for pat in (a.parent, a.new):
        reps = [per_class(p) for p in sorted(glob.glob(pat))]
        assert reps, pat
        sides.append(reps)
    nstep = sides[0][0][0]
    keys = list(sides[0][0][1])
    print("# %d parent / %d new repetitions, %d profiled steps each; us = mean launch duration of the class in a repetition" % (len(sides[0]), len(sides[1]), nstep))
    print("%-8s %-34s %6s %5s %5s %5s %4s | %8s %8s %7s %7s %8s %6s" % ("layout", "epilogue", "M", "N", "K", "calls", "var", "parent", "new", "spread", "delta", "ms/step", "wins"))
    total = 0.0
    rows = []
    for k in keys:
        if any(k not in r[1] for s in sides for r in s):
            continue
        pu = [r[1][k][1] / r[1][k][0] * 1e3 for r in sides[0]]
        nu = [r[1][k][1] / r[1][k][0] * 1e3 for r in sides[1]]
        var = sorted(sides[1][0][1][k][2])
        if a.only_variant is not None and a.only_variant not in var:
            continue
        calls = sides[0][0][1][k][0] / nstep
        pm, nm, spread = sum(pu) / len(pu), sum(nu) / len(nu), max(pu) - min(pu)
        lay, epi, _ = classify(list(k) + [var[0]], H)
        rows.append(((pm - nm) * calls, "%-8s %-34s %6d %5d %5d %5.1f %4s | %8.1f %8.1f %7.1f %+7.1f %+8.3f %6s" % (
            lay.split()[0], epi, k[0], k[1], k[2], calls, ",".join(map(str, var)), pm, nm, spread, nm - pm, (nm - pm) * calls / 1e3,
            "yes" if pm - nm > 3 * spread else "no")))
        total += (nm - pm) * calls / 1e3
    for _, line in sorted(rows, key=lambda r: -abs(r[0])):
        print(line)
    print("# sum over the listed classes: %+.3f ms per step" % total)


if __name__ == "__main__":
    main()
