"""The fixed-length entries (scl_btse_bio_fwd / _bwd) on FULL-LENGTH rows of the small sizes tests/test_btse_varlen_gpu.py uses, against
the float64 oracle: per row and per tensor, and for gradients summed over the two groups of six utterances of its back-end test.  The
bars of that test for the gradients are 3 x the worst values printed here (profiles/btse_varlen.txt).
    python tools/btse_small_shapes_probe.py [output file]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import test_btse_varlen_gpu as G
from test_backends_train_gpu import maxrel, rl2

dev = torch.device("cuda:0")
SIZES = (1, 2, 4, 5, 9, 63, 64, 65, 66, 70, 128, 129, 130)
GROUPS = ((70, 1, 5, 64, 65, 9), (4, 70, 63, 70, 2, 66))
B = 12
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def say(*a):
    s = " ".join(str(x) for x in a)
    print(s); out.write(s + "\n"); out.flush()
overall = {"grad": (0, ""), "zero-grad": (0, ""), "row": (0, ""), "out": (0, ""), "out-max": (0, ""), "group-grad": (0, ""), "group-zero": (0, "")}
def upd(kind, v, tag):
    if v > overall[kind][0]:
        overall[kind] = (v, tag)
for is_add in (False, True):
    for wseed in (4070, 4130):
        store = {}
        for L in SIZES:
            k = G.Bio(dev, is_add, L, B, wseed)
            bio, d_out = G._kernel_inputs(B, L, k.args["bio_out"], 100 + L)
            o, slab, _ = k.run(bio, [L] * B, d_out.to(dev), own=False)
            ref, rows = k.oracle(bio, [L] * B, d_out)
            worst = {"grad": (0, ""), "zero-grad": (0, ""), "row": (0, "")}
            upd("out", rl2(o, ref), "L%d" % L); upd("out-max", maxrel(o, ref), "L%d" % L)
            for b in range(B):
                upd("out", rl2(o[b], ref[b]), "L%d row" % L)
                got = k.split(slab[b])
                rowmax = max(rows[n][b].abs().max().item() for n in k.names)
                v = rl2(slab[b], torch.cat([rows[n][b].flatten() for n in k.names]))
                if v > worst["row"][0]: worst["row"] = (v, "row %d" % b)
                for n in k.names:
                    r, g = rows[n][b].flatten(), got[n]
                    if r.abs().max().item() < G.ZERO_REF * rowmax:
                        kind, v = "zero-grad", g.abs().max().item() / rowmax
                    else:
                        kind, v = "grad", rl2(g, r)
                    if v > worst[kind][0]: worst[kind] = (v, n.replace("bioScoring.encoder.", ""))
            for kind, (v, t) in worst.items():
                upd(kind, v, "add=%d w%d L%d %s" % (is_add, wseed, L, t))
            say("add=%d w%d L=%3d: grad %.3e (%s)  zero-grad %.3e (%s)  row %.3e" % (is_add, wseed, L, worst["grad"][0], worst["grad"][1],
                worst["zero-grad"][0], worst["zero-grad"][1], worst["row"][0]))
            store[L] = (slab, rows, k.names, k)
        for grp in GROUPS:
            for b in range(B):
                names, k = store[grp[0]][2], store[grp[0]][3]
                s32 = torch.zeros_like(store[grp[0]][0][0])
                for L in grp:
                    s32 = s32 + store[L][0][b]
                got = k.split(s32)
                refs = {n: sum(store[L][1][n][b] for L in grp) for n in names}
                gmax = max(v.abs().max().item() for v in refs.values())
                for n in names:
                    if "conv_k.bias" in n:
                        upd("group-zero", max(got[n].abs().max().item(), refs[n].abs().max().item()) / gmax, "add=%d w%d %s %s" % (is_add, wseed, grp, n))
                    else:
                        upd("group-grad", rl2(got[n], refs[n].flatten()), "add=%d w%d %s %s" % (is_add, wseed, grp, n.replace("bioScoring.encoder.", "")))
for kind, (v, t) in overall.items():
    say("OVERALL %-10s %.3e  (%s)" % (kind, v, t))
out.close()
