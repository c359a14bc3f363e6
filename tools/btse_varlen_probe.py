"""The bio transformer's own-last-token entries (scl_btse_bio_fwd_own / _bwd_own) against the fixed-length ones on full-length rows:
microseconds per forward + backward at B = 128 x 199 tokens, one process, the two variants alternating (profiles/btse_varlen.txt).
The kernel bodies are the same behind a template flag; on full-length rows the results are bit-identical (checked here too)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from scl_amd import ops
from scl_amd.btse_head import BtseHead, DEFAULT_BTSE, _plan
dev = torch.device("cuda:0")
B, Lt, ROUNDS, N = 128, 199, 7, 200
head = BtseHead(DEFAULT_BTSE).to(dev)
pl = _plan(head, B, 8, Lt, dev, own=True)
pl["bio"].copy_(torch.randint(0, 3, (B, Lt), dtype=torch.int32, generator=torch.Generator().manual_seed(0)))
pl["lens"].fill_(Lt)
pl["ds"].copy_(torch.randn(pl["ds"].shape, generator=torch.Generator().manual_seed(1)))
VARIANTS = {"fixed": (ops.btse_bio_fwd, ops.btse_bio_bwd), "own": (ops.btse_bio_fwd_own, ops.btse_bio_bwd_own)}


def step(name):
    f, b = VARIANTS[name]
    f(pl["desc"]); b(pl["desc"])


def timed(name, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        step(name)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


res = {}
for name in VARIANTS:
    for _ in range(20):
        step(name)
    torch.cuda.synchronize()
    res[name] = (pl["bvec"].clone(), pl["slab"].clone())
print("full-length rows, own against fixed: scores %s, slab %s" % tuple("bit-identical" if torch.equal(a, b) else "DIFFERENT"
                                                                       for a, b in zip(res["fixed"], res["own"])))
times = {name: [] for name in VARIANTS}
for r in range(ROUNDS):
    for name in VARIANTS:
        times[name].append(timed(name, N))
print("B %d x %d tokens, forward + backward, %d rounds of %d alternating, us per step" % (B, Lt, ROUNDS, N))
for name, ts in times.items():
    print("  %-5s  median %8.1f  min %8.1f  max %8.1f   %s" % (name, sorted(ts)[len(ts) // 2], min(ts), max(ts), " ".join("%.1f" % t for t in ts)))
