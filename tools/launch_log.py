"""Every C-ABI launch of a step in a canonical form, to compare two versions of the host code launch by launch (needs the MI355X; the
method of profiles/encoder_switch_removal.txt).  Per case a fresh model; ops._call is wrapped and every call of the FIRST step is printed
in issue order; after a SECOND step every recorded plan held in the model's states is printed, in the order they were recorded, and then
the forward and backward plans the AASIST / ResNet back-ends keep themselves (resstack._PLANS, graph._PLANS).  A call
prints as the entry-point name, every integer and float argument — each field of the descriptor and job structs passed by reference
included — and every address as the index of its first appearance in the section.  Two versions issue the same launches when their
outputs are equal (both on the same libscl_hip.so, SCL_LIB_PATH); the "# counts" lines give calls / scalar / address arguments.
Python's cyclic collector is off while a case runs: when it runs depends on how many container objects the host code has allocated, and
it decides when a temporary held in a reference cycle goes back to torch's caching allocator, that is, which later buffer aliases it.
The head-level cases (aasist-long, aasist-train-lengths: the AASIST back-end alone on zero-padded batches, which records no plan) print every
step's calls and then a SHA-256 of each output, d(feats), parameter gradient and buffer: equal digests are equal bits.

    python tools/launch_log.py [--cases small,other,resnet,aasist,aasist-long,aasist-train-lengths,btse,xlsr] > launches.txt
"""
import argparse
import ctypes
import gc
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import graph, resstack  # noqa: E402
from scl_amd import model_front as MF  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402

LINEAR = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)
LENGTHS = [20880, 400, 20560, 7777, 12000, 4000]      # tests/test_varlen_pack_gpu.py: 65, 1, 64, 24, 37 and 12 frames
RESNET_COUNTS = [17680, 18000, 25500, 33040, 41680]   # tests/test_resnet_varlen_gpu.py, in a [5, 48000] batch


class Canon:
    """Arguments -> tokens; an address is the index of its first appearance."""

    def __init__(self):
        self.addr, self.calls, self.scalars, self.addrs = {}, 0, 0, 0

    def a(self, v):
        v = v.value if isinstance(v, ctypes.c_void_p) else v
        self.addrs += 1
        return "@nil" if not v else "@%d" % self.addr.setdefault(int(v), len(self.addr))

    def n(self, v):
        self.scalars += 1
        return repr(v.value if hasattr(v, "value") else v)

    def tok(self, v, ctype=None):
        v = getattr(v, "_obj", v)      # ctypes.byref(x)
        if isinstance(v, ctypes.Structure):
            return "{%s}" % " ".join("%s=%s" % (f[0], self.tok(getattr(v, f[0]), f[1])) for f in v._fields_ if f[0] != "_pad")
        if isinstance(v, ctypes.Array):
            return "[%s]" % " ".join(self.tok(e, v._type_) for e in v)
        if ctype is ctypes.c_void_p or isinstance(v, ctypes.c_void_p) or (v is None and ctype is not None):
            return self.a(v)
        return self.n(v)

    def call(self, name, fn, args):
        types = getattr(fn, "argtypes", None) or [None] * len(args)
        self.calls += 1
        return "%s %s" % (name, " ".join(self.tok(v, t) for v, t in zip(args, types)))

    def counts(self):
        return "# counts: %d calls, %d scalar arguments, %d address arguments" % (self.calls, self.scalars, self.addrs)


def print_plan(header, plan):
    c = Canon()
    print(header)
    for fn, args, name, _ in plan:
        print(c.call(name, fn, args))
    print(c.counts())


def run(title, model, step):
    """First step under the wrapped ops._call, second step, then the plans of every state of the model and of the back-ends."""
    print("== %s: first step" % title)
    del resstack._PLANS[:], graph._PLANS[:]      # the back-ends' plans outlive a model: only this case's
    gc.collect()
    gc.disable()
    try:
        _run(title, model, step)
    finally:
        gc.enable()


def log_calls(step):
    """step() under the wrapped ops._call: every launch printed in issue order, then the counts; what step returned."""
    first, real = Canon(), ops._call

    def logged(name, *args, keep=None):
        e = real(name, *args, keep=keep)
        fn = getattr(ops.L.load(), name)
        print(first.call(name, fn, args))
        return e
    ops._call = logged
    try:
        out = step()
    finally:
        ops._call = real
    print(first.counts())
    return out


def _run(title, model, step):
    torch.manual_seed(0)
    log_calls(step)
    step()
    torch.cuda.synchronize()
    k = 0
    for store in ("_states", "_vstates_train", "_vstates"):
        for st in getattr(model, store, {}).values():
            for plan in st["plans"].values():
                print_plan("== %s: plan %d after the second step" % (title, k), plan["calls"] if isinstance(plan, dict) else plan)
                k += 1
    for mod in (resstack, graph):
        for i, pl in enumerate(mod._PLANS):
            for which in ("fwd_calls", "bwd_calls"):
                if getattr(pl, which) is not None:
                    print_plan("== %s: %s plan %d %s after the second step" % (title, mod.__name__.split(".")[-1], i, which), getattr(pl, which))


def batch(B, L, lengths=None, seed=0):
    x = 0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lengths or ()):
        x[b, n:] = 0
    return x.cuda()


def train(m, x, lengths=None, extra=()):
    def step():
        out = m(x, lengths=lengths) if lengths is not None else m(x, *extra)
        torch.autograd.backward(list(out), [torch.ones_like(o) for o in out])
    m.train()
    return step


def score(m, x, lengths=None):
    def step():
        with torch.no_grad():
            m(x, lengths=lengths) if lengths is not None else m(x)
    m.eval()
    return step


def layouts(fixed=True):
    """(name, lengths or None, pack switches on) of the three row layouts, PACK_ROWS = 64."""
    return ([("fixed", None, False)] if fixed else []) + [("padded", True, False), ("packed", True, True)]


def switches(pack, fp32):
    ENC.PACK_ROWS = 64
    ENC.VARLEN_PACK = ENC.SCORE_PACK = pack
    ML.SCORE_FP32 = MF.SCORE_FP32 = fp32


def case_small(dev):
    x = batch(len(LENGTHS), max(LENGTHS), LENGTHS)
    for p in (0.0, 0.1):
        for name, var, pack in layouts():
            switches(pack, True)
            m = ML.Model(LINEAR, dev, w2v_cfg=W2VConfig(**SMALL, dropout=p, attention_dropout=p, activation_dropout=p, dropout_input=p))
            run("linear small train %s dropout %g" % (name, p), m, train(m, x, LENGTHS if var else None))
    for fp32 in (True, False):
        for name, var, pack in layouts(fixed=fp32):
            switches(pack, fp32)
            m = ML.Model(LINEAR, dev, w2v_cfg=W2VConfig(**SMALL))
            run("linear small score %s %s" % ("fp32" if fp32 else "bf16", name), m, score(m, x, LENGTHS if var else None))


def case_other(dev):
    switches(False, True)
    m = ML.Model(LINEAR, dev, w2v_cfg=W2VConfig.tiny())
    run("linear tiny 5x9000 train (materialised scores)", m, train(m, batch(5, 9000)))
    m = ML.Model(LINEAR, dev, w2v_cfg=W2VConfig(**SMALL))
    run("linear small 4x200000 train (streaming)", m, train(m, batch(4, 200000)))
    cfg = W2VConfig(**SMALL)
    T = cfg.conv_lens(200000)[-1]
    ENC.F32_ATTN_CHUNK_BYTES, keep = 4 * cfg.heads * T * ((T + 7) // 8 * 8), ENC.F32_ATTN_CHUNK_BYTES      # one utterance per chunk
    m = ML.Model(LINEAR, dev, w2v_cfg=cfg)
    run("linear small 2x200000 score fp32 (chunked)", m, score(m, batch(2, 200000)))
    ENC.F32_ATTN_CHUNK_BYTES = keep


def case_resnet(dev):
    from scl_amd.model_resnet import Model
    from scl_amd.resnet_head import DEFAULT_RESNET
    args = dict(LINEAR, resnet=DEFAULT_RESNET)
    switches(False, True)
    m = Model(args, dev, w2v_cfg=W2VConfig.tiny())
    run("resnet tiny 4x24000 train", m, train(m, batch(4, 24000)))
    x = batch(5, 48000, RESNET_COUNTS)
    for fp32 in (True, False):
        for name, _, pack in layouts(fixed=False):
            switches(pack, fp32)
            m = Model(args, dev, w2v_cfg=W2VConfig(**SMALL))
            run("resnet small score %s %s" % ("fp32" if fp32 else "bf16", name), m, score(m, x, RESNET_COUNTS))


def case_aasist(dev):
    from scl_amd.aasist_head import UPSTREAM_AASIST
    from scl_amd.model_aasist import Model
    switches(False, True)
    m = Model({"contra_mode": "all", "loss_type": 1, "aasist": UPSTREAM_AASIST}, dev, w2v_cfg=W2VConfig.tiny())
    run("aasist tiny 4x20000 train", m, train(m, batch(4, 20000)))


def run_head(title, head, steps):
    """The back-end alone, no recorded plans: every step under the wrapped ops._call, then a SHA-256 of every tensor the step returned, of
    every parameter gradient and of every buffer of the head."""
    gc.collect()
    gc.disable()
    try:
        for i, step in enumerate(steps):
            print("== %s: step %d" % (title, i))
            out = log_calls(step)
            torch.cuda.synchronize()
            out.update({"grad " + k: p.grad for k, p in head.named_parameters() if p.grad is not None})
            out.update({"buffer " + k: v for k, v in head.named_buffers()})
            for k, v in out.items():
                print("sha256 %s %s" % (hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest(), k))
            for p in head.parameters():
                p.grad = None
    finally:
        gc.enable()


def aasist_head(dev):
    """tests/test_aasist_varlen_long_gpu.py's head: the upstream configuration filled by oracle.aasist.fill_state, seed 3."""
    from oracle.aasist import fill_state
    from scl_amd.aasist_head import AasistHead
    head = AasistHead()
    sd = fill_state({k: tuple(v.shape) for k, v in head.state_dict().items()}, seed=3)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return head.to(dev)


def case_aasist_long(dev):
    """Scoring on the count-table composition: 390 frames = 130 nodes (the first tiled pair-score size), 283 the first beyond the fused stack,
    two short rows; NaN in the padding."""
    frames, T = [390, 283, 100, 3], 400
    gen = torch.Generator().manual_seed(110)
    feats = torch.full((len(frames), T, 128), float("nan"))
    for b, n in enumerate(frames):
        feats[b, :n] = torch.randn(n, 128, generator=gen)
    feats, head = feats.to(dev), aasist_head(dev).eval()

    def step():
        with torch.no_grad():
            return dict(zip(("logits", "last_hidden"), head.forward_frames_long(feats, frames)))
    run_head("aasist-long %r padded to %d" % (frames, T), head, [step])


def case_aasist_train_lengths(dev):
    """Training on the count-table composition, dropout on: tests/aasist_train_cases.py's ragged batches (780 frames: 260 nodes, the tiled
    backward), two steps each with its inputs and cotangents."""
    from tests import aasist_train_cases as AC
    for case in sorted(AC.HEAD_RAGGED):
        frames = AC.HEAD_RAGGED[case][0]
        B, T = len(frames), max(frames)
        head = aasist_head(dev).train()
        torch.manual_seed(0)

        def step(i):
            x = AC.head_input(i, B, T)
            for b, n in enumerate(frames):
                x[b, n:] = float("nan")
            x = x.to(dev).requires_grad_(True)
            out, hid = head.forward_frames_train(x, frames)
            torch.autograd.backward([out, hid], [g.float().to(dev) for g in AC.head_cotangents(i, B)])
            return {"logits": out, "last_hidden": hid, "d(feats)": x.grad}
        run_head("aasist-train-lengths %r" % (frames,), head, [lambda i=i: step(i) for i in range(2)])


def case_btse(dev):
    import numpy as np
    from oracle import btse as OB
    from scl_amd.model_btse import Model
    switches(False, True)
    m = Model(dict(OB.default_args(), name="wav2vec2_btse"), dev, w2v_cfg=W2VConfig.tiny())
    B, Lt = 6, 23      # tests/test_btse_gpu.py: 23-token bio sequences, two of them shorter
    bio = torch.from_numpy(np.random.RandomState(3).randint(0, 3, size=(B, Lt)).astype(np.int32))
    lens = torch.tensor([Lt, Lt, 7, Lt, 1, Lt], dtype=torch.int32)
    run("btse tiny 6x8000 train", m, train(m, batch(B, 8000), extra=(bio, lens)))


def case_xlsr(dev):
    switches(False, True)
    m = ML.Model(LINEAR, dev, w2v_cfg=W2VConfig())
    run("linear xlsr 64x64000 train", m, train(m, batch(64, 64000)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="small,other,resnet,aasist,aasist-long,aasist-train-lengths,btse,xlsr")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    for name in args.cases.split(","):
        globals()["case_" + name.replace("-", "_")](torch.device("cuda:0"))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
