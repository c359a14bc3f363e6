"""Bits and launch times of the streaming attention kernels in their three row layouts (needs the MI355X), for comparing two builds of the
library: the fixed-length kernels of csrc/attention_long.hip, the padded ones of csrc/attention_varlen.hip and the packed ones of
csrc/attention_packed.hip are one body (csrc/attn_stream_body.h), so a change to it has to leave all three unchanged.

One process loads one library (SCL_LIB_PATH selects another build than the in-tree one), so two builds are compared by running this tool
in alternating fresh processes and handing their output files to --summary.

  --digest   seeded inputs through attn_fwd_long / attn_bwd_long, attn_fwd_varlen(_drop) / attn_bwd_varlen, attn_fwd_packed(_drop) /
             attn_bwd_packed and the looped fp32 soft-max (softmax_fwd_f32_long / _varlen above 512 columns) at the parameter lists of the
             kernel tests (imported from tests/); outputs prefilled with NaN; one line per output: digest <case> <tensor> <SHA-256 of its
             bytes>.  Packed outputs are digested over the launch's Mq rows (the rows the kernels promise to write).
  --time     per-launch device-event times of the forward and of the backward (delta + dK / dV + dQ), H = 16, drop_p 0 and 0.1: fixed
             length at 16 x 749 and 16 x 513 frames, padded and packed at 64 x 199 frames with the ASVspoof-like length mix of
             tools/varlen_train_probe.py; each shape warmed; one line per figure: time <case> <fwd|bwd> <median us of --iters launches>.
  --summary  no GPU: --parent FILES and --new FILES (outputs of the two modes above) -> both digest lists and whether they are equal line
             for line; per figure the per-process medians of both builds, the parent's spread (max - min of its processes: the noise of
             the box on that day) and whether the new build's median of medians stays within parent median + spread.

    python tools/attn_stream_probe.py --digest --time [--iters 200] [--out FILE]
    python tools/attn_stream_probe.py --summary --parent P1 P2 P3 --new N1 N2 N3 [--out FILE]
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAN = float("nan")
D = 64


def _params(test, names):
    """The argument list of a test's @pytest.mark.parametrize(names, [...])."""
    for m in test.pytestmark:
        if m.name == "parametrize" and m.args[0] == names:
            return list(m.args[1])
    raise KeyError(names)


def _sha(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _inputs(B, T, H, seed, dev):
    import torch
    gen = torch.Generator().manual_seed(seed)
    qkv = (0.7 * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16).to(dev)
    dctx = torch.randn(B, T, H * D, generator=gen).to(torch.bfloat16).to(dev)
    return qkv, dctx


class Family:
    """One row layout: allocates NaN-filled outputs and launches its forward / backward on them."""

    def __init__(self, layout, B, T, H, klen, drop_p, seed, dev, drop_entry=True):
        import torch
        from scl_amd import ops
        self.ops, self.layout, self.B, self.T, self.H, self.p, self.drop_entry = ops, layout, B, T, H, drop_p, drop_entry
        self.scale, self.dseed = D ** -0.5, 0x2468ACE
        E = H * D
        qkv, dctx = _inputs(B, T, H, seed, dev)
        i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device=dev)
        self.rows = B * T
        if layout == "padded":
            self.lens = i32(klen)
            for b, n in enumerate(klen):      # rows at or beyond klen[b] must never be read
                qkv[b, n:] = NAN
                dctx[b, n:] = NAN
        elif layout == "packed":
            row0, self.rows = ops.packed_rows(klen, T, 64)
            self.lens = i32(row0)
            packed = []
            for src, C in ((qkv, 3 * E), (dctx, E)):
                dst = torch.full((self.rows, C), NAN, dtype=torch.bfloat16, device=dev)
                ops.pack_rows(src.view(B, T, C), dst, self.lens, B, T, C, self.rows)
                packed.append(dst)
            qkv, dctx = packed
        self.qkv, self.dctx = qkv, dctx
        self.ctx = torch.full((self.rows, E), NAN, dtype=torch.bfloat16, device=dev)
        self.lse = torch.full((B, H, T), NAN, device=dev)
        self.dqkv = torch.full((self.rows, 3 * E), NAN, dtype=torch.bfloat16, device=dev)
        self.ws = torch.full((ops.attn_long_ws_bytes(B, T, H) // 4,), NAN, device=dev)

    def fwd(self):
        o, a = self.ops, (self.B, self.T, self.H, D)
        kw = dict(drop_p=self.p, drop_seed=self.dseed)
        if self.layout == "fixed":
            o.attn_fwd_long(self.qkv, self.ctx, self.lse, *a, self.scale, **kw)
        elif self.layout == "padded":
            if self.drop_entry:
                o.attn_fwd_varlen_drop(self.qkv, self.ctx, self.lse, self.lens, *a, self.scale, **kw)
            else:
                o.attn_fwd_varlen(self.qkv, self.ctx, self.lse, self.lens, *a, self.scale)
        elif self.p > 0:
            o.attn_fwd_packed_drop(self.qkv, self.ctx, self.lse, self.lens, *a, self.rows, self.scale, **kw)
        else:
            o.attn_fwd_packed(self.qkv, self.ctx, self.lse, self.lens, *a, self.rows, self.scale)

    def bwd(self):
        o, a = self.ops, (self.B, self.T, self.H, D)
        kw = dict(drop_p=self.p, drop_seed=self.dseed)
        if self.layout == "fixed":
            o.attn_bwd_long(self.qkv, self.ctx, self.dctx, self.lse, self.dqkv, self.ws, *a, self.scale, **kw)
        elif self.layout == "padded":
            o.attn_bwd_varlen(self.qkv, self.ctx, self.dctx, self.lse, self.lens, self.dqkv, self.ws, *a, self.scale, **kw)
        else:
            o.attn_bwd_packed(self.qkv, self.ctx, self.dctx, self.lse, self.lens, self.dqkv, self.ws, *a, self.rows, self.scale, **kw)


def digest(dev, emit):
    import torch
    from scl_amd import ops
    from tests import test_attention_packed_gpu as TP
    from tests import test_long_clip_gpu as TL
    from tests import test_varlen_gpu as TV
    from tests import test_varlen_train_gpu as TT
    drops = _params(TL.test_long_attention_kernels_against_fp64, "drop_p")
    cases = [("fixed", B, T, H, None, p, T * 7 + H, True)
             for B, T, H in _params(TL.test_long_attention_kernels_against_fp64, "B,T,H") for p in drops]
    cases += [("padded", B, T, H, klen, 0.0, T * 7 + H, False)      # the entry point without dropout
              for B, H, T, klen in _params(TV.test_varlen_attention_against_fp64_and_bitwise_against_the_fixed_length_kernel, "B,H,T,klen")]
    cases += [("padded", B, T, H, klen, p, T * 7 + H, True)
              for B, H, T, klen in _params(TT.test_varlen_attention_backward_against_fp64_with_a_key_mask, "B,H,T,klen")
              for p in _params(TT.test_varlen_attention_backward_against_fp64_with_a_key_mask, "drop_p")]
    cases += [("packed", B, T, H, klen, p, T * 13 + H, True)
              for B, H, T, klen in _params(TP.test_packed_attention_carries_the_bits_of_the_padded_kernels, "B,H,T,klen")
              for p in _params(TP.test_packed_attention_carries_the_bits_of_the_padded_kernels, "drop_p")]
    for layout, B, T, H, klen, p, seed, drop_entry in cases:
        f = Family(layout, B, T, H, klen, p, seed, dev, drop_entry)
        f.fwd()
        f.bwd()
        torch.cuda.synchronize()
        name = "%s%s_B%d_T%d_H%d_p%.1f%s" % (layout, "" if drop_entry else "_nodrop", B, T, H, p,
                                             "" if klen is None else "_klen" + "-".join(map(str, klen)))
        for tensor in ("ctx", "lse", "dqkv"):
            emit("digest %s %s %s" % (name, tensor, _sha(getattr(f, tensor))))
    # the looped fp32 soft-max: more than 512 columns
    for R, T, Tp in _params(TL.test_long_f32_softmax_rows, "R,T,Tp"):
        if Tp > 512:
            S = (4.0 * torch.randn(R, Tp, generator=torch.Generator().manual_seed(T))).to(dev)
            P = torch.full((R, Tp), NAN, device=dev)
            ops.softmax_fwd_f32_long(S, P, R, T, Tp, Tp)
            emit("digest softmax_long_R%d_T%d_Tp%d P %s" % (R, T, Tp, _sha(P)))
    for B, H, T, Tp, klen in _params(TV.test_varlen_f32_softmax_against_fp64, "B,H,T,Tp,klen"):
        if Tp > 512:
            S = (4.0 * torch.randn(B, H * T, Tp, generator=torch.Generator().manual_seed(T))).to(dev)
            P = torch.full((B, H * T, Tp), NAN, device=dev)
            ops.softmax_fwd_f32_varlen(S, P, torch.tensor(klen, dtype=torch.int32, device=dev), B * H * T, H * T, T, Tp, Tp)
            emit("digest softmax_varlen_B%d_H%d_T%d_Tp%d_klen%s P %s" % (B, H, T, Tp, "-".join(map(str, klen)), _sha(P)))


def time_launches(dev, emit, iters, warmup=20):
    import torch
    from scl_amd.encoder import W2VConfig
    from tools.varlen_train_probe import asvspoof_like_lengths
    cfg = W2VConfig()
    frames = [cfg.conv_lens(n)[-1] for n in asvspoof_like_lengths(64, 64000)]
    shapes = [("fixed", 16, 749, None), ("fixed", 16, 513, None), ("padded", 64, 199, frames), ("packed", 64, 199, frames)]
    for layout, B, T, klen in shapes:
        for p in (0.0, 0.1):
            f = Family(layout, B, T, 16, klen, p, T * 7 + 16, dev)
            f.fwd()      # the backward reads this ctx and lse
            for what, launch in (("fwd", f.fwd), ("bwd", f.bwd)):
                for _ in range(warmup):
                    launch()
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
                for e0, e1 in ev:
                    e0.record()
                    launch()
                    e1.record()
                torch.cuda.synchronize()
                us = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3
                emit("time %s_B%d_T%d_H16_p%.1f %s %.2f" % (layout, B, T, p, what, us))


def summary(parent_files, new_files, emit):
    def read(files):
        digs, tim = [], {}
        for path in files:
            dig = []
            for ln in open(path):
                w = ln.split()
                if w[:1] == ["digest"]:
                    dig.append(ln.strip())
                elif w[:1] == ["time"]:
                    tim.setdefault((w[1], w[2]), []).append(float(w[3]))
            if dig:
                digs.append(dig)
        return digs, tim
    (pds, pt), (nds, nt) = read(parent_files), read(new_files)
    ok = True
    for title, digs in (("parent", pds), ("new", nds)):
        if not digs or any(d != digs[0] for d in digs):      # no process digested, or two processes of one library disagree
            emit("digests, %s library: %s" % (title, "none" if not digs else "the processes disagree"))
            ok = False
            continue
        emit("digests, %s library (%d lines, %d process(es))" % (title, len(digs[0]), len(digs)))
        for ln in digs[0]:
            emit("  " + ln)
    same = ok and pds[0] == nds[0]
    ok &= same
    emit("digest lists equal line for line: %s" % ("yes" if same else "NO"))
    if pds and nds:
        for a, b in zip(pds[0], nds[0]):
            if a != b:
                emit("  differs: %s | %s" % (a, b))
    emit("")
    emit("per-launch device-event medians, us; one value per process; spread = max - min of the parent's processes")
    emit("%-28s %-3s  %-30s %-30s %8s %8s %7s  %s" % ("case", "", "parent", "new", "parent", "new", "spread", "new <= parent + spread"))
    if not pt or set(pt) != set(nt) or any(len(v) < 3 for v in list(pt.values()) + list(nt.values())):
        emit("timing: need the same figures from at least three processes of each library")
        return False
    for key in pt:
        a, b = pt[key], nt[key]
        ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
        within = mb <= ma + spread
        ok &= within
        emit("%-28s %-3s  %-30s %-30s %8.2f %8.2f %7.2f  %s" % (key[0], key[1], " ".join("%.2f" % v for v in a), " ".join("%.2f" % v for v in b),
                                                              ma, mb, spread, "yes" if within else "NO"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--parent", nargs="+", default=[])
    ap.add_argument("--new", nargs="+", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    if args.summary:
        ok = summary(args.parent, args.new, emit)
    elif args.digest or args.time:
        import torch
        if not torch.cuda.is_available():
            sys.exit("attn_stream_probe: needs the GPU (a CPU run measures nothing)")
        from scl_amd import lib
        dev = torch.device("cuda:0")
        emit("attn_stream_probe: library %s" % lib.LIB_PATH)
        if args.digest:
            digest(dev, emit)
        if args.time:
            time_launches(dev, emit, args.iters)
    else:
        ap.error("one of --digest, --time, --summary")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
