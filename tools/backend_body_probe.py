"""Bits and launch times of the back-end kernels that share one body between their fixed-length and their zero-padded form (needs the
MI355X), for comparing two builds of the library: BatchNorm statistics / backward / average of csrc/nn.hip and the element-wise, copy and
attention-pooling kernels of csrc/resstack.hip.  A change to a shared body has to leave both forms unchanged.

One process loads one library (SCL_LIB_PATH selects another build than the in-tree one), so two builds are compared by running this tool
in alternating fresh processes and handing their output files to --summary (tools/attn_stream_probe.py's, reused).

  --digest   seeded inputs through scl_bn_fwd / scl_bn_bwd (train and eval), scl_bn_eval_masked, scl_bn_fwd_masked / scl_bn_bwd_masked,
             scl_avgpool_fwd(_masked), scl_avgpool_bwd_masked, scl_rs_bn_act(_w), scl_rs_copy (both modes) / scl_rs_copy_w,
             scl_rs_attn_pool_fwd(_w) and one scl_rs_conv / scl_rs_conv_w launch, at the case lists of the kernel tests (imported from
             tests/); outputs prefilled with NaN; one line per output: digest <case> <tensor> <SHA-256 of its bytes>.
  --time     per-launch device-event times (an entry point is two or three kernels): BatchNorm forward / backward and the average at the
             ResNet back-end's largest and smallest maps at batch 32 x 199 frames, fixed and masked with the length mix of
             tools/resnet_varlen_train_probe.py; rs_bn_act, rs_copy and rs_attn_pool_fwd at the AASIST stack's 42 x 80 map, batch 32, fixed
             and with the widths of tools/aasist_varlen_probe.py's length mix; one line per figure: time <case> <what> <median us>.

    python tools/backend_body_probe.py --digest --time [--iters 200] [--out FILE]
    python tools/backend_body_probe.py --summary --parent P1 P2 P3 --new N1 N2 N3 [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from attn_stream_probe import _sha, summary  # noqa: E402

NAN = float("nan")


def _nan(dev, *shape):
    import torch
    return torch.full(shape, NAN, device=dev)


class BN:
    """One BatchNorm case on the GPU, fixed-length (valid None: x [N, C]) or masked (x [B, H, W, C]); outputs prefilled with NaN."""

    def __init__(self, inp, act, dev, valid=None, training=True, eval_masked=False):
        import torch
        from scl_amd import ops
        self.ops, self.act, self.valid, self.training, self.eval_masked = ops, act, valid, training, eval_masked
        d = lambda t: None if t is None else t.clone().to(dev)
        self.x, self.dy, self.gamma, self.beta = d(inp.x), d(inp.dy), d(inp.gamma), d(inp.beta)
        self.rm, self.rv, self.nbt = d(inp.running_mean), d(inp.running_var), d(inp.nbt)
        self.C = C = self.x.shape[-1]
        self.N = self.x.numel() // C
        if valid is None:
            nslab = ops.bn_nslabs(self.N)
        else:
            self.dims = tuple(self.x.shape[:3])
            self.counts, self.vd = tuple(valid), torch.tensor(valid, dtype=torch.int32, device=dev)
            nslab = ops.bn_masked_nslabs(*self.dims)
        self.part = torch.full((nslab * 2 * C,), NAN, dtype=torch.float64, device=dev)
        self.mean, self.rstd, self.y, self.dx = _nan(dev, C), _nan(dev, C), torch.full_like(self.x, NAN), torch.full_like(self.x, NAN)
        self.sums, self.dg, self.db = _nan(dev, 2 * C + (0 if valid is None else 1)), _nan(dev, C), _nan(dev, C)

    def fwd(self):
        o = self.ops
        if self.valid is None:
            o.bn_fwd(self.x, self.N, self.C, self.gamma, self.beta, self.rm, self.rv, self.nbt, self.training, 0.1, 1e-5, self.act, self.part,
                     self.mean, self.rstd, self.y)
        elif self.eval_masked:
            o.bn_eval_masked(self.x, *self.dims, self.C, self.gamma, self.beta, self.rm, self.rv, 1e-5, self.act, self.vd, self.mean, self.rstd, self.y)
        else:
            o.bn_fwd_masked(self.x, *self.dims, self.C, self.gamma, self.beta, self.rm, self.rv, self.nbt, 0.1, 1e-5, self.act, self.vd, self.counts,
                            self.part, self.mean, self.rstd, self.y)

    def bwd(self):
        o = self.ops
        if self.valid is None:
            o.bn_bwd(self.dy, self.y, self.x, self.mean, self.rstd, self.gamma, self.N, self.C, self.act, self.training, self.part, self.sums,
                     self.dg, self.db, self.dx)
        else:
            o.bn_bwd_masked(self.dy, self.y, self.x, self.mean, self.rstd, self.gamma, *self.dims, self.C, self.act, self.vd, self.counts, self.part,
                            self.sums, self.dg, self.db, self.dx)

    def digests(self, name, emit, backward=True):
        import torch
        self.fwd()
        if backward:
            self.bwd()
        torch.cuda.synchronize()
        for t in ("y", "mean", "rstd", "rm", "rv") + (("dx", "dg", "db", "sums") if backward else ()):
            emit("digest %s %s %s" % (name, t, _sha(getattr(self, t))))


class Stack:
    """The resstack.hip launches on a batch of WIDTHS-wide utterances in one [B, H, max width] geometry, as tests/test_aasist_varlen_gpu.py
    makes them; wt None: the fixed-length entry points."""

    def __init__(self, B, H, W, widths, dev, seed):
        import torch
        from scl_amd import ops
        from tests import test_aasist_varlen_gpu as TA
        self.ops, self.TA, self.B, self.H, self.W, self.dev = ops, TA, B, H, W, dev
        gen = torch.Generator().manual_seed(seed)
        C = self.C = 64
        self.wt = TA.i32(widths, dev)
        self.g1, self.g0 = TA._geom(B, H, W, 1, H), TA._geom(B, H, W, 0, H)
        self.stats = torch.cat([0.2 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen), 0.5 + torch.rand(C, generator=gen),
                                0.3 * torch.randn(C, generator=gen)]).to(dev)
        self.pos = torch.randn(H, C, generator=gen).to(dev)
        self.x, self.l = TA.Map(B, H, W, C, dev), TA.Map(B, H, W, C, dev)
        self.x.v[:, 1:H + 1, 1:W + 1] = torch.randn(B, H, W, C, generator=gen).to(dev)
        self.l.v[:, 1:H + 1, 1:W + 1] = (2.0 * torch.randn(B, H, W, C, generator=gen)).to(dev)
        self.dense = torch.randn(B, H, W, 1, generator=gen).to(dev)
        self.a, self.b16 = TA.Map(B, H, W, C, dev, fill=NAN), TA.Map(B, H, W, 16, dev, fill=NAN)
        self.back = _nan(dev, B * H * W, 32)
        self.eS, self.eT = _nan(dev, B, H, C), _nan(dev, B, W, C)

    def _w(self, wt):
        return () if wt is None else (wt.data_ptr(),)

    def bn_act(self, wt, act=1):
        self.ops._call("scl_rs_bn_act" + ("_w" if wt is not None else ""), self.x.ptr, self.stats.data_ptr(), self.a.ptr, self.C, act,
                       ctypes.byref(self.g1), *self._w(wt), self.TA.S())

    def copy(self, wt):
        if wt is None:
            self.ops._call("scl_rs_copy", self.dense.data_ptr(), self.b16.ptr, 1, 16, 0, ctypes.byref(self.g1), self.TA.S())
        else:
            self.ops._call("scl_rs_copy_w", self.dense.data_ptr(), self.b16.ptr, 1, 16, self.W, ctypes.byref(self.g1), wt.data_ptr(), self.TA.S())

    def copy_back(self):
        self.ops._call("scl_rs_copy", self.x.ptr, self.back.data_ptr(), self.C, 32, 1, ctypes.byref(self.g1), self.TA.S())

    def attn_pool(self, wt):
        self.ops._call("scl_rs_attn_pool_fwd" + ("_w" if wt is not None else ""), self.x.ptr, self.l.ptr, self.pos.data_ptr(), self.eS.data_ptr(),
                       self.eT.data_ptr(), self.C, ctypes.byref(self.g1), *self._w(wt), self.TA.S())

    def conv(self, wt):      # conv1's form of the tests: 32 -> 64 channels, six taps, rows 0..H
        import numpy as np
        import torch
        TA, dev, B, H, W = self.TA, self.dev, self.B, self.H, self.W
        gen = torch.Generator().manual_seed(2)
        w = (torch.randn(64, 32, 2, 3, generator=gen) / np.sqrt(6 * 32)).to(dev)
        bias = (0.1 * torch.randn(64, generator=gen)).to(dev)
        xin, ad, out = TA.Map(B, H, W, 32, dev), TA.Map(B, H, W, 64, dev), TA.Map(B, H, W, 64, dev, fill=NAN)
        xin.v[:, 1:H + 1, 1:W + 1] = torch.randn(B, H, W, 32, generator=gen).to(dev)
        ad.v[:, 0:H + 1, 1:W + 1] = torch.randn(B, H + 1, W, 64, generator=gen).to(dev)
        shifts = [kh * (W + 2) + kw - 1 for kh in (0, 1) for kw in (0, 1, 2)]
        TA._conv("", xin.ptr, TA._pack(w, 32, 64, dev), bias, ad.ptr, out.ptr, self.g0, shifts, 32, 64, wt)
        return out


def digest(dev, emit):
    import torch
    from scl_amd import ops
    from tests import masked_train_cases as MT
    from tests import nn_cases as NC
    from tests import test_aasist_varlen_gpu as TA
    for C, N in NC.BN_SHAPES:
        for act in NC.ACTS:
            BN(NC.bn_inputs(C, N, act), act, dev).digests("bn_C%d_N%d_%s" % (C, N, NC.ACT_NAMES[act]), emit)
    C, N = NC.BN_EVAL_SHAPE
    for act in NC.ACTS:
        BN(NC.bn_inputs(C, N, act, training=False), act, dev, training=False).digests("bn_eval_C%d_N%d_%s" % (C, N, NC.ACT_NAMES[act]), emit)
    for B, H, W, C, valid in MT.MASKED_BN_CASES:
        for act in NC.ACTS:
            name = "B%d_H%d_W%d_C%d_%s_valid%s" % (B, H, W, C, NC.ACT_NAMES[act], "-".join(map(str, valid)))
            inp = MT.masked_bn_inputs(B, H, W, C, valid, act)
            BN(inp, act, dev, valid, eval_masked=True).digests("bn_eval_masked_" + name, emit, backward=False)
            BN(inp, act, dev, valid).digests("bn_masked_" + name, emit)
    for B, R, C in NC.AVGPOOL_SHAPES:
        x, y = NC.avgpool_inputs(B, R, C)[0].to(dev), _nan(dev, B, C)
        ops.avgpool_fwd(x, B, R, C, y)
        emit("digest avgpool_B%d_R%d_C%d y %s" % (B, R, C, _sha(y)))
    B, H, W, C, valid = MT.MASKED_AVG_CASE
    x, dy = NC.avgpool_inputs(B, H * W, C)
    x = x.view(B, H, W, C).clone()
    for b, v in enumerate(valid):
        x[b, v:] = NAN
    x, dy, y, dx, vd = x.to(dev), dy.to(dev), _nan(dev, B, C), _nan(dev, B, H, W, C), torch.tensor(valid, dtype=torch.int32, device=dev)
    ops.avgpool_fwd_masked(x, vd, B, H, W, C, y)
    ops.avgpool_bwd_masked(dy, vd, tuple(valid), B, H, W, C, dx)
    emit("digest avgpool_masked y %s" % _sha(y))
    emit("digest avgpool_masked dx %s" % _sha(dx))
    s = Stack(len(TA.WIDTHS), TA.H, max(TA.WIDTHS), TA.WIDTHS, dev, seed=5)
    for tag, wt in (("fixed", None), ("w", s.wt)):
        for act in (1, 0):
            s.bn_act(wt, act)
            emit("digest rs_bn_act_%s_act%d a %s" % (tag, act, _sha(s.a.v)))
        s.copy(wt)
        emit("digest rs_copy_%s bordered %s" % (tag, _sha(s.b16.v)))
        s.attn_pool(wt)
        emit("digest rs_attn_pool_fwd_%s eS %s" % (tag, _sha(s.eS)))
        emit("digest rs_attn_pool_fwd_%s eT %s" % (tag, _sha(s.eT)))
        emit("digest rs_conv_%s out %s" % (tag, _sha(s.conv(wt).v)))
    s.copy_back()
    emit("digest rs_copy_to_dense dense %s" % _sha(s.back))


def time_launches(dev, emit, iters, warmup=20):
    import torch
    from collections import namedtuple
    from scl_amd import ops
    from scl_amd import resnet_head as RH
    from scl_amd.encoder import W2VConfig
    from tools.varlen_eval_probe import lengths_log_uniform
    from tools.varlen_train_probe import asvspoof_like_lengths

    def timed(name, what, launch):
        for _ in range(warmup):
            launch()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record()
            launch()
            e1.record()
        torch.cuda.synchronize()
        emit("time %s %s %.2f" % (name, what, statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3))

    cfg = W2VConfig()
    B, L = 32, 64000
    T = cfg.conv_lens(L)[-1]
    frames = [max(cfg.conv_lens(n)[-1], RH.min_frames()) for n in asvspoof_like_lengths(B, L)]      # the plugin's shortest utterance
    rows_full, rows_mix = RH.batch_rows([T] * B), RH.batch_rows(frames)
    Inp = namedtuple("Inp", "x dy gamma beta running_mean running_var nbt")
    gen = torch.Generator().manual_seed(9)
    for level, W, C in ((2, 128, 64), (6, 16, 256)):      # layer1's maps (the largest) and conv5's (the smallest)
        H = rows_full[level][0]
        inp = Inp(torch.randn(B, H, W, C, generator=gen), torch.randn(B, H, W, C, generator=gen), 0.5 + torch.rand(C, generator=gen),
                  torch.randn(C, generator=gen), torch.zeros(C), torch.ones(C), torch.tensor([0]))
        for tag, valid in (("fixed", None), ("masked", rows_mix[level])):
            bn = BN(inp, 1, dev, valid)
            name = "bn_%s_B%d_H%d_W%d_C%d" % (tag, B, H, W, C)
            timed(name, "fwd", bn.fwd)
            timed(name, "bwd", bn.bwd)
        x, y = inp.x.to(dev), _nan(dev, B, C)
        vd = torch.tensor(rows_mix[level], dtype=torch.int32, device=dev)
        timed("avgpool_fixed_B%d_R%d_C%d" % (B, H * W, C), "fwd", lambda: ops.avgpool_fwd(x, B, H * W, C, y))
        timed("avgpool_masked_B%d_H%d_W%d_C%d" % (B, H, W, C), "fwd", lambda: ops.avgpool_fwd_masked(x, vd, B, H, W, C, y))
    widths = [min(int(cfg.conv_lens(int(n))[-1]), 242) // 3 for n in lengths_log_uniform(B, 2024)]
    s = Stack(B, 42, 80, widths, dev, seed=6)
    for tag, wt in (("fixed", None), ("w", s.wt)):
        name = "rs_%s_B%d_H42_W80" % (tag, B)
        timed(name, "bn_act", lambda: s.bn_act(wt))
        timed(name, "copy", lambda: s.copy(wt))
        timed(name, "attn_pool_fwd", lambda: s.attn_pool(wt))


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
            sys.exit("backend_body_probe: needs the GPU (a CPU run measures nothing)")
        from scl_amd import lib
        dev = torch.device("cuda:0")
        emit("backend_body_probe: library %s" % lib.LIB_PATH)
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
