"""Training the AASIST plugin on zero-padded batches (SCL_AASIST_TRAIN_LENGTHS=1): step times, and per-launch times of its new kernels.

Step times: one XLS-R-300M `wav2vec2_aasist` model in train mode, batch 64 x 64000 samples (199 frames), forward + loss + backward + AdamW,
input resident in HBM; five variants alternated round by round inside one process, a warm-up each, then the median (min - max) over 5 rounds
of the mean step time of 10 steps:

  fixed_fused    model(x), the fused stack and graph kernels
  fixed_unfused  model(x) with SCL_AASIST_FUSED=0: the fixed-length per-layer composition, the like-for-like baseline
  padded_full    model(x, lengths=[64000] * 64): AasistHead.forward_frames_train with every frame valid
  padded_mix     model(x, lengths=mix): the ASVspoof-like length mix of tools/varlen_train_probe.py
  pack_mix       padded_mix with SCL_VARLEN_PACK=1: the encoder on packed rows, the back-end padded

Per-launch times of the kernels the step is built from, each beside the kernel it is the twin of (same process, same sizes), timed between
two stream events around 20 back-to-back calls (not a kernel trace: a launch gap of a few microseconds is inside every figure, on both sides):

  bn     scl_bn_fwd_cols + scl_bn_bwd_cols (every column own / the ASVspoof-like width mix) against scl_bn_fwd_masked + scl_bn_bwd_masked with
         every row valid and against the fixed-length scl_bn_fwd + scl_bn_bwd, on the stack's [64, 42, 66, 64] map (45 MB) and its [.., 32] map
  score  scl_gat_score_bwd_var against scl_gat_score_bwd at 66 / 171 / 500 nodes, every utterance full (like for like) and on a node mix
  agg    scl_gat_softmax_agg_var_bwd against the backward of torch's softmax(s / temp, -1) @ x (bmm) at 66 / 171 / 500 nodes

Method there: 3 warm-up calls, then the median (min - max) over 5 rounds of 20 calls.  Nothing is asserted.

    python tools/aasist_varlen_train_probe.py [--only steps|kernels] [--batch 64] [--tiny] [--out profiles/aasist_varlen_train.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scl_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS, CALLS = 5, 20


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(CALLS):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / CALLS * 1e3)
    return "%8.1f us (%.1f - %.1f)" % (statistics.median(ms), min(ms), max(ms))


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def width_mix(B, W):
    """The length mix of tools/varlen_train_probe.py scaled to W columns: most utterances between a third and the whole, one full."""
    g = torch.Generator().manual_seed(0)
    w = (W * (0.3 + 0.7 * torch.rand(B, generator=g))).long().clamp(1, W).tolist()
    w[0] = W
    return w


def bn_rows(B, H, W, C, act=2):
    z = lambda *s, **kw: torch.randn(*s, device=DEV, **kw)          # noqa: E731
    x, dy, y, dx = z(B, H, W, C), z(B, H, W, C), torch.empty(B, H, W, C, device=DEV), torch.empty(B, H, W, C, device=DEV)
    gamma, beta, rm, rv = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    mean, rstd, sums, dg, db = (torch.empty(n, device=DEV) for n in (C, C, 2 * C + 4, C, C))
    N = B * H * W
    part = torch.empty(max(ops.bn_masked_nslabs(B, H, W), ops.bn_nslabs(N)) * 2 * C, dtype=torch.float64, device=DEV)

    def fixed():
        ops.bn_fwd(x, N, C, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5, act, part, mean, rstd, y)
        ops.bn_bwd(dy, y, x, mean, rstd, gamma, N, C, act, True, part, sums, dg, db, dx)

    def rows():
        ops.bn_fwd_masked(x, B, H, W, C, gamma, beta, rm, rv, nbt, 0.1, 1e-5, act, vh, [H] * B, part, mean, rstd, y)
        ops.bn_bwd_masked(dy, y, x, mean, rstd, gamma, B, H, W, C, act, vh, [H] * B, part, sums, dg, db, dx)

    def cols(wd, wl):
        def run():
            ops.bn_fwd_cols(x, B, H, W, C, gamma, beta, rm, rv, nbt, 0.1, 1e-5, act, wd, wl, part, mean, rstd, y)
            ops.bn_bwd_cols(dy, y, x, mean, rstd, gamma, B, H, W, C, act, wd, wl, part, sums, dg, db, dx)
        return run

    vh = i32([H] * B)
    mix = width_mix(B, W)
    mb = B * H * W * C * 4 / 1e6
    out = ["bn  [%d, %d, %d, %d] (%.1f MB), forward + backward pair (6 launches), SELU" % (B, H, W, C, mb)]
    out.append("    fixed-length scl_bn_fwd + scl_bn_bwd            %s" % timed(fixed))
    out.append("    row-masked, every row valid                     %s" % timed(rows))
    out.append("    column-masked, every column own                 %s" % timed(cols(i32([W] * B), [W] * B)))
    out.append("    column-masked, width mix (%.0f %% of the map own)  %s" % (100.0 * sum(mix) / (B * W), timed(cols(i32(mix), mix))))
    return out


def score_rows(B, N, D=64, Do=64):
    z = lambda *s: torch.randn(*s, device=DEV)          # noqa: E731
    x, W, bias, a3, ds = z(B, N, D), z(Do, D) / D ** 0.5, 0.1 * z(Do), z(3, Do), z(B, N * N)
    dP, dx = torch.empty(B * N * N * D, device=DEV), torch.empty(B, N, D, device=DEV)
    part = torch.empty(B * ops.gat_score_nblocks(N), Do * D + 4 * Do, device=DEV)
    g = torch.Generator().manual_seed(1)
    mix = (N * (0.3 + 0.7 * torch.rand(B, generator=g))).long().clamp(1, N).tolist()
    mix[0] = N
    full, mixd = i32([N] * B), i32(mix)
    out = ["score backward  B = %d, N = %d, (D, Do) = (%d, %d), homogeneous" % (B, N, D, Do)]
    out.append("    fixed scl_gat_score_bwd                         %s" % timed(lambda: ops.gat_score_bwd(x, W, bias, a3, ds, dP, part, dx, B, N, D, Do, N)))
    out.append("    scl_gat_score_bwd_var, every utterance N nodes  %s" % timed(lambda: ops.gat_score_bwd_var(x, W, bias, a3, ds, dP, part, dx, full, full, B, N, D, Do)))
    out.append("    scl_gat_score_bwd_var, node mix (%.0f %% of N^2)   %s" % (100.0 * sum(m * m for m in mix) / (B * N * N),
                                                                          timed(lambda: ops.gat_score_bwd_var(x, W, bias, a3, ds, dP, part, dx, mixd, mixd, B, N, D, Do))))
    return out


def agg_rows(B, N, D=64, temp=2.0):
    z = lambda *s: torch.randn(*s, device=DEV)          # noqa: E731
    s, x, dout = (3.0 * z(B, N, N)).requires_grad_(True), z(B, N, D).requires_grad_(True), z(B, N, D)
    o = torch.bmm(torch.softmax(s / temp, -1), x)
    sd, xd = s.detach().view(B, N * N).contiguous(), x.detach()
    ds, dx, stats, nodes = torch.empty_like(sd), torch.empty_like(xd), torch.empty(B * N * 2, device=DEV), i32([N] * B)
    out = ["soft-max + aggregation backward  B = %d, N = %d, D = %d, temp %g" % (B, N, D, temp)]
    out.append("    torch: backward of softmax(s / temp, -1) @ x    %s" % timed(lambda: torch.autograd.grad(o, (s, x), dout, retain_graph=True)))
    out.append("    scl_gat_softmax_agg_var_bwd (2 launches)        %s" % timed(lambda: ops.gat_softmax_agg_var_bwd(sd, xd, nodes, dout, ds, dx, stats, B, N, D, temp)))
    return out


def step_rows(args):
    import time
    os.environ["SCL_AASIST_TRAIN_LENGTHS"] = "1"      # read at call time; model(x) without lengths is not affected
    from scl_amd import aasist_head as AH
    from scl_amd import encoder as ENC
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_aasist import Model
    from scl_amd.optim import FusedAdamW
    from tools.varlen_train_probe import asvspoof_like_lengths
    cfg = W2VConfig(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8,
                    latent_groups=2) if args.tiny else W2VConfig()
    model = Model({"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "aasist": AH.UPSTREAM_AASIST}, DEV, w2v_cfg=cfg, seed=0)
    model.train()
    opt = FusedAdamW(model, lr=1e-5, weight_decay=1e-4)
    conf = {"model": {"contra_mode": "all", "loss_type": 1}}
    B, L = args.batch, 64000
    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(1234))).to(DEV)
    y = torch.tensor(([1] * ((5 * B + 10) // 11) + [0] * B)[:B], device=DEV)
    mix = [max(n, model.min_samples()) for n in asvspoof_like_lengths(B, L)]
    T = cfg.conv_lens(L)[-1]
    frames = [cfg.conv_lens(n)[-1] for n in mix]
    fused0 = (AH.FUSED_STACK, AH.FUSED_GRAPH)
    variants = [("fixed_fused", None, False, True), ("fixed_unfused", None, False, False), ("padded_full", [L] * B, False, True),
                ("padded_mix", mix, False, True), ("pack_mix", mix, True, True)]

    def step(lengths, packed, fused):
        ENC.VARLEN_PACK = packed                                                     # read by the model at call time
        AH.FUSED_STACK, AH.FUSED_GRAPH = fused0 if fused else (False, False)         # what SCL_AASIST_FUSED=0 sets at import
        out, feats, hid = model(x) if lengths is None else model(x, lengths=lengths)
        total = sum(model.loss(out, feats, hid, y, conf).values())
        opt.zero_grad()
        total.backward()
        opt.step()
        return total

    for _, lengths, packed, fused in variants:
        for _ in range(3):
            step(lengths, packed, fused)
    torch.cuda.synchronize()
    ms = {v[0]: [] for v in variants}
    for _ in range(ROUNDS):
        for name, lengths, packed, fused in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                last = step(lengths, packed, fused)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / 10)
            assert torch.isfinite(last).all()
    AH.FUSED_STACK, AH.FUSED_GRAPH = fused0
    out = ["train step: %s encoder + AASIST back-end, batch %d x %d samples (%d frames), forward + loss + backward + AdamW; %d rounds of 10 steps, "
           "variants alternated; ms per step" % ("tiny" if args.tiny else "XLS-R-300M", B, L, T, ROUNDS),
           "length mix: %d..%d samples, mean %.0f (%.1f of %d frames valid on average, ratio %.3f)"
           % (min(mix), max(mix), sum(mix) / B, sum(frames) / B, T, sum(frames) / (B * T)),
           "    %-16s %9s %9s %9s   %s" % ("variant", "median", "min", "max", "utterances/s at the median")]
    for name, _, _, _ in variants:
        v = ms[name]
        med = statistics.median(v)
        out.append("    %-16s %9.2f %9.2f %9.2f   %.0f" % (name, med, min(v), max(v), B / med * 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="steps or kernels (default: both)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tiny", action="store_true", help="a two-layer encoder with 64-wide heads (plumbing check, not a measurement)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aasist_varlen_train.txt"))
    args = ap.parse_args()
    lines = ["# tools/aasist_varlen_train_probe.py on %s: median (min - max) of %d rounds of %d calls, per call" % (torch.cuda.get_device_name(0), ROUNDS, CALLS),
             "# AASIST training on zero-padded batches: step times, then its kernels beside their fixed-length / row-masked / torch twins (stream events, not a kernel trace)"]
    if args.only in ("", "steps"):
        lines += step_rows(args)
    if args.only in ("", "kernels"):
        for C in (64, 32):
            lines += bn_rows(64, 42, 66, C)
        for B, N in ((64, 66), (16, 171), (8, 500)):
            lines += score_rows(B, N)
        for B, N in ((64, 66), (64, 171), (16, 500)):
            lines += agg_rows(B, N)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
