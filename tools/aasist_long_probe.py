"""The AASIST back-end on long clips, measured (writes profiles/aasist_long.txt when run with --out).

Kernel level: the pair-score forward (scl_gat_score_fwd) and backward (scl_gat_score_bwd: the pair kernel + gat_dx_kernel) of csrc/gat.hip at
B = 64, D = Do = 64, N = 128 (the whole-graph kernels) and 171, 260, 500 (the tiled kernels), time per launch and per node pair.  The
expectation checked: the tiled kernels' time per pair at N = 171 and 260 within 1.5 x the whole-graph kernels' at N = 128 measured in the
same run (the inner loop is the same; the 1.5 covers the tile re-staging).

Step level: the wav2vec2_aasist train step (forward, loss, backward, AdamW) and eval forward (fp32 scoring) at XLS-R-300M shape on
16 x 164,240 samples (513 frames, 171 temporal nodes: the per-layer composition), and the back-end alone on the same features (forward +
backward in train mode; forward in eval mode) as its share of each.

One process; the variants alternate; one warm-up round, then ROUNDS windows per variant; median (min - max).  Times are device events
around a window of launches, or a host clock around a window that ends in a device synchronise.

    python tools/aasist_long_probe.py --out profiles/aasist_long.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
KERNEL_N = (128, 171, 260, 500)
MARGIN = 1.5


def fmt(v, scale=1.0, f="%.3f"):
    v = np.asarray(v, dtype=np.float64) * scale
    return (f + " (" + f + " - " + f + ")") % (np.median(v), v.min(), v.max())


def kernel_level(say, B, reps):
    from scl_amd import ops
    dev = torch.device("cuda:0")
    D = Do = 64
    g = torch.Generator().manual_seed(1)
    W = (torch.randn(Do, D, generator=g) / D ** 0.5).to(dev)
    bias = (0.1 * torch.randn(Do, generator=g)).to(dev)
    a3 = torch.zeros(3, Do, device=dev)
    a3[0] = torch.randn(Do, generator=g).to(dev)
    bufs = {}
    for N in KERNEL_N:
        nb = ops.gat_score_nblocks(N) * B
        bufs[N] = dict(x=torch.randn(B, N, D, generator=g).to(dev), s=torch.empty(B, N, N, device=dev), ds=torch.randn(B, N, N, generator=g).to(dev),
                       dP=torch.empty(B * N * N * D, device=dev), part=torch.empty(nb, Do * D + 4 * Do, device=dev), dx=torch.empty(B, N, D, device=dev))

    def fwd(N):
        b = bufs[N]
        ops.gat_score_fwd(b["x"], W, bias, a3, b["s"], B, N, D, Do, N)

    def bwd(N):
        b = bufs[N]
        ops.gat_score_bwd(b["x"], W, bias, a3, b["ds"], b["dP"], b["part"], b["dx"], B, N, D, Do, N)

    def window(fn, N):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(N)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps      # ms per launch

    times = {(k, N): [] for k in ("fwd", "bwd") for N in KERNEL_N}
    for rnd in range(ROUNDS + 1):
        for N in KERNEL_N:
            for k, fn in (("fwd", fwd), ("bwd", bwd)):
                t = window(fn, N)
                if rnd:
                    times[(k, N)].append(t)
    say("pair scores, B = %d, D = Do = 64, %d launches per window, %d windows per variant after one warm-up round, variants alternating: median (min - max)"
        % (B, reps, ROUNDS))
    ok = True
    for k, what in (("fwd", "forward (scl_gat_score_fwd)"), ("bwd", "backward (scl_gat_score_bwd: pair kernel + dx gather)")):
        base = np.median(times[(k, 128)]) / (B * 128 * 128)
        for N in KERNEL_N:
            t = np.array(times[(k, N)])
            per_pair = t / (B * N * N) * 1e6      # ns
            ratio = np.median(t) / (B * N * N) / base
            say("    %-56s N = %3d (%s, %4d blocks per graph)  %s ms per launch  %s ns per pair  %.2f x the N = 128 time per pair"
                % (what, N, "whole-graph" if N <= 128 else "tiled", ops.gat_score_nblocks(N), fmt(t), fmt(per_pair, f="%.4f"), ratio))
            if N in (171, 260) and ratio > MARGIN:
                ok = False
    say("    expectation (tiled kernels at N = 171 and 260 within %.1f x the whole-graph kernels' time per pair at N = 128): %s" % (MARGIN, "holds" if ok else "DOES NOT HOLD"))


def step_level(say, B, samples, steps):
    from scl_amd import model_front as MF
    from scl_amd.aasist_head import UPSTREAM_AASIST, AasistHead
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_aasist import Model
    from scl_amd.optim import FusedAdamW
    dev = torch.device("cuda:0")
    conf = {"model": {"contra_mode": "all", "loss_type": 1}}
    m = Model({"contra_mode": "all", "loss_type": 1, "aasist": UPSTREAM_AASIST}, dev, w2v_cfg=W2VConfig(), seed=1)
    opt = FusedAdamW(m, lr=1e-5, weight_decay=1e-4)
    g = torch.Generator().manual_seed(5)
    x = (0.1 * torch.randn(B, samples, generator=g)).to(dev)
    y = torch.tensor(([1] * 5 + [0] * 6) * B)[:B].to(dev)
    m.eval()
    with torch.no_grad():
        feats = m(x)[1].detach().clone()
    T = feats.shape[1]

    def train_step():
        m.train()
        out, f, hid = m(x)
        losses = m.loss(out, f, hid, y, conf)
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()

    def eval_forward():
        m.eval()
        with torch.no_grad():
            m(x)

    def head_train():
        m.train()
        f = feats.clone().requires_grad_(True)
        out, hid = AasistHead.forward(m, f)
        (out.sum() + hid.sum()).backward()

    def head_eval():
        m.eval()
        with torch.no_grad():
            AasistHead.forward(m, feats)

    variants = (("train step", train_step), ("back-end alone, train forward + backward", head_train), ("eval forward, fp32 scoring", eval_forward),
                ("back-end alone, eval forward", head_eval))
    times = {n: [] for n, _ in variants}
    for rnd in range(ROUNDS + 1):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
    opt.zero_grad()
    say("wav2vec2_aasist, XLS-R-300M shape, %d x %d samples (%d frames, %d temporal nodes; SCL_SCORE_FP32 %s), %d steps per window, %d windows per variant "
        "after one warm-up round, variants alternating, host clock around a synchronised window: median (min - max) ms"
        % (B, samples, T, T // 3, "on" if MF.SCORE_FP32 else "off", steps, ROUNDS))
    for name, _ in variants:
        say("    %-44s %s" % (name, fmt(times[name], f="%.2f")))
    say("    back-end's share: %.3f of the train step, %.3f of the eval forward (the back-end alone on the same features over the whole)"
        % (np.median(times["back-end alone, train forward + backward"]) / np.median(times["train step"]),
           np.median(times["back-end alone, eval forward"]) / np.median(times["eval forward, fp32 scoring"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64, help="graphs per pair-score launch")
    ap.add_argument("--reps", type=int, default=10, help="launches per kernel window")
    ap.add_argument("--step_batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=164240)
    ap.add_argument("--steps", type=int, default=4, help="steps per step-level window")
    ap.add_argument("--no_steps", action="store_true", help="kernel level only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is meaningful on a CPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("the AASIST back-end on long clips on %s (tools/aasist_long_probe.py --batch %d --reps %d --step_batch %d --samples %d --steps %d)"
        % (torch.cuda.get_device_name(0), args.batch, args.reps, args.step_batch, args.samples, args.steps))
    kernel_level(say, args.batch, args.reps)
    if not args.no_steps:
        step_level(say, args.step_batch, args.samples, args.steps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
