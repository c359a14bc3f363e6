"""Per-layer launch times of the attention at head dims 64, 80 (XLS-R 1B) and 120 (XLS-R 2B), B = 64, H = 16 (needs the MI355X):

  201 frames   the streaming kernels (csrc/attention_long.hip for 64, csrc/attention_wide.hip for 80 / 120) against the materialised-score
               chain of encoder.py (QK^T GEMM -> soft-max -> PV GEMM and its backward, on the buffers of tests/test_attention_mat_gpu.py's MatChain) — the
               A/B behind the default: fixed-length batches of at most 512 frames with heads other than 64 wide stay on the chain, and
               SCL_ATTN_LONG=1 sends 225-512 frames to the streaming kernels
  624 frames   the streaming kernels only (the chain stops at 512 frames)

Forward = one layer's attention forward; backward = delta + dK / dV + dQ (streaming) or the five launches of the chain's backward.  No
dropout.  Every figure: the median, with min and max, over --repeats interleaved rounds (each round times every variant once, --iters
launches between two device events after a warm-up), so a drift of the box hits all variants alike.

    python tools/attn_headdim_probe.py [--dims 64 80 120] [--repeats 7] [--iters 20] [--out profiles/attn_headdim.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAN = float("nan")
B, H = 64, 16


def chain_fwd(ch):
    """MatChain.forward without its NaN fills and without dropout: encoder.py's three launches."""
    from scl_amd import ops
    from scl_amd.ops import Op
    Bn, Hn, T, D, E, Tp, qkv = ch.B, ch.H, ch.T, ch.D, ch.E, ch.Tp, ch.qkv
    ops.gemm(Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), ch.S, T, T, D,
             nb1=Bn, nb2=Hn, alpha=D ** -0.5, ldc=Tp, c_bs1=Hn * T * Tp, c_bs2=T * Tp)
    ops.softmax_fwd(ch.S, ch.P, Bn * Hn * T, T, Tp, Tp)
    ops.gemm(Op(ch.P, Tp, bs1=Hn * T * Tp, bs2=T * Tp), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E),
             ch.ctx, T, D, T, b_t=True, nb1=Bn, nb2=Hn, ldc=E, c_bs1=T * E, c_bs2=D)


def chain_bwd(ch):
    """MatChain.backward likewise: dV, dP, the soft-max backward, dQ, dK."""
    from scl_amd import ops
    from scl_amd.ops import Op
    Bn, Hn, T, D, E, Tp, qkv, dqkv, d_ctx = ch.B, ch.H, ch.T, ch.D, ch.E, ch.Tp, ch.qkv, ch.dqkv, ch.d_ctx
    bq = dict(nb1=Bn, nb2=Hn)
    ops.gemm(Op(ch.P, Tp, bs1=Hn * T * Tp, bs2=T * Tp), Op(d_ctx, E, bs1=T * E, bs2=D), dqkv, T, D, T, a_t=True, b_t=True,
             ldc=3 * E, c_bs1=T * 3 * E, c_bs2=D, c_offset=2 * E, **bq)
    ops.gemm(Op(d_ctx, E, bs1=T * E, bs2=D), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E), ch.S, T, T, D,
             ldc=Tp, c_bs1=Hn * T * Tp, c_bs2=T * Tp, **bq)
    ops.softmax_bwd(ch.P, ch.S, ch.dS, Bn * Hn * T, T, Tp, Tp)
    sc = D ** -0.5
    dS = Op(ch.dS, Tp, bs1=Hn * T * Tp, bs2=T * Tp)
    ops.gemm(dS, Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), dqkv, T, D, T, b_t=True, alpha=sc, ldc=3 * E,
             c_bs1=T * 3 * E, c_bs2=D, c_offset=0, **bq)
    ops.gemm(dS, Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=0), dqkv, T, D, T, a_t=True, b_t=True, alpha=sc, ldc=3 * E,
             c_bs1=T * 3 * E, c_bs2=D, c_offset=E, **bq)


def variants(dev, D, T, with_chain):
    """{name: launch} for one (D, T): streaming fwd / bwd and, with_chain, the materialised chain's."""
    import torch
    from scl_amd import ops
    from tests.test_attention_mat_gpu import MatChain, make_inputs
    E, scale = H * D, D ** -0.5
    qkv, dctx = (t.to(dev) for t in make_inputs(B, H, T, D, T * 7 + D))
    ctx = torch.full((B, T, E), NAN, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    dqkv = torch.full((B, T, 3, H, D), NAN, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    out = {"streaming fwd": lambda: ops.attn_fwd_long(qkv, ctx, lse, B, T, H, D, scale),
           "streaming bwd": lambda: ops.attn_bwd_long(qkv, ctx, dctx, lse, dqkv, ws, B, T, H, D, scale)}
    out["streaming fwd"]()      # the backward reads this ctx and lse
    if with_chain:
        ch = MatChain(dev, B, H, T, D)
        ch.load(qkv, dctx)
        chain_fwd(ch)      # the backward reads this P
        out["chain fwd"] = lambda: chain_fwd(ch)
        out["chain bwd"] = lambda: chain_bwd(ch)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 80, 120], help="head dims (a build without attention_wide.hip takes 64 only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("attn_headdim_probe: needs the GPU (a CPU run measures nothing)")
    from scl_amd import lib
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("attn_headdim_probe: library %s; B = %d, H = %d, no dropout; us per launch group, median (min .. max) of %d interleaved rounds x %d launches"
         % (os.path.relpath(lib.LIB_PATH, ROOT), B, H, args.repeats, args.iters))
    for T in (201, 624):
        for D in args.dims:
            v = variants(dev, D, T, T <= 512)
            times = {k: [] for k in v}
            for k, launch in v.items():      # warm-up
                for _ in range(5):
                    launch()
            torch.cuda.synchronize()
            for _ in range(args.repeats):
                for k, launch in v.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
            for k, t in times.items():
                emit("T=%-4d D=%-4d %-14s %9.1f (%9.1f .. %9.1f)" % (T, D, k, statistics.median(t), min(t), max(t)))
            if T <= 512:
                for d in ("fwd", "bwd"):
                    s, c = statistics.median(times["streaming " + d]), statistics.median(times["chain " + d])
                    emit("T=%-4d D=%-4d %s: streaming / chain = %.2f" % (T, D, d, s / c))
            del v
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
