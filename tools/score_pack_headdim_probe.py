"""The packed fp32 attention for 80- and 120-wide heads (csrc/attention_f32_wide.hip), measured: part (b) of tools/score_pack_probe.py with
the head dim as a parameter (writes profiles/score_pack_headdim.txt when run with --out).  One process, the variants alternating, one
warm-up pass per variant first (code objects, allocator), then three repeats; median (min - max) reported.

scl_attn_fwd_packed_f32 on the packed rows against the materialised chain of Encoder.forward_f32 on the padded rectangle (score GEMM,
scl_softmax_fwd_f32_varlen, P V GEMM through the S / Pm buffers, in chunks of utterances above 512 frames as the encoder cuts them),
B = 64, H = 16, D = 80 and 120: T = 201 with every frame valid, T = 201 ragged, T = 624 ragged (the lengths of tools/score_pack_probe.py).
us per layer: device events around groups of 50 layers.  rel-L2 against fp64 attention for both, over the first 8 utterances.

--alt-lib PATH: a second build of the library (build.py with SCL_BUILD_TAG and SCL_BUILD_DEFINES=-DSCL_ATTN_F32_WIDE_KB=64) whose
scl_attn_fwd_packed_f32 is timed as a third variant in the same windows — the tile variants of the kernel side by side.

    python tools/score_pack_headdim_probe.py --out profiles/score_pack_headdim.txt
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_pack_probe import GROUP, GROUPS, REPEATS, fmt  # noqa: E402
from varlen_eval_probe import lengths_log_uniform  # noqa: E402

NREF = 8      # utterances compared with fp64


def rel_l2_fp64(qkv, got_of, klen, T, H, D):
    """rel-L2 of got_of(b) [n, H * D] against fp64 attention on utterance b's own frames, pooled over the first NREF utterances."""
    E = H * D
    num = den = 0.0
    for b in range(min(NREF, len(klen))):
        n = int(klen[b])
        x = qkv[b * T * 3 * E:(b * T + n) * 3 * E].view(n, 3, H, D).double()
        q, k, v = (x[:, i].permute(1, 0, 2) for i in range(3))
        ref = (torch.softmax((q @ k.transpose(-1, -2)) * D ** -0.5, -1) @ v).permute(1, 0, 2).reshape(n, E)
        num += ((got_of(b, n).double() - ref) ** 2).sum().item()
        den += (ref ** 2).sum().item()
    return (num / den) ** 0.5


def kernel(say, D, alt):
    from scl_amd import encoder as ENC
    from scl_amd import ops
    from scl_amd.encoder import W2VConfig
    from scl_amd.ops import Op
    dev = torch.device("cuda:0")
    B, H = 64, 16
    E = H * D
    say("D = %d (E = %d): scl_attn_fwd_packed_f32 (packed rows) against the materialised chain (score GEMM, soft-max, P V GEMM; padded "
        "rows), B = %d, H = %d, us per layer: device events around groups of %d layers, %d groups per repeat, the variants alternating; "
        "one warm-up pass each, then %d repeats: median (min - max) of the groups" % (D, E, B, H, GROUP, GROUPS, REPEATS))
    rag_of = lambda T: np.minimum([W2VConfig().conv_lens(int(v))[-1] for v in lengths_log_uniform(B, 99)], T)
    for T, klen, what in ((201, np.full(B, 201), "every frame valid"), (201, rag_of(201), "ragged"), (624, rag_of(624), "ragged")):
        Tp, M = (T + 7) // 8 * 8, B * T
        slack = 128 * E
        gen = torch.Generator().manual_seed(T)
        qkv = torch.zeros(M * 3 * E + slack, device=dev)
        qkv[:M * 3 * E] = (0.7 * torch.randn(M * 3 * E, generator=gen)).to(dev)
        bc = max(1, min(B, ENC.F32_ATTN_CHUNK_BYTES // (4 * H * T * Tp))) if T > ENC.MAT_ATTN_MAX_T else B      # the encoder's chunk rule
        S, Pm = torch.empty(bc * H * T * Tp, device=dev), torch.zeros(bc * H * T * Tp + 1024, device=dev)
        ctx = torch.zeros(M * E + slack, device=dev)
        frames = torch.tensor(klen, dtype=torch.int32, device=dev)
        row0, Mq = ops.packed_rows([int(k) for k in klen], T, ENC.PACK_ROWS)
        r0 = torch.tensor(row0, dtype=torch.int32, device=dev)
        qkv_p, ctx_p = torch.zeros(Mq * 3 * E + slack, device=dev), torch.zeros(Mq * E + slack, device=dev)
        ctx_a = torch.zeros(Mq * E + slack, device=dev)
        ops.pack_rows(qkv, qkv_p, r0, B, T, 3 * E, Mq)

        def chain():
            for c0 in range(0, B, bc):
                nb, o3 = min(bc, B - c0), c0 * T * 3 * E
                ops.gemm(Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3 + E), S, T, T, D,
                         nb1=nb, nb2=H, alpha=D ** -0.5, ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp)
                ops.softmax_fwd_f32_varlen(S, Pm, frames, nb * H * T, H * T, T, Tp, Tp, klen_offset=c0)
                ops.gemm(Op(Pm, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3 + 2 * E), ctx, T, D, T,
                         b_t=True, nb1=nb, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D, c_offset=c0 * T * E)

        def alt_kernel():
            rc = alt.scl_attn_fwd_packed_f32(ctypes.c_void_p(qkv_p.data_ptr()), ctypes.c_void_p(ctx_a.data_ptr()), ctypes.c_void_p(r0.data_ptr()),
                                             B, T, H, D, Mq, ctypes.c_float(D ** -0.5), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc

        NEW = "streaming pair-form kernel"
        runs = {"materialised chain": chain, NEW: lambda: ops.attn_fwd_packed_f32(qkv_p, ctx_p, r0, B, T, H, D, Mq, D ** -0.5)}
        if alt is not None:
            runs["the kernel of --alt-lib"] = alt_kernel
        for f in runs.values():      # warm-up
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        say("    T = %d, %s: frames min %d, mean %.1f, max %d; %d valid rows of %d padded, Mq = %d; chain: %d chunk(s), S + Pm = %.0f MiB"
            % (T, what, klen.min(), klen.mean(), klen.max(), row0[-1], M, Mq, (B + bc - 1) // bc, 2 * 4.0 * bc * H * T * Tp / 2 ** 20))
        packed_rows_of = lambda buf: lambda b, n: buf[row0[b] * E:(row0[b] + n) * E].view(n, E)
        say("      rel-L2 against fp64 (first %d utterances): materialised chain %.3e, streaming pair-form kernel %.3e%s"
            % (NREF, rel_l2_fp64(qkv, lambda b, n: ctx[b * T * E:(b * T + n) * E].view(n, E), klen, T, H, D),
               rel_l2_fp64(qkv, packed_rows_of(ctx_p), klen, T, H, D),
               "" if alt is None else ", the kernel of --alt-lib %.3e" % rel_l2_fp64(qkv, packed_rows_of(ctx_a), klen, T, H, D)))
        for rep in range(REPEATS):
            evs = {k: [] for k in runs}
            for _ in range(GROUPS):
                for k, f in runs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(GROUP):
                        f()
                    b.record()
                    evs[k].append((a, b))
            torch.cuda.synchronize()
            us = {k: np.array([a.elapsed_time(b) for a, b in v]) * 1000.0 / GROUP for k, v in evs.items()}      # ms per window -> us per layer
            say("      repeat %d: " % rep + "; ".join("%s %s" % (k, fmt(v)) for k, v in us.items())
                + "; kernel / chain %.3f" % (np.median(us[NEW]) / np.median(us["materialised chain"])))
        del S, Pm, qkv, qkv_p, ctx, ctx_p, ctx_a
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head-dim", type=int, nargs="+", default=[80, 120])
    ap.add_argument("--alt-lib", default=None, help="a second libscl_hip.so whose kernel is timed beside the shipped one")
    ap.add_argument("--alt-note", default="", help="what the second build is, for the report")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is meaningful on a CPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("packed fp32 attention at head dims %s on %s (tools/score_pack_headdim_probe.py)" % (args.head_dim, torch.cuda.get_device_name(0)))
    alt = None
    if args.alt_lib:
        alt = ctypes.CDLL(os.path.abspath(args.alt_lib))
        alt.scl_attn_fwd_packed_f32.restype = ctypes.c_int
        say("--alt-lib: %s" % (args.alt_note or os.path.relpath(os.path.abspath(args.alt_lib), ROOT)))
    for D in args.head_dim:
        kernel(say, D, alt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
