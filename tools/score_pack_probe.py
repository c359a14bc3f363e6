"""The packed fp32 scoring path (SCL_SCORE_PACK=1), measured (writes profiles/score_pack.txt when run with --out).  One process, the
variants alternating, one warm-up run per variant first (code objects, allocator), then three repeats; median (min - max) reported.

(b) kernel: scl_attn_fwd_packed_f32 on the packed rows against the materialised chain of Encoder.forward_f32 on the padded rectangle
    (score GEMM, scl_softmax_fwd_f32_varlen, P V GEMM through the S / Pm buffers, in chunks of utterances above 512 frames as the
    encoder cuts them), B = 64, H = 16: T = 201 with every frame valid, T = 201 ragged, T = 624 ragged (lengths from
    tools/varlen_eval_probe.py's log-uniform distribution, capped at T).  us per layer: device events around groups of 50 layers.
(a) end to end: tools/varlen_eval_probe.py's run — main.py's scoring loop over N seeded synthetic WAV files of 1-12 s, XLS-R-300M
    shape, fp32 scoring — with --padding_type none and the switch off, --padding_type none and the switch on, and --padding_type zero.

    python tools/score_pack_probe.py --out profiles/score_pack.txt
"""
import argparse
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from varlen_eval_probe import lengths_log_uniform  # noqa: E402

REPEATS = 3
GROUP, GROUPS = 50, 8      # layers per timed window, windows per repeat and variant


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "%.1f (%.1f - %.1f)" % (np.median(v), v.min(), v.max())


def kernel(say):
    from scl_amd import encoder as ENC
    from scl_amd import ops
    from scl_amd.encoder import W2VConfig
    from scl_amd.ops import Op
    dev = torch.device("cuda:0")
    B, H, D = 64, 16, 64
    E = H * D
    say("(b) kernel: scl_attn_fwd_packed_f32 (packed rows) against the materialised chain (score GEMM, soft-max, P V GEMM; padded rows), "
        "B = %d, H = %d, us per layer: device events around groups of %d layers, %d groups per repeat, the two alternating; one warm-up "
        "pass each, then %d repeats: median (min - max) of the groups" % (B, H, GROUP, GROUPS, REPEATS))
    rag_of = lambda T: np.minimum([W2VConfig().conv_lens(int(v))[-1] for v in lengths_log_uniform(B, 99)], T)
    for T, klen, what in ((201, np.full(B, 201), "every frame valid"), (201, rag_of(201), "ragged"), (624, rag_of(624), "ragged")):
        Tp, M = (T + 7) // 8 * 8, B * T
        slack = 128 * E
        gen = torch.Generator().manual_seed(T)
        qkv = torch.zeros(M * 3 * E + slack, device=dev)
        qkv[:M * 3 * E] = (0.7 * torch.randn(M * 3 * E, generator=gen)).to(dev)
        bc = max(1, min(B, ENC.F32_ATTN_CHUNK_BYTES // (4 * H * T * Tp))) if T > ENC.MAT_ATTN_MAX_T else B      # the encoder's chunk rule
        S, Pm = torch.empty(bc * H * T * Tp, device=dev), torch.zeros(bc * H * T * Tp + 1024, device=dev)
        ctx = torch.empty(M * E + slack, device=dev)
        frames = torch.tensor(klen, dtype=torch.int32, device=dev)
        row0, Mq = ops.packed_rows([int(k) for k in klen], T, ENC.PACK_ROWS)
        r0 = torch.tensor(row0, dtype=torch.int32, device=dev)
        qkv_p, ctx_p = torch.zeros(Mq * 3 * E + slack, device=dev), torch.empty(Mq * E + slack, device=dev)
        ops.pack_rows(qkv, qkv_p, r0, B, T, 3 * E, Mq)

        def chain():
            for c0 in range(0, B, bc):
                nb, o3 = min(bc, B - c0), c0 * T * 3 * E
                ops.gemm(Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3 + E), S, T, T, D,
                         nb1=nb, nb2=H, alpha=D ** -0.5, ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp)
                ops.softmax_fwd_f32_varlen(S, Pm, frames, nb * H * T, H * T, T, Tp, Tp, klen_offset=c0)
                ops.gemm(Op(Pm, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=o3 + 2 * E), ctx, T, D, T,
                         b_t=True, nb1=nb, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D, c_offset=c0 * T * E)

        runs = {"materialised chain": chain,
                "streaming pair-form kernel": lambda: ops.attn_fwd_packed_f32(qkv_p, ctx_p, r0, B, T, H, D, Mq, D ** -0.5)}
        for f in runs.values():      # warm-up
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        say("    T = %d, %s: frames min %d, mean %.1f, max %d; %d valid rows of %d padded, Mq = %d; chain: %d chunk(s), S + Pm = %.0f MiB"
            % (T, what, klen.min(), klen.mean(), klen.max(), row0[-1], M, Mq, (B + bc - 1) // bc, 2 * 4.0 * bc * H * T * Tp / 2 ** 20))
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
                + "; kernel / chain %.3f" % (np.median(us["streaming pair-form kernel"]) / np.median(us["materialised chain"])))
        del S, Pm, qkv, qkv_p, ctx, ctx_p
        torch.cuda.empty_cache()


def end_to_end(n, batch_size, say):
    import main as M
    from scl_amd import encoder as ENC
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_linear import Model
    from scl_amd.pack import EvalDataset
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="score_pack_probe_")
    try:
        lens = lengths_log_uniform(n, 2024)
        rs = np.random.RandomState(7)
        ids = []
        for i, ln in enumerate(lens):
            ids.append("u%05d.wav" % i)
            with wave.open(os.path.join(root, ids[-1]), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                w.writeframes((np.clip(0.1 * rs.randn(ln), -1, 1) * 32767).astype("<i2").tobytes())
        model = Model({"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}, dev, w2v_cfg=W2VConfig(), seed=1)
        say("(a) end to end: %d files, %.1f h of audio, lengths log-uniform 1-12 s (mean %.2f s), --batch_size %d, XLS-R-300M shape, fp32 "
            "scoring, PACK_ROWS %d; one warm-up run per variant, then %d repeats, the variants alternating: median (min - max)"
            % (n, lens.sum() / 16000 / 3600, lens.mean() / 16000, batch_size, ENC.PACK_ROWS, REPEATS))
        variants = (("none, switch off", "none", False), ("none, SCL_SCORE_PACK=1", "none", True), ("zero", "zero", False))
        times = {v[0]: [] for v in variants}
        scores = {}
        for rnd in range(REPEATS + 1):
            for name, mode, pack in variants:
                ENC.SCORE_PACK = pack
                ds = EvalDataset(ids, root, mode, subdir="")
                out = os.path.join(root, "scores_%d_%d.txt" % (rnd, variants.index((name, mode, pack))))      # a fresh file per run
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M.produce_evaluation_file(ds, model, dev, out, batch_size=batch_size)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert sum(1 for _ in open(out)) == n
                if rnd == 0:      # the warm-up run: not timed, its scores kept for the comparison below
                    scores[name] = np.array([[float(v) for v in l.split()[1:]] for l in open(out)])
                    continue
                times[name].append(dt)
        ENC.SCORE_PACK = False
        for name, mode, _ in variants:
            audio = lens.sum() / 16000.0 if mode == "none" else np.minimum(lens, 64600).sum() / 16000.0
            t = np.array(times[name])
            say("    --padding_type %-24s %s s  %s utterances/s  %s audio-seconds/s (%s)"
                % (name, "%.2f (%.2f - %.2f)" % (np.median(t), t.min(), t.max()), fmt(n / t), fmt(audio / t),
                   "whole files" if mode == "none" else "the first 4.04 s of each file at most"))
        a, b = scores["none, switch off"], scores["none, SCL_SCORE_PACK=1"]
        say("    scores, switch on against switch off: largest difference %.2e of the largest score" % (np.abs(a - b).max() / np.abs(a).max()))
        say("    switch on / switch off: %.3f of the time" % (np.median(times["none, SCL_SCORE_PACK=1"]) / np.median(times["none, switch off"])))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_end_to_end", action="store_true")
    ap.add_argument("--skip_kernel", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is meaningful on a CPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("packed fp32 scoring on %s (tools/score_pack_probe.py --n %d --batch_size %d)" % (torch.cuda.get_device_name(0), args.n, args.batch_size))
    if not args.skip_kernel:
        kernel(say)
    if not args.skip_end_to_end:
        end_to_end(args.n, args.batch_size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
