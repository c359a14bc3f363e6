"""Variable-length scoring, measured (writes profiles/varlen_eval.txt when run with --out):

(a) end to end: main.py's scoring loop (produce_evaluation_file, the --eval writer) over N seeded synthetic WAV files with lengths
    log-uniform in 1-12 s, --padding_type none against --padding_type zero on the same files and the same model (XLS-R-300M shape, seeded
    random weights, fp32 scoring path); host clock around the loop, which ends in a device synchronise.  The modes alternate, two runs
    each: the first run of a mode also loads code objects and fills the allocator.
(b) kernel: scl_attn_fwd_varlen against scl_attn_fwd_long at B = 64, H = 16, T = 201 and T = 624, klen all T and klen drawn from the
    length distribution of (a) (capped at T); the three launches alternate in one process, device events around groups of 10 launches,
    200 launches each, the whole comparison three times.

    python tools/varlen_eval_probe.py --out profiles/varlen_eval.txt
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


def lengths_log_uniform(n, seed, lo_s=1.0, hi_s=12.0, sr=16000):
    rs = np.random.RandomState(seed)
    return (np.exp(rs.uniform(np.log(lo_s), np.log(hi_s), n)) * sr).astype(np.int64)


def end_to_end(n, batch_size, say):
    import main as M
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_linear import Model
    from scl_amd.pack import EvalDataset
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="varlen_probe_")
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
        cfg = model.cfg
        say("(a) end to end: %d files, %.1f h of audio, lengths log-uniform 1-12 s (mean %.2f s), --batch_size %d, XLS-R-300M shape, fp32 scoring"
            % (n, lens.sum() / 16000 / 3600, lens.mean() / 16000, batch_size))
        frames_none = sum(cfg.conv_lens(int(v))[-1] for v in lens)
        say("    frames scored: none %d, zero %d (every clip cut / padded to 64600 samples = 201 frames)" % (frames_none, 201 * n))
        for rnd in range(2):
            for mode in ("none", "zero"):
                ds = EvalDataset(ids, root, mode, subdir="")
                out = os.path.join(root, "scores_%s_%d.txt" % (mode, rnd))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M.produce_evaluation_file(ds, model, dev, out, batch_size=batch_size)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert sum(1 for _ in open(out)) == n
                audio = lens.sum() / 16000.0 if mode == "none" else np.minimum(lens, 64600).sum() / 16000.0
                say("    run %d  --padding_type %-4s  %7.2f s  %8.1f utterances/s  %9.1f audio-seconds/s (%s)"
                    % (rnd, mode, dt, n / dt, audio / dt, "whole files" if mode == "none" else "the first 4.04 s of each file at most"))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def kernel(say):
    from scl_amd import ops
    from scl_amd.encoder import W2VConfig
    dev = torch.device("cuda:0")
    B, H, D = 64, 16, 64
    say("(b) kernel: scl_attn_fwd_varlen against scl_attn_fwd_long, B = %d, H = %d, us per launch (device events around groups of 10 launches, "
        "200 launches each, the three launches alternating; three repeats)" % (B, H))
    for T in (201, 624):
        qkv = (0.7 * torch.randn(B, T, 3, H, D, generator=torch.Generator().manual_seed(T))).to(torch.bfloat16).to(dev)
        ctx = torch.empty(B, T, H * D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, H, T, device=dev)
        rag = np.minimum([W2VConfig().conv_lens(int(v))[-1] for v in lengths_log_uniform(B, 99)], T)
        k_full = torch.full((B,), T, dtype=torch.int32, device=dev)
        k_rag = torch.tensor(rag, dtype=torch.int32, device=dev)
        blocks = lambda ks: int(sum(int(k) * ((int(k) + 63) // 64) for k in ks))      # query rows x key blocks visited
        runs = {"long": lambda: ops.attn_fwd_long(qkv, ctx, lse, B, T, H, D, D ** -0.5),
                "varlen, klen = T": lambda: ops.attn_fwd_varlen(qkv, ctx, lse, k_full, B, T, H, D, D ** -0.5),
                "varlen, ragged": lambda: ops.attn_fwd_varlen(qkv, ctx, lse, k_rag, B, T, H, D, D ** -0.5)}
        for f in runs.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        say("    T = %d; ragged klen: min %d, mean %.1f, max %d; key-block work ragged / full = %.3f"
            % (T, rag.min(), rag.mean(), rag.max(), blocks(rag) / blocks([T] * B)))
        for rep in range(3):
            evs = {k: [] for k in runs}
            for _ in range(20):
                for k, f in runs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(10):
                        f()
                    b.record()
                    evs[k].append((a, b))
            torch.cuda.synchronize()
            us = {k: np.array([a.elapsed_time(b) for a, b in v]) * 100.0 for k, v in evs.items()}      # ms per 10 launches -> us per launch
            say("      repeat %d: " % rep + "; ".join("%s %.1f (min %.1f, max %.1f)" % (k, np.median(v), v.min(), v.max()) for k, v in us.items())
                + "; varlen(T) / long %.3f, ragged / long %.3f" % (np.median(us["varlen, klen = T"]) / np.median(us["long"]),
                                                                  np.median(us["varlen, ragged"]) / np.median(us["long"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_end_to_end", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is meaningful on a CPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("variable-length scoring on %s (tools/varlen_eval_probe.py --n %d --batch_size %d)" % (torch.cuda.get_device_name(0), args.n, args.batch_size))
    kernel(say)
    if not args.skip_end_to_end:
        end_to_end(args.n, args.batch_size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
