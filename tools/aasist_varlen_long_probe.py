"""Whole-utterance scoring through the AASIST plugin beyond 242 frames (SCL_AASIST_LENGTHS=long), measured (writes
profiles/aasist_varlen_long.txt when run with --out).

End to end: tools/aasist_varlen_probe.py's run - main.py's scoring loop over N seeded synthetic WAV files of 1-12 s, XLS-R-300M shape, fp32
scoring - with SCL_AASIST_LENGTHS=1 (files cut to 77,839 samples), SCL_AASIST_LENGTHS=long (nothing cut) and --padding_type zero, each with
and without SCL_SCORE_PACK=1.  One process, the variants alternating, one warm-up run per variant, then three repeats; median (min - max).

Per kernel at B = 32 and N = 171 / 500 / 999 nodes, (D, Do) = (64, 64): scl_gat_score_fwd_var (every utterance N nodes, so the work is the
fixed kernel's) against scl_gat_score_fwd, and scl_gat_softmax_agg_var against F.softmax(s / temp, -1) + hipnn.bmm; 3 warm-up launches,
then 10 timed ones between events: median (min - max).

    python tools/aasist_varlen_long_probe.py --out profiles/aasist_varlen_long.txt
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


def fmt(v):
    v = np.asarray(v, dtype=np.float64)
    return "%.1f (%.1f - %.1f)" % (np.median(v), v.min(), v.max())


def end_to_end(n, batch_size, say):
    import main as M
    from scl_amd import encoder as ENC
    from scl_amd.aasist_head import UPSTREAM_AASIST
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_aasist import Model
    from scl_amd.pack import EvalDataset
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="aasist_varlen_long_probe_")
    try:
        lens = lengths_log_uniform(n, 2024)
        rs = np.random.RandomState(7)
        ids = []
        for i, ln in enumerate(lens):
            ids.append("u%05d.wav" % i)
            with wave.open(os.path.join(root, ids[-1]), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                w.writeframes((np.clip(0.1 * rs.randn(ln), -1, 1) * 32767).astype("<i2").tobytes())
        model = Model({"contra_mode": "all", "loss_type": 1, "aasist": UPSTREAM_AASIST}, dev, w2v_cfg=W2VConfig(), seed=1)
        say("%d files, %.1f h of audio, lengths log-uniform 1-12 s (mean %.2f s), --batch_size %d, XLS-R-300M shape, AASIST back-end, fp32 scoring, "
            "PACK_ROWS %d; one warm-up run per variant, then %d repeats, the variants alternating: median (min - max)"
            % (n, lens.sum() / 16000 / 3600, lens.mean() / 16000, batch_size, ENC.PACK_ROWS, REPEATS))
        variants = [(sw, mode, pack) for sw, mode in (("1", "none"), ("long", "none"), ("1", "zero")) for pack in (False, True)]
        label = lambda v: ("--padding_type zero" if v[1] == "zero" else "none, SCL_AASIST_LENGTHS=%s" % v[0]) + (" + SCL_SCORE_PACK=1" if v[2] else "")
        times = {v: [] for v in variants}
        cut, his = {}, {}
        for rnd in range(REPEATS + 1):
            for v in variants:
                sw, mode, pack = v
                os.environ[Model.LENGTHS_SWITCH] = sw
                ENC.SCORE_PACK = pack
                ds = EvalDataset(ids, root, mode, subdir="")
                ds.min_samples, ds.max_samples = model.min_samples(), model.max_samples()
                his[v] = ds.max_samples
                out = os.path.join(root, "scores_%d_%d.txt" % (rnd, variants.index(v)))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M.produce_evaluation_file(ds, model, dev, out, batch_size=batch_size)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert sum(1 for _ in open(out)) == n
                cut[v] = ds.n_cut
                if rnd:
                    times[v].append(dt)
        ENC.SCORE_PACK = False
        for v in variants:
            audio = np.minimum(lens, his[v] if v[1] == "none" else 64600).sum() / 16000.0
            t = np.array(times[v])
            say("    %-50s %s s  %s utterances/s  %s audio-seconds/s, %d files cut"
                % (label(v), "%.2f (%.2f - %.2f)" % (np.median(t), t.min(), t.max()), fmt(n / t), fmt(audio / t), cut[v]))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def _time(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return np.median(ms), "%.3f (%.3f - %.3f) ms" % (np.median(ms), ms.min(), ms.max())


def kernels(say):
    import torch.nn.functional as F
    from scl_amd import hipnn, ops
    dev = torch.device("cuda:0")
    B, D, Do = 32, 64, 64
    say("per kernel, B = %d, (D, Do) = (%d, %d), every utterance N nodes; 3 warm-up launches, 10 timed: median (min - max)" % (B, D, Do))
    for N in (171, 500, 999):
        g = torch.Generator().manual_seed(N)
        x = torch.randn(B, N, D, generator=g).to(dev)
        W = (torch.randn(Do, D, generator=g) / 8).to(dev)
        bias = (0.1 * torch.randn(Do, generator=g)).to(dev)
        a = torch.randn(3, Do, generator=g).to(dev)
        s = torch.empty(B, N, N, device=dev)
        nodes = torch.full((B,), N, dtype=torch.int32, device=dev)
        out = torch.empty(B, N, D, device=dev)
        m_fix, t_fix = _time(lambda: ops.gat_score_fwd(x, W, bias, a, s, B, N, D, Do, N))
        m_var, t_var = _time(lambda: ops.gat_score_fwd_var(x, W, bias, a, s, nodes, nodes, B, N, D, Do))
        say("    N = %3d pair scores: scl_gat_score_fwd %s, scl_gat_score_fwd_var %s: %.3f of the time" % (N, t_fix, t_var, m_var / m_fix))
        for temp in (2.0, 100.0):
            m_ch, t_ch = _time(lambda: hipnn.bmm(F.softmax(s / temp, dim=-1), x))
            m_ag, t_ag = _time(lambda: ops.gat_softmax_agg_var(s, x, nodes, out, B, N, D, temp))
            say("    N = %3d temp %5.1f: softmax + bmm %s, scl_gat_softmax_agg_var %s: %.3f of the time" % (N, temp, t_ch, t_ag, m_ag / m_ch))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--skip_end_to_end", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is meaningful on a CPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("AASIST whole-utterance scoring beyond 242 frames on %s (tools/aasist_varlen_long_probe.py --n %d --batch_size %d)"
        % (torch.cuda.get_device_name(0), args.n, args.batch_size))
    with torch.no_grad():
        kernels(say)
    if not args.skip_end_to_end:
        end_to_end(args.n, args.batch_size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
