"""Whole-utterance scoring through the AASIST plugin (wav2vec2_aasist, forward(x, lengths) behind SCL_AASIST_LENGTHS=1), measured end to end
(writes profiles/aasist_varlen.txt when run with --out).  tools/varlen_eval_probe.py's run — main.py's scoring loop over N seeded synthetic
WAV files of 1-12 s, XLS-R-300M shape, fp32 scoring — with --padding_type none and the switch on, the same with SCL_SCORE_PACK=1 on top,
and --padding_type zero (every file cut / padded to 64600 samples).  One process, the variants alternating, one warm-up run per variant
first (code objects, allocator, per-shape buffer sets and plans), then three repeats; median (min - max) reported.  Files longer than the
back-end's max_samples() (77,839: 242 frames, 80 temporal nodes) are cut to it by the data path, as main.py does, and counted.

    python tools/aasist_varlen_probe.py --out profiles/aasist_varlen.txt
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
    root = tempfile.mkdtemp(prefix="aasist_varlen_probe_")
    os.environ[Model.LENGTHS_SWITCH] = "1"
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
        lo, hi = model.min_samples(), model.max_samples()
        say("%d files, %.1f h of audio, lengths log-uniform 1-12 s (mean %.2f s; %d beyond the back-end's %d samples and cut to it, %d below its %d), "
            "--batch_size %d, XLS-R-300M shape, AASIST back-end, fp32 scoring, PACK_ROWS %d; one warm-up run per variant, then %d repeats, "
            "the variants alternating: median (min - max)"
            % (n, lens.sum() / 16000 / 3600, lens.mean() / 16000, int((lens > hi).sum()), hi, int((lens < lo).sum()), lo, batch_size, ENC.PACK_ROWS, REPEATS))
        variants = (("none, SCL_AASIST_LENGTHS=1", "none", False), ("none, + SCL_SCORE_PACK=1", "none", True), ("zero", "zero", False))
        times = {v[0]: [] for v in variants}
        scores, cut = {}, {}
        for rnd in range(REPEATS + 1):
            for name, mode, pack in variants:
                ENC.SCORE_PACK = pack
                ds = EvalDataset(ids, root, mode, subdir="")
                ds.min_samples, ds.max_samples = lo, hi
                out = os.path.join(root, "scores_%d_%d.txt" % (rnd, variants.index((name, mode, pack))))      # a fresh file per run
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                M.produce_evaluation_file(ds, model, dev, out, batch_size=batch_size)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert sum(1 for _ in open(out)) == n
                cut[name] = ds.n_cut
                if rnd == 0:      # the warm-up run: not timed, its scores kept for the comparison below
                    scores[name] = np.array([[float(v) for v in l.split()[1:]] for l in open(out)])
                    continue
                times[name].append(dt)
        ENC.SCORE_PACK = False
        for name, mode, _ in variants:
            audio = np.minimum(lens, hi if mode == "none" else 64600).sum() / 16000.0
            t = np.array(times[name])
            say("    --padding_type %-28s %s s  %s utterances/s  %s audio-seconds/s (%s)"
                % (name, "%.2f (%.2f - %.2f)" % (np.median(t), t.min(), t.max()), fmt(n / t), fmt(audio / t),
                   "whole files up to %.2f s, %d cut" % (hi / 16000.0, cut[name]) if mode == "none" else "the first 4.04 s of each file at most"))
        a, b = scores["none, SCL_AASIST_LENGTHS=1"], scores["none, + SCL_SCORE_PACK=1"]
        say("    scores, SCL_SCORE_PACK=1 against the padded rows: largest difference %.2e of the largest score" % (np.abs(a - b).max() / np.abs(a).max()))
        say("    none / zero: %.3f of the time per utterance; with SCL_SCORE_PACK=1 / without: %.3f of the time"
            % (np.median(times["none, SCL_AASIST_LENGTHS=1"]) / np.median(times["zero"]),
               np.median(times["none, + SCL_SCORE_PACK=1"]) / np.median(times["none, SCL_AASIST_LENGTHS=1"])))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: nothing here is meaningful on a CPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("whole-utterance scoring through the AASIST plugin on %s (tools/aasist_varlen_probe.py --n %d --batch_size %d)"
        % (torch.cuda.get_device_name(0), args.n, args.batch_size))
    end_to_end(args.n, args.batch_size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
