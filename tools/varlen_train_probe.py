"""Step time of training on a zero-padded batch with `lengths` against the fixed-length step (needs the MI355X).

One XLS-R-300M linear-plugin model in train mode, batch 64 x 64000 samples (199 frames), forward + loss + backward + AdamW step, input
resident in HBM, no RawBoost.  Six variants, alternated round by round inside one process so that they share the box's state:

  fixed        model(x): the fused attention kernels of csrc/attention.hip (T <= 224)
  varlen_full  model(x, lengths=[64000] * 64): the streaming kernels of csrc/attention_varlen.hip, every frame valid
  varlen_mix   model(x, lengths=mix): lengths drawn from a log-normal fit of ASVspoof 2019 LA durations (median 3.2 s, cut at the 4 s
               trim, at least 0.6 s), seeded
  pack_full    varlen_full with encoder.VARLEN_PACK on: the transformer layers on packed rows (csrc/attention_packed.hip) with nothing
               to skip — the cost of the pack / unpack passes
  pack_mix     varlen_mix with the switch on: the layers run over roundup(valid frames, PACK_ROWS) rows instead of 64 x 199
  pack_mix_varying  eight seeded mixes cycled step by step, all warmed: the launch plans switch between row-count buckets inside the
               timed window

Per variant: the median over the rounds of the mean step time of a round, and the rounds' minimum and maximum (the box's spread: a
difference between variants inside it is not a difference).  On the padded path the GEMMs run over all 64 x 199 rows whatever the lengths
are, so no speed-up is expected from varlen_mix (attention is about 3 ms of the step); on the packed path the row-wise kernels of the 24
layers follow the packed row count.  profiles/varlen_train.txt holds the first three variants as measured before the packed path existed.

    python tools/varlen_train_probe.py [--batch 64] [--samples 64000] [--rounds 5] [--steps 10] [--out profiles/varlen_pack.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def asvspoof_like_lengths(n, trim, seed=0, sr=16000):
    import numpy as np
    rs = np.random.RandomState(seed)
    sec = np.exp(rs.normal(np.log(3.2), 0.45, n))
    return [int(v) for v in np.clip(sec * sr, 0.6 * sr, trim).astype(np.int64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="a two-layer encoder with 64-wide heads (plumbing check, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_pack.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("varlen_train_probe: needs the GPU (a CPU run measures nothing)")
    from scl_amd import encoder as ENC
    from scl_amd import ops
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_linear import Model
    from scl_amd.optim import FusedAdamW
    dev = torch.device("cuda:0")
    cfg = W2VConfig(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8,
                    latent_groups=2) if args.tiny else W2VConfig()
    model = Model({"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}, dev, w2v_cfg=cfg, seed=0)
    model.train()
    opt = FusedAdamW(model, lr=1e-5, weight_decay=1e-4)
    conf = {"model": {"contra_mode": "all", "loss_type": 1}}
    B, L = args.batch, args.samples
    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(1234))).to(dev)
    y = torch.tensor(([1] * ((5 * B + 10) // 11) + [0] * B)[:B], device=dev)
    mix = asvspoof_like_lengths(B, L)
    T = cfg.conv_lens(L)[-1]
    frames = [cfg.conv_lens(n)[-1] for n in mix]
    mixes = [mix] + [asvspoof_like_lengths(B, L, seed=s) for s in range(1, 8)]
    # (name, the lengths of successive steps (cycled), encoder.VARLEN_PACK)
    variants = [("fixed", [None], False), ("varlen_full", [[L] * B], False), ("varlen_mix", [mix], False),
                ("pack_full", [[L] * B], True), ("pack_mix", [mix], True), ("pack_mix_varying", mixes, True)]
    rows = lambda lens: ops.packed_rows([cfg.conv_lens(n)[-1] for n in lens], T, ENC.PACK_ROWS)[1]

    def step(lengths, packed):
        ENC.VARLEN_PACK = packed      # read by the model at call time
        out, feats, emb = model(x) if lengths is None else model(x, lengths=lengths)
        total = sum(model.loss(out, feats, emb, y, conf).values())
        opt.zero_grad()
        total.backward()
        opt.step()
        return total

    for _, seq, packed in variants:      # every set of lengths warmed: each packed row count records its plans here
        for lengths in seq:
            for _ in range(args.warmup):
                step(lengths, packed)
    torch.cuda.synchronize()
    ms = {v[0]: [] for v in variants}
    for _ in range(args.rounds):
        for name, seq, packed in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                last = step(seq[i % len(seq)], packed)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert torch.isfinite(last).all()
    lines = ["varlen_train_probe: %s encoder, batch %d x %d samples (%d frames), train step = forward + loss + backward + AdamW"
             % ("tiny" if args.tiny else "XLS-R-300M", B, L, T),
             "%d rounds of %d steps per variant, variants alternated inside one process; ms per step" % (args.rounds, args.steps),
             "length mix: %d..%d samples, mean %.0f (%.1f of %d frames valid on average)"
             % (min(mix), max(mix), sum(mix) / B, sum(frames) / B, T),
             "packed rows (PACK_ROWS = %d) of %d padded: pack_full %d, pack_mix %d (%d valid, ratio %.3f), pack_mix_varying %s"
             % (ENC.PACK_ROWS, B * T, rows([L] * B), rows(mix), sum(frames), rows(mix) / (B * T), " ".join(str(rows(m)) for m in mixes)),
             "%-16s %9s %9s %9s   %s" % ("variant", "median", "min", "max", "utterances/s at the median")]
    for name, _, _ in variants:
        v = ms[name]
        med = statistics.median(v)
        lines.append("%-16s %9.2f %9.2f %9.2f   %.0f" % (name, med, min(v), max(v), B / med * 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
