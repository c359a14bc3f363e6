"""Step time of training the ResNet plugin on a zero-padded batch with `lengths` against the fixed-length step (needs the MI355X).

One XLS-R-300M `wav2vec2_resnet_nll` model (ResNet-18 back-end) in train mode, batch 32 x 64000 samples (199 frames), forward + loss +
backward + AdamW step, input resident in HBM.  Five variants, alternated round by round inside one process so that they share the box's
state (after tools/varlen_train_probe.py, the linear plugin's twin):

  fixed        model(x): unmasked BatchNorm kernels (scl_bn_fwd / scl_bn_bwd), fused attention
  varlen_full  model(x, lengths=[64000] * 32): the masked BatchNorm pair (scl_bn_fwd_masked / scl_bn_bwd_masked) with every row valid,
               the encoder's streaming attention under its padding mask
  varlen_mix   model(x, lengths=mix): lengths drawn from the log-normal fit of ASVspoof 2019 LA durations of profiles/varlen_train.txt
               (median 3.2 s, cut at the 4 s trim), counted as at least 17,680 samples (the back-end's minimum, as main.py's packs are)
  pack_full    varlen_full with encoder.VARLEN_PACK on: the transformer layers on packed rows, nothing to skip; the back-end stays padded
  pack_mix     varlen_mix with the switch on

Per variant: the median over the rounds of the mean step time of a round, and the rounds' minimum and maximum.  `--only a,b` runs a subset
(for a kernel trace of one masked variant next to the fixed step: the masked kernels carry `_masked` in their names).

    python tools/resnet_varlen_train_probe.py [--batch 32] [--samples 64000] [--rounds 5] [--steps 10] [--out profiles/resnet_varlen_train.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.varlen_train_probe import asvspoof_like_lengths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated variant names (default: all)")
    ap.add_argument("--tiny", action="store_true", help="a two-layer encoder with 64-wide heads (plumbing check, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_varlen_train.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("resnet_varlen_train_probe: needs the GPU (a CPU run measures nothing)")
    from scl_amd import encoder as ENC
    from scl_amd import resnet_head as RH
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_resnet import Model
    from scl_amd.optim import FusedAdamW
    dev = torch.device("cuda:0")
    cfg = W2VConfig(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8,
                    latent_groups=2) if args.tiny else W2VConfig()
    model = Model({"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "resnet": RH.DEFAULT_RESNET}, dev, w2v_cfg=cfg, seed=0)
    model.train()
    opt = FusedAdamW(model, lr=1e-5, weight_decay=1e-4)
    conf = {"model": {"contra_mode": "all", "loss_type": 1}}
    B, L = args.batch, args.samples
    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(1234))).to(dev)
    y = torch.tensor(([1] * ((5 * B + 10) // 11) + [0] * B)[:B], device=dev)
    lo = model.min_samples()
    mix = [max(n, lo) for n in asvspoof_like_lengths(B, L)]
    T = cfg.conv_lens(L)[-1]
    frames = [cfg.conv_lens(n)[-1] for n in mix]
    variants = [("fixed", None, False), ("varlen_full", [L] * B, False), ("varlen_mix", mix, False), ("pack_full", [L] * B, True),
                ("pack_mix", mix, True)]
    if args.only:
        keep = args.only.split(",")
        variants = [v for v in variants if v[0] in keep]

    def step(lengths, packed):
        ENC.VARLEN_PACK = packed      # read by the model at call time
        out, feats, emb = model(x) if lengths is None else model(x, lengths=lengths)
        total = sum(model.loss(out, feats, emb, y, conf).values())
        opt.zero_grad()
        total.backward()
        opt.step()
        return total

    for _, lengths, packed in variants:
        for _ in range(args.warmup):
            step(lengths, packed)
    torch.cuda.synchronize()
    ms = {v[0]: [] for v in variants}
    for _ in range(args.rounds):
        for name, lengths, packed in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last = step(lengths, packed)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert torch.isfinite(last).all()
    rows_full, rows_mix = RH.batch_rows([T] * B), RH.batch_rows(frames)
    lines = ["resnet_varlen_train_probe: %s encoder + ResNet-18 back-end, batch %d x %d samples (%d frames), train step = forward + loss + "
             "backward + AdamW" % ("tiny" if args.tiny else "XLS-R-300M", B, L, T),
             "%d rounds of %d steps per variant, variants alternated inside one process; ms per step" % (args.rounds, args.steps),
             "length mix: %d..%d samples, mean %.0f (%.1f of %d frames valid on average, ratio %.3f)"
             % (min(mix), max(mix), sum(mix) / B, sum(frames) / B, T, sum(frames) / (B * T)),
             "valid rows of the back-end's maps, mix / full, per level (frames, conv1, layer1..4, conv5): %s"
             % " ".join("%.3f" % (sum(a) / sum(b)) for a, b in zip(rows_mix, rows_full)),
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
