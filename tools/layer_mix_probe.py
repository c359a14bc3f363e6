"""The layer mix (YAML `ssl_layer_mix`, csrc/layer_mix.hip) measured in one process.

    python tools/layer_mix_probe.py                    step of the linear plugin at 64 x 64000 with the mix off / on / on with a frozen
                                                       encoder, the fp32 scoring forward at 64 x 64600 off / on, each new kernel's achieved
                                                       bytes/s from stream events beside scl_adamw_flat's in the same process
    python tools/layer_mix_probe.py --launch-log F     the launch sequence of one recorded train step with the switch OFF (tiny encoder, train
                                                       mode: names and scalar arguments, no addresses) written to F — run it on two
                                                       commits and compare the files

Variants alternate, a warm-up each, median (min - max) of 5 rounds of 10 steps.  --batch / --layers shrink the run."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("SCL_PROBE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from scl_amd.optim import FusedAdamW  # noqa: E402

CONF = {"model": {"contra_mode": "all", "loss_type": 1}}
ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
ROUNDS, STEPS = 5, 10


def med(ts):
    return "%.3f (%.3f - %.3f)" % (statistics.median(ts), min(ts), max(ts))


def timed(fn, steps=STEPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def launch_log(path, dev):
    m = Model(dict(ARGS, w2v_arch="tiny"), dev, seed=0)
    m.train()
    x = 0.1 * torch.randn(4, 16000, generator=torch.Generator().manual_seed(1))
    y = torch.tensor([1, 1, 0, 0], device=dev)
    out, feats, emb = m(x.to(dev))
    sum(m.loss(out, feats, emb, y, CONF).values()).backward()
    torch.cuda.synchronize()
    lines = []
    for st in m._states.values():
        for key, plan in sorted(st["plans"].items(), key=lambda kv: str(kv[0])):
            lines.append("plan %s: %d calls" % (key, len(plan["calls"])))
            for _fn, args, name, _keep in plan["calls"]:
                scal = [a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and abs(a) < (1 << 31)]
                lines.append("  %s %s" % (name, " ".join(repr(a) for a in scal if not isinstance(a, ctypes.c_void_p))))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("launch log: %d lines -> %s" % (len(lines), path))


def kernel_rates(dev, rows, E, S):
    """Achieved bytes/s of the four kernels at [rows, E] with S states, and scl_adamw_flat's on 315 M parameters (30 B each)."""
    n = rows * E
    states = [torch.randn(n, device=dev) for _ in range(S)]
    logits = torch.randn(S, device=dev)
    g = (0.01 * torch.randn(n, device=dev)).to(torch.bfloat16)
    mix, gl, da = torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, device=dev), torch.empty(S, device=dev)
    ws = torch.empty(ops.layer_mix_bwd_w_ws_bytes(n, S), dtype=torch.uint8, device=dev)
    dx, dxb, acc = torch.randn(n, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, device=dev)
    npar = 315_438_720
    p, gr = torch.randn(npar, device=dev) * 0.02, torch.randn(npar, device=dev) * 1e-3
    m1, v1, pb = torch.zeros(npar, device=dev), torch.zeros(npar, device=dev), torch.empty(npar, dtype=torch.bfloat16, device=dev)
    cases = {
        "scl_layer_mix_fwd": (lambda: ops.layer_mix_fwd(states, logits, mix, n), n * (4 * S + 2)),
        "scl_layer_mix_bwd_w": (lambda: ops.layer_mix_bwd_w(g, states, logits, gl, ws, da, n), n * (4 * S + 2 + 4)),
        "scl_layer_mix_bwd_inject": (lambda: ops.layer_mix_bwd_inject(g, logits, 1, dx, dxb, n, seed=5, p=0.1), n * (2 + 4 + 4 + 2)),
        "scl_layer_mix_acc_f32": (lambda: ops.layer_mix_acc_f32(states[0], logits, 0, acc, n), n * 12),
        "scl_adamw_flat": (lambda: ops.adamw_flat(p, gr, m1, v1, pb, npar, 1e-5, 0.9, 0.999, 1e-8, 1e-4, 1), npar * 30),
    }
    ts = {k: [] for k in cases}
    for fn, _ in cases.values():
        fn()
    for _ in range(ROUNDS):
        for k, (fn, _) in cases.items():
            ts[k].append(timed(fn))
    rates = {}
    for k, (_, nbytes) in cases.items():
        t = statistics.median(ts[k])
        rates[k] = nbytes / t / 1e9
        print("%-26s %s ms  %.2f TB/s (%.3f GB per launch)" % (k, med(ts[k]), rates[k], nbytes / 1e9))
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch-log")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layers", type=int, default=24)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.launch_log:
        return launch_log(a.launch_log, dev)
    B, Lyr = a.batch, a.layers
    cfg_off = W2VConfig(layers=Lyr)
    T = cfg_off.conv_lens(64000)[-1]
    rates = kernel_rates(dev, B * T, cfg_off.embed, Lyr + 1)
    variants = {"off": (cfg_off, False), "on": (cfg_off.with_layer_mix(), False), "on_frozen": (cfg_off.with_layer_mix(), True)}
    x = (0.1 * torch.randn(B, 64000, generator=torch.Generator().manual_seed(2))).to(dev)
    xs = (0.1 * torch.randn(B, 64600, generator=torch.Generator().manual_seed(3))).to(dev)
    y = (torch.arange(B) % 2).to(dev)
    run = {}
    for name, (cfg, frozen) in variants.items():
        m = Model(dict(ARGS, flag_fix_ssl=frozen), dev, w2v_cfg=cfg, seed=0)
        m.train()
        opt = FusedAdamW(m, lr=1e-5, weight_decay=1e-4)

        def train_step(m=m, opt=opt):
            out, feats, emb = m(x)
            opt.zero_grad()
            sum(m.loss(out, feats, emb, y, CONF).values()).backward()
            opt.step()

        def score(m=m):
            m.eval()
            with torch.no_grad():
                m(xs)
            m.train()
        run[name] = (train_step, score)
        for _ in range(2):
            train_step()
        if not frozen:
            score()
    t_train, t_score = {k: [] for k in run}, {k: [] for k in run if k != "on_frozen"}
    for _ in range(ROUNDS):
        for k, (train_step, score) in run.items():
            t_train[k].append(timed(train_step))
        for k in t_score:
            t_score[k].append(timed(run[k][1], 3))
    for k in run:
        print("train step %-10s %s ms" % (k, med(t_train[k])))
    for k in t_score:
        print("fp32 score %-10s %s ms" % (k, med(t_score[k])))
    n = B * T * cfg_off.embed
    S = Lyr + 1
    bytes_step = n * (4 * S + 2) + n * (4 * S + 2 + 4) + (Lyr - 1) * n * 12 + n * 8
    added = statistics.median(t_train["on"]) - statistics.median(t_train["off"])
    budget = 2 * bytes_step / rates["scl_adamw_flat"] / 1e9      # bytes / (TB/s) = 1e-12 s = 1e-9 ms
    print("added step time %.3f ms; budget 2 x (%.2f GB / %.2f TB/s) = %.3f ms -> %s"
          % (added, bytes_step / 1e9, rates["scl_adamw_flat"], budget, "within" if added <= budget else "EXCEEDED"))


if __name__ == "__main__":
    main()
