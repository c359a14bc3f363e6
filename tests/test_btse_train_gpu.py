"""The wav2vec2_btse back-end at the batch sizes training runs, against the float64 oracle on the CPU.

The goldens (tests/golden/btse.npz) stop at batch 4 x 20 frames, the other oracle comparisons of tests/test_btse_gpu.py at
M = B x T = 144 rows, and the batch-128 plugin step there compares the head's gradients but not the head on its own.  Several
reductions of the backward (scl_amd/btse_head.py::_BtseFn.backward) are partitioned by the batch size and open up only at large M:
  * the weight gradients of the three frame-level linears run as sk = min(32, M // 128) split-K slabs of the exact-fp32 GEMM
    (csrc/gemm_f32.hip: nk_per / kbegin / kend) summed by reduce_slabs.  At B = 128 (M = 25472) that is 32 slabs of 25 K-steps, the
    last one 21.  At B = 14 (one conf-5 pack, M = 2786) it is 21 slabs of which only 18 hold K-steps, the last of those ending in a
    2-row partial tile; slabs 18 - 20 must be written as zeros;
  * the bias column sums (colsum_reduce: 100 / 11 partial rows, finished by a ticket);
  * meanpool_bwd and the backward GEMMs (rmode 2) redraw the forward's dropout masks from their seeds at element indices up to 3.26 M;
  * the bio-transformer gradients: one slab row per utterance (csrc/btse.hip btse_rows_bwd_kernel; a padded utterance's row is
    zeroed), summed over B rows by reduce_slabs; with is_add, the join's dW1 / db1 summed over B (btse_join_bwd_kernel).
Here the product head (BtseHead on the GPU, default kernels, fp32) and the oracle (oracle/btse.py, pinned to the reference's own Model
by tests/test_btse_cpu.py) run in float64 on the CPU with an identity LL, on the same features [B, 199, 128], weights
(oracle.aasist.fill_state) and tokens in [0, 3).  Cases: conf-5-btse-trans64 (concat) at B = 128 and at B = 14 (7 bona fide + 7
spoof) in train and eval mode; B = 128 with mixed token lengths (1, 63, 64, 65, 128, 198, 199, ...) in eval mode; is_add with
bio_out 128 and 200 tokens at B = 128 in train mode.  In train mode the MLP dropout (p = 0.5, not switchable) is rebuilt on the host
from the head's seed (test_dropout_gpu.keep_scale) and handed to the oracle.

The upstream gradient is the real loss's: oracle.head.model_loss on the float64 outputs gives d logp (L_CE) and d b (L_CF2), and
both backward passes receive the same values.  The oracle runs in chunks of CHUNK utterances (forward_chunked without autograd for
the outputs and the upstream gradient, then one autograd pass per chunk with its slice of that gradient; the parameter gradients
accumulate in float64).  Each case runs two steps on two inputs with the same weights; the second runs with the parameters' .grad
zeroed in place (the plugin's flat buffer) instead of None and with device-resident tokens (bench.py's path through
_queue_token_check), on the same cached plan.  Between each forward and its backward every plan buffer the backward writes in full
before it reads it is filled with NaN (POISONED): a slab, a partial row or a scratch entry left unwritten reaches a gradient.

Compared: logp and b (and b's emb / bio-score column blocks), the gradient at the features, EVERY parameter gradient (conv_k.bias
is analytically zero: bounded against the step's largest reference gradient; the frozen m_utt_level gets none), and with mixed
lengths an exactly-zero bio score for every padded utterance.  Metric: relative L2 per tensor, plus max |error| / max |reference| for
the outputs.  Measured worst values on the MI355X are written next to the bars.

Discontinuities are not tolerances.  The pre-activations of the MLP's leaky_relu and the bio FFN's relu within KINK_REL of their
site's RMS of zero are counted and printed.  Where the GPU's fp32 pre-activation of an MLP layer and the float64 one fall on opposite
sides of the leaky_relu kink (a few elements per step at B = 128, ~1e-7 x RMS from zero), the oracle takes the product's side
(product_branches); every such element must lie within KINK_REL x RMS of zero, and the counts are printed.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import btse as OB  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402
from scl_amd.btse_head import DROP_P, BtseHead  # noqa: E402
from test_backends_train_gpu import KINK_REL, Report, kink_counter, maxrel, rl2, upstream  # noqa: E402
from test_dropout_gpu import keep_scale  # noqa: E402

pytestmark = pytest.mark.gpu

# Bars: about 2-3 x the worst value measured on the MI355X over every case and both steps (measured value in the comment).
# out: logp / b / b's column blocks, rel-L2 and max |error| / max |reference|; grad_x: d feats, rel-L2; grad: a parameter gradient,
# rel-L2; zero-grad: conv_k.bias, max |g| over the step's largest reference gradient.
BARS = {"out": 5e-7,            # 1.9e-7  (logp, add-128-train)
        "out-max": 1e-6,        # 4.6e-7  (logp, padded-128-eval)
        "grad_x": 1e-6,         # 3.6e-7  (concat-14-eval)
        "grad": 1e-4,           # 4.6e-5  (attn_layers.2.conv_q.bias, concat-14-eval)
        "zero-grad": 1e-7}      # 4.6e-8  (attn_layers.2.conv_k.bias, padded-128-eval)
T = 199             # frames of a 64000-sample clip
CHUNK = 32          # utterances per oracle chunk
KINK_SITES = ((F, "leaky_relu"), (torch, "relu"))       # the MLP (linear.py:30) and the bio FFN (transformer.py:288)
PADDED_LENS = (1, 63, 64, 65, 128, 198, 199)
# plan buffers the backward writes in full before it reads them: the weight-gradient slabs, the per-utterance bio rows and their sum,
# the column-sum partial rows, the tail's and the join's outputs, the tail's scratch, the MLP's pre-activation gradients
POISONED = ("wslab", "slab", "gbio", "cs", "db", "demb", "ds", "tail_ws")

# (id, B, tokens, mixed lengths, is_add, train mode)
CASES = [("concat-128-train", 128, 199, False, False, True),
         ("concat-128-eval", 128, 199, False, False, False),
         ("concat-14-train", 14, 199, False, False, True),
         ("concat-14-eval", 14, 199, False, False, False),
         ("padded-128-eval", 128, 199, True, False, False),
         ("add-128-train", 128, 200, False, True, True)]


def labels(B):
    """58 bona fide + 70 spoof at B = 128 (tests/test_btse_gpu.py), 7 + 7 in one conf-5 pack."""
    nb = 58 if B == 128 else B // 2
    return torch.tensor([1] * nb + [0] * (B - nb))


def lengths(B, Lt, mixed, rs):
    if not mixed:
        return torch.full((B,), Lt, dtype=torch.int32)          # what bench.py and get_Bio produce
    lens = rs.randint(1, Lt + 1, size=B)
    lens[:len(PADDED_LENS)] = PADDED_LENS
    lens[len(PADDED_LENS)::3] = Lt         # a third of the rest at full length: only those carry bio-transformer gradients
    return torch.from_numpy(lens.astype(np.int32))


def dropout_masks(seed, B, T):
    """The three MLP masks of the forward that finds `seed` in the head (btse_head.py::_BtseFn.forward draws from the next state)."""
    s0 = (seed * 1664525 + 1013904223) & 0x7FFFFFFF
    return [keep_scale((s0 + 7919 * j) & 0x7FFFFFFF, B * T * 128, DROP_P).view(B, T, 128) for j in range(3)]


def product_branches(sd, x, masks, pres):
    """The three MLP masks for the oracle with the product's side of every leaky_relu kink folded in.  Where the fp32 pre-activation
    on the GPU (the plan's `pre`, which the backward differentiates) and the float64 one have opposite signs, the slopes differ by 100x;
    one such element of 3.26 M moves d feats by ~5e-4 rel-L2.  There the factor 100 or 0.01 gives the oracle the product's slope (the
    forward value moves by less than KINK_REL x RMS).  Every sign difference must lie within KINK_REL x RMS of zero: one away from
    the kink is an error of the product, not a kink.  Returns (masks, flips per layer)."""
    B, T = x.shape[:2]
    out, flips = [], []
    h = x.double()
    with torch.no_grad():
        for j in range(3):
            pre = "backend.mlp.m_frame_level.linear_%d." % j
            z = F.linear(h, sd[pre + "weight"], sd[pre + "bias"])
            flip = (z > 0) != (pres[j].view(B, T, 128).cpu() > 0)
            rms = z.pow(2).mean().sqrt()
            assert (z[flip].abs() < KINK_REL * rms).all(), \
                "layer %d: %d pre-activations with the wrong sign, largest %.2e x RMS" % (j, int(flip.sum()), (z[flip].abs().max() / rms).item())
            m = torch.ones_like(z) if masks is None else masks[j].double()
            m = torch.where(flip, torch.where(z > 0, 0.01, 100.0).to(z.dtype), 1.0) * m
            h = F.leaky_relu(z, 0.01) * m
            out.append(m)
            flips.append(int(flip.sum()))
    return out, flips


def oracle_sd(filled):
    """Float64 leaves of the head's parameters; the oracle applies LL first, so LL is the identity (the product starts at feats)."""
    sd = {k: v.double().requires_grad_(True) for k, v in filled.items() if not k.startswith("backend.LL.")}
    sd["backend.LL.weight"] = torch.eye(128, dtype=torch.float64)
    sd["backend.LL.bias"] = torch.zeros(128, dtype=torch.float64)
    return sd


def oracle_backward(sd, args, x, bio, lens, masks, dl, db):
    """Autograd through oracle.btse.forward chunk by chunk with that chunk's slice of the fixed upstream gradient (dl, db); the
    parameter gradients accumulate in sd's .grad.  Returns d x."""
    dx = []
    for i in range(0, x.shape[0], CHUNK):
        xc = x[i:i + CHUNK].double().requires_grad_(True)
        mc = None if masks is None else [m[i:i + CHUNK] for m in masks]
        lp, _, b = OB.forward(sd, args, xc, bio[i:i + CHUNK], lens[i:i + CHUNK], mc)
        torch.autograd.backward([lp, b], [dl[i:i + CHUNK].to(lp.dtype), db[i:i + CHUNK].to(b.dtype)])
        dx.append(xc.grad)
    return torch.cat(dx)


def compare_head_grads(rep, got, sd):
    """got: {name: gradient or None} of every BtseHead parameter.  rel-L2 per gradient; conv_k.bias (analytically zero) bounded against
    the step's largest reference gradient; the frozen m_utt_level has no gradient on either side.  Returns the number compared."""
    casemax = max(v.grad.abs().max().item() for v in sd.values() if v.grad is not None)
    n = 0
    for name, g in got.items():
        r = sd[name].grad
        if name in BtseHead.frozen_names:
            assert (g is None or not g.any()) and r is None, "%s: the frozen MLP logits layer got a gradient" % name
            continue
        assert g is not None and r is not None and tuple(g.shape) == tuple(r.shape), name
        if "conv_k.bias" in name:
            rep.check("zero-grad", name, max(g.abs().max().item(), r.abs().max().item()) / casemax)
        else:
            rep.check("grad", name, rl2(g, r))
        n += 1
    return n


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_btse_backend_matches_float64_oracle(dev, case):
    tag, B, Lt, mixed, is_add, training = case
    args = OB.default_args(is_add=is_add, bio_out=128 if is_add else 64)
    filled = {k: torch.from_numpy(v) for k, v in fill_state(OB.state_shapes(args, 128), seed=3000 + B + Lt).items()}
    head = BtseHead(args).to(dev)
    missing, unexpected = head.load_state_dict({k: v for k, v in filled.items() if not k.startswith("backend.LL.")}, strict=True)
    assert not missing and not unexpected
    head.train(training)
    BtseHead.reseed(head, 4099 + B + Lt)
    sd = oracle_sd(filled)
    hp = dict(head.named_parameters())
    # preconditions: the split-K weight gradient path with the slab layout the module docstring describes
    M = B * T
    sk = min(32, M // 128)
    nk = (M + 31) // 32
    per = (nk + sk - 1) // sk
    assert (sk, per, nk - (nk - 1) // per * per, (nk + per - 1) // per) == {128: (32, 25, 21, 32), 14: (21, 5, 3, 18)}[B]
    rs = np.random.RandomState(B + Lt)
    lens = lengths(B, Lt, mixed, rs)
    y = labels(B)
    rep = Report(tag, BARS)
    plan = None
    for step in range(2):
        rep.step = step
        x = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(6007 * step + B + Lt))
        bio = torch.from_numpy(rs.randint(0, 3, size=(B, Lt)).astype(np.int32))
        masks = dropout_masks(head.__dict__["_seed"], B, T) if training else None
        if training:
            fr = [(m == 0).double().mean().item() for m in masks]
            assert all(abs(f - DROP_P) < 5e-3 for f in fr), fr
        # ---- product forward: host int32 tokens in step 0, device-resident ones in step 1
        xg = x.to(dev).requires_grad_(True)
        tok, tl = (bio, lens) if step == 0 else (bio.to(dev), lens.to(dev))
        logp, b = BtseHead.forward(head, xg, tok, tl)
        plans = [pl for key, pl in head.__dict__["_btse_plans"].items() if key[:3] == (B, T, Lt)]
        assert len(plans) == 1 and (plan is None or plans[0] is plan), "the second step did not reuse the cached plan"
        plan = plans[0]
        # ---- float64 reference: outputs and the loss's upstream gradient without autograd, then the backward chunk by chunk
        omasks, flips = product_branches(sd, x, masks, plan["pre"])
        kinks = {}
        with torch.no_grad(), kink_counter(kinks, KINK_SITES):
            ro, _, rb = OB.forward_chunked(sd, args, x.double(), bio, lens, omasks, CHUNK)
        dl, db = upstream(ro, rb, x.double(), y, 1.0)
        assert dl.abs().max() > 0 and db.abs().max() > 0
        rdx = oracle_backward(sd, args, x, bio, lens, omasks, dl, db)
        # ---- product backward on poisoned scratch
        for k in POISONED:
            plan[k].fill_(float("nan"))
        for t in plan["dpre"]:
            t.fill_(float("nan"))
        torch.autograd.backward([logp, b], [dl.float().to(dev), db.float().to(dev)])
        torch.cuda.synchronize()
        if step:
            BtseHead.check_tokens(head)
        print("\n[%s step %d] pre-activations within %.0e x RMS of a kink: %s; leaky_relu sign differences (GPU / float64) per layer: %s"
              % (tag, step, KINK_REL, kinks, flips))
        blocks = [("logp", logp, ro), ("b", b, rb)]
        if not is_add:
            blocks += [("b[emb]", b[:, :128], rb[:, :128]), ("b[bio]", b[:, 128:], rb[:, 128:])]
        for name, g, r in blocks:
            rep.check("out", name, rl2(g, r))
            rep.check("out-max", name, maxrel(g, r))
        if mixed:
            for i, n in enumerate(lens.tolist()):
                if n < Lt:      # model.py:234-236: the read-out position is padding
                    assert (b[i, 128:] == 0).all() and (rb[i, 128:] == 0).all(), (step, i, n)
        rep.check("grad_x", "feats", rl2(xg.grad, rdx))
        n = compare_head_grads(rep, {k: p.grad for k, p in hp.items()}, sd)
        assert n == len(hp) - 2, n
        for p in list(hp.values()) + list(sd.values()):
            if p.grad is not None:
                p.grad.zero_()
    rep.done()
