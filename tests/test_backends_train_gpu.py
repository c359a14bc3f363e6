"""The AASIST and ResNet back-ends at the batch sizes training runs, against the float64 oracles on the CPU.

The goldens (tests/golden/aasist.npz, resnet.npz) stop at batch 4, and the head tests of the full-size steps check only
size-independent properties.  Several reductions of the back-ends are partitioned by the batch size: the BatchNorm statistics
(csrc/nn.hip scl_bn_nslabs, the rs_finish.h atomics + ticket of csrc/resstack.hip and csrc/graph.hip), the convolution weight
gradients of hipnn.py (flat split-K slabs, or one slab per utterance), the per-utterance gradient rows of graph.py and the bias
column sums.  Here the product back-end (scl_amd/aasist_head.py, scl_amd/resnet_head.py; default kernels, fp32 on the GPU) and the
oracle head (oracle/aasist_head.py, oracle/resnet_head.py; pinned to the reference's own Model by tests/test_aasist_cpu.py and
tests/test_resnet_cpu.py) run in float64 on the CPU on the same features and weights (oracle.aasist.fill_state), at batch 64 / 11
(AASIST) and 32 / 11 (ResNet; 11 = one multi-view pack, 5 bona fide + 6 spoof), in train mode (dropout p = 0) and in eval mode.

The upstream gradient is the real loss's: oracle.head.model_loss on the float64 outputs gives d logits and d hidden / d emb, and both
backward passes receive the same values.  Two steps on two inputs with the same weights check everything twice; the second step's
running statistics have seen two updates, and the second step runs with the parameters' .grad zeroed in place (the plugins' flat
gradient buffer) instead of None.  A reduction that leaves its accumulators or ticket dirty, or a cached plan with stale state, shows
up by step 2 at the latest.

Compared: logits, hidden / emb, the input gradient, EVERY parameter gradient (the analytically zero ones bounded near zero, as
tests/test_aasist_cpu.py::analytically_zero), every BatchNorm running_mean / running_var / num_batches_tracked.  Metric: relative L2
per tensor, plus max |error| / max |reference| for the outputs.  Measured worst values on the MI355X are written next to the bars.

Discontinuities are preconditions, not tolerances: the top-k of every GraphPool must have a margin between its k-th and (k+1)-th
float64 score above TOPK_MARGIN for every utterance (the seeds are chosen so; AASIST eval mode runs on running statistics taken from
a separate batch, see calibrate()), and the pre-activations of every SELU / ReLU within
1e-5 of their site's RMS of zero are counted and printed (a slope flip there is the only O(1) effect fp32 can have).

Where a bar is wider than 1e-3, the cause is the conditioning of the function in fp32, not the kernels; measured:
  * one-element gradients (first_bn.weight / .bias: BatchNorm2d(1) over the whole map; GraphPool proj.bias) are single sums over
    every position of the batch with heavy cancellation.  The same oracle run by torch in fp32 on the CPU is off by 6e-3
    (AASIST first_bn.weight, B = 11), 7.8e-4 (pool_hS2.proj.bias, B = 64, T = 202), 3.6e-2 / 1.6e-2 (ResNet first_bn, B = 32).
  * ResNet gradients in train mode: torch fp32 on the CPU is off by 4.3e-3 at B = 32 (layer4.1.bn2.bias; 2.9e-3 at B = 11), the
    GPU by 4.8e-3.  With exact-fp32 backward products (SCL_RESNET_X3BWD=0) the GPU errors are unchanged to two digits, so the
    bf16-pair backward is not the cause; in eval mode the same comparison gives grad_x 3.8e-4 (torch fp32, B = 32) against 1.2e-3.
The mutations these tests were checked against (one slab fewer in the BatchNorm finish or in a convolution's weight-gradient
reduction, one utterance fewer in a reduction, accumulators not re-zeroed) move the affected tensors by 1e-5 .. 1e+1.
"""
import contextlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import head as OH  # noqa: E402
from oracle import resnet_head as ORH  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402
from oracle.aasist_head import AasistHead as OracleAasist  # noqa: E402
from oracle.aasist_head import GraphPool as OracleGraphPool  # noqa: E402
from scl_amd import graph, resnet_head, resstack  # noqa: E402
from scl_amd.aasist_head import UPSTREAM_AASIST, AasistHead  # noqa: E402
from scl_amd.resnet_head import DEFAULT_RESNET, ResNetHead  # noqa: E402
from test_aasist_cpu import analytically_zero  # noqa: E402

pytestmark = pytest.mark.gpu

# Bars: about 2-3 x the worst value measured on the MI355X over every case of the group and both steps (measured value in the comment).
# out: logits / hidden / emb, rel-L2 and max |error| / max |reference|; grad: a parameter gradient, rel-L2; grad-scalar: a one-element
# parameter (see the module docstring); buffer: running_mean / running_var, rel-L2; zero-grad: an analytically zero gradient, max |g|
# over the step's largest reference gradient.
BARS_AASIST = {"out": 3e-6,             # 9.8e-7  (hidden)
               "out-max": 5e-6,         # 1.9e-6
               "grad_x": 3e-4,          # 1.1e-4
               "grad": 1e-3,            # 4.5e-4  (encoder.2.0.bn2.bias, B = 11)
               "grad-scalar": 5e-2,     # 1.7e-2  (pool_hS2.proj.bias, B = 64, T = 202); 1.1e-2 (first_bn.weight, B = 11)
               "buffer": 2e-6,          # 7.7e-7  (first_bn.running_mean, B = 11)
               "zero-grad": 2e-6}       # 5.3e-7
BARS_RESNET = {True: {"out": 3e-6,              # 9.6e-7
                      "out-max": 5e-6,          # 2.0e-6
                      "grad_x": 1e-2,           # 3.6e-3  (B = 32)
                      "grad": 1.2e-2,           # 4.8e-3  (layer4.1.bn2.bias, B = 32)
                      "grad-scalar": 3e-1,      # 1.1e-1  (first_bn.bias, B = 32)
                      "buffer": 3e-7},          # 9.9e-8
               False: {"out": 1e-6,             # 3.6e-7
                       "out-max": 2e-6,         # 6.7e-7
                       "grad_x": 4e-3,          # 1.5e-3  (B = 11)
                       "grad": 3e-3,            # 1.1e-3  (conv1.weight, B = 11)
                       "grad-scalar": 3e-3,     # 1.0e-3  (first_bn.bias, B = 11)
                       "buffer": 1e-6}}         # 0: eval leaves them alone
TOPK_MARGIN = 1e-5      # float64 gap between the k-th and (k+1)-th GraphPool score, every pool and utterance
KINK_REL = 1e-5         # |pre-activation| < KINK_REL * RMS of its site counts as "at the kink"


def n_bona(B):
    """Labels in the proportion of one pack (5 bona fide of 11): both classes present at every batch size."""
    return B * 5 // 11


def labels(B):
    return torch.tensor([1] * n_bona(B) + [0] * (B - n_bona(B)))


def rl2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def maxrel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


@contextlib.contextmanager
def kink_counter(counts, sites=((F, "selu"), (F, "relu"))):
    """Counts, per activation function, the pre-activations within KINK_REL x RMS of zero of every call inside of the (module,
    function name) sites (default: F.selu / F.relu)."""
    orig = {(m, n): getattr(m, n) for m, n in sites}

    def wrap(m, n):
        def f(x, *a, **kw):
            with torch.no_grad():
                rms = x.detach().pow(2).mean().sqrt()
                counts[n] = counts.get(n, 0) + int((x.detach().abs() < KINK_REL * rms).sum())
            return orig[(m, n)](x, *a, **kw)
        return f
    for m, n in orig:
        setattr(m, n, wrap(m, n))
    try:
        yield counts
    finally:
        for (m, n), f in orig.items():
            setattr(m, n, f)


class Report:
    """Collects every metric against its bar; the test fails once, listing every tensor over its bar."""

    def __init__(self, tag, bars):
        self.tag, self.bars, self.worst, self.fails, self.step = tag, bars, {}, [], 0

    def check(self, kind, name, value):
        bar = self.bars[kind]
        name = "step %d %s" % (self.step, name)
        if not (value == value) or value >= bar:
            self.fails.append("%s %s: %.3e >= %.0e" % (kind, name, value, bar))
        w = self.worst.get(kind)
        if w is None or value > w[0]:
            self.worst[kind] = (value, name)

    def done(self):
        print("\n[%s] worst:" % self.tag, ", ".join("%s %.2e (%s)" % (k, v, n) for k, (v, n) in sorted(self.worst.items())))
        assert not self.fails, "%s: %d over the bar:\n  %s" % (self.tag, len(self.fails), "\n  ".join(self.fails))


def fill(module, seed):
    filled = fill_state({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed=seed)
    return {k: torch.from_numpy(v) for k, v in filled.items()}


def set_mode(modules, training):
    for m in modules:
        m.train(training)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0


def compare_params(rep, gpu_params, ref_params, training, zero_ok=lambda name, training: False):
    """Every parameter: rel-L2 of the gradient, or (analytically zero) both sides bounded by the step's largest gradient x a bar.
    Returns the number of parameters checked; parameters without a reference gradient must have none (or an all-zero one) on the GPU."""
    casemax = max(p.grad.abs().max().item() for p in ref_params.values() if p.grad is not None)
    assert set(gpu_params) == set(ref_params)
    n = 0
    for name, rp in ref_params.items():
        g = gpu_params[name].grad
        if rp.grad is None:
            assert g is None or not g.any(), "%s has a gradient on the GPU only" % name
            continue
        assert g is not None and g.shape == rp.grad.shape, name
        if zero_ok(name, training):
            rep.check("zero-grad", name, max(g.abs().max().item(), rp.grad.abs().max().item()) / casemax)
        else:
            rep.check("grad-scalar" if rp.numel() == 1 else "grad", name, rl2(g, rp.grad))
        n += 1
    return n


def batch_counts(module):
    return {n: int(b) for n, b in module.named_buffers() if n.endswith("num_batches_tracked")}


def compare_buffers(rep, gpu, ref, nbt0, steps):
    """running_mean / running_var by rel-L2; num_batches_tracked exactly, `steps` more than at the start (0 in eval; an unused
    BatchNorm stays put)."""
    gb, rb = dict(gpu.named_buffers()), dict(ref.named_buffers())
    assert set(gb) == set(rb)
    for name, r in rb.items():
        if name.endswith("num_batches_tracked"):
            assert int(gb[name]) == int(r) and int(r) - nbt0[name] in (0, steps), (name, int(gb[name]), int(r), nbt0[name])
        else:
            rep.check("buffer", name, rl2(gb[name], r))


def upstream(out, hid_or_emb, feats, y, scale):
    """d logits, d hidden / d emb of the plugin's loss (oracle.head.model_loss, x scale) at the float64 reference outputs; the feature
    term L_CF1 does not pass through the back-end.  Leaf copies: the partial derivatives, the logits path into hidden / emb is the
    back-end's own."""
    o, h = out.detach().requires_grad_(True), hid_or_emb.detach().requires_grad_(True)
    losses = OH.model_loss(o, feats.detach(), h, y, 1)
    return torch.autograd.grad(scale * sum(losses.values()), [o, h])


# ---- AASIST -----------------------------------------------------------------------------------------------------------------------------
AASIST_CASES = [(64, 199, True), (64, 199, False), (11, 199, True), (11, 199, False), (64, 202, True)]


def topk_margins(ref, store):
    """Forward hooks on every oracle GraphPool: the float64 gap between the k-th and (k+1)-th score, per utterance."""
    def hook(mod, inp, out):
        with torch.no_grad():
            h = inp[0]
            s = torch.sigmoid(mod.proj(h)).squeeze(-1)
            keep = max(int(h.size(1) * mod.k), 1)
            top = torch.topk(s, keep + 1, dim=1).values
            store.append((top[:, keep - 1] - top[:, keep]).min().item())
    return [m.register_forward_hook(hook) for m in ref.modules() if isinstance(m, OracleGraphPool)]


def calibrate(ref, x):
    """Eval-mode running statistics that fit the data: one train-mode float64 forward with momentum 1 (running = that batch's
    statistics).  With fill_state's arbitrary running statistics the graph's scores saturate the sigmoid and the top-k margins fall
    to ~1e-6, below what fp32 can order reliably."""
    bns = [m for m in ref.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    for m in bns:
        m.momentum = 1.0
    set_mode((ref,), True)
    with torch.no_grad():
        ref(x)
    for m in bns:
        m.momentum = 0.1


@pytest.mark.parametrize("B,T,training", AASIST_CASES, ids=["%d-%d-%s" % (B, T, "train" if t else "eval") for B, T, t in AASIST_CASES])
def test_aasist_backend_matches_float64_oracle(dev, B, T, training):
    gpu = AasistHead(UPSTREAM_AASIST).to(dev)
    ref = OracleAasist(UPSTREAM_AASIST).double()
    ref.load_state_dict(fill(gpu, seed=1000 + B))
    if not training:
        calibrate(ref, torch.randn(B, T, 128, generator=torch.Generator().manual_seed(31 + B + T)).double())
    gpu.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    set_mode((gpu, ref), training)
    y = labels(B)
    nbt0 = batch_counts(ref)
    gparams, rparams = dict(gpu.named_parameters()), dict(ref.named_parameters())
    rep = Report("aasist B=%d T=%d %s" % (B, T, "train" if training else "eval"), BARS_AASIST)
    seen = lambda mod: {(id(pl), getattr(pl, "gen", 0)) for pl in mod._PLANS}
    for step in range(2):
        rep.step = step
        x = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(7919 * step + B + T))
        # ---- float64 reference
        xr = x.double().requires_grad_(True)
        margins, kinks = [], {}
        hooks = topk_margins(ref, margins)
        with kink_counter(kinks):
            ro, rh = ref(xr)
        for h in hooks:
            h.remove()
        assert len(margins) == 6 and min(margins) > TOPK_MARGIN, \
            "step %d: a GraphPool top-k margin of %.2e in float64 (floor %.0e): the selection is not stable under fp32 round-off; pick " \
            "another seed" % (step, min(margins), TOPK_MARGIN)
        dl, dh = upstream(ro, rh, xr, y, 1.0)
        torch.autograd.backward([ro, rh], [dl, dh])
        # ---- product back-end on the GPU, the fused resstack.hip / graph.hip path
        xg = x.to(dev).requires_grad_(True)
        rs_before, gr_before = seen(resstack), seen(graph)
        out, hid = gpu(xg)
        key = (B, 42, T // 3)
        assert any(pl.key[:3] == key for pl in resstack._PLANS if (id(pl), pl.gen) not in rs_before), "resstack.hip did not run"
        assert any(pl.key == key for pl in graph._PLANS if (id(pl), pl.gen) not in gr_before), "graph.hip did not run"
        torch.autograd.backward([out, hid], [dl.float().to(dev), dh.float().to(dev)])
        torch.cuda.synchronize()
        print("\n[aasist B=%d T=%d %s step %d] min top-k margin %.2e; pre-activations within %.0e x RMS of a kink: %s"
              % (B, T, "train" if training else "eval", step, min(margins), KINK_REL, kinks))
        for name, g, r in (("logits", out, ro), ("hidden", hid, rh)):
            rep.check("out", name, rl2(g, r))
            rep.check("out-max", name, maxrel(g, r))
        rep.check("grad_x", "input", rl2(xg.grad, xr.grad))
        n = compare_params(rep, gparams, rparams, training, analytically_zero)
        assert n == sum(1 for p in rparams.values() if p.grad is not None)
        # every parameter has a gradient but the weight and bias of the five bn1 whose output Residual_block discards
        assert n == len(rparams) - 10, n
        compare_buffers(rep, gpu, ref, nbt0, step + 1 if training else 0)
        assert not training or all(v == nbt0[k] + step + 1 for k, v in batch_counts(gpu).items()), batch_counts(gpu)
        for p in list(gparams.values()) + list(rparams.values()):
            if p.grad is not None:
                p.grad.zero_()
    rep.done()


# ---- ResNet -----------------------------------------------------------------------------------------------------------------------------
RESNET_CASES = [(32, True), (32, False), (11, True), (11, False)]


@pytest.mark.parametrize("B,training", RESNET_CASES, ids=["%d-%s" % (B, "train" if t else "eval") for B, t in RESNET_CASES])
def test_resnet_backend_matches_float64_oracle(dev, monkeypatch, B, training):
    monkeypatch.delenv("SCL_RESNET_CONV", raising=False)
    assert resnet_head._conv_dtype() == torch.float32 and resnet_head.X3_BWD, "not the training default (f32 forward, bf16-pair backward)"
    T = 199
    gpu = ResNetHead(DEFAULT_RESNET).to(dev)
    sd = fill(gpu, seed=2000 + B)
    gpu.load_state_dict(sd)
    ref = ORH.ParamTree({k: tuple(v.shape) for k, v in sd.items()})
    ref.load_state_dict(sd)
    ref = ref.double()
    set_mode((gpu, ref), training)
    y = labels(B)
    nbt0 = batch_counts(ref)
    gparams, rparams = dict(gpu.named_parameters()), dict(ref.named_parameters())
    rep = Report("resnet B=%d %s" % (B, "train" if training else "eval"), BARS_RESNET[training])
    for step in range(2):
        rep.step = step
        x = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(104729 * step + B))
        xr = x.double().requires_grad_(True)
        kinks = {}
        with kink_counter(kinks):
            ro, re = ORH.forward(ref.tensors(), xr, training)
        dl, de = upstream(ro, re, xr, y, float(B))         # this plugin's Model.loss has no 1/bz (tests/test_resnet_gpu.py)
        torch.autograd.backward([ro, re], [dl, de])
        xg = x.to(dev).requires_grad_(True)
        out, emb = gpu(xg)
        torch.autograd.backward([out, emb], [dl.float().to(dev), de.float().to(dev)])
        torch.cuda.synchronize()
        print("\n[resnet B=%d %s step %d] pre-activations within %.0e x RMS of a kink: %s"
              % (B, "train" if training else "eval", step, KINK_REL, kinks))
        for name, g, r in (("logits", out, ro), ("emb", emb, re)):
            rep.check("out", name, rl2(g, r))
            rep.check("out-max", name, maxrel(g, r))
        rep.check("grad_x", "input", rl2(xg.grad, xr.grad))
        n = compare_params(rep, gparams, rparams, training)
        assert n == sum(1 for p in rparams.values() if p.grad is not None)
        assert n == len(rparams) - 2, n          # all but first_bn1 (defined, never used by the reference)
        compare_buffers(rep, gpu, ref, nbt0, step + 1 if training else 0)
        assert not training or batch_counts(gpu)["resnet.bn5.num_batches_tracked"] == step + 1
        for p in list(gparams.values()) + list(rparams.values()):
            if p.grad is not None:
                p.grad.zero_()
    rep.done()
