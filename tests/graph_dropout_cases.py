"""Shared pieces of the AASIST graph-module dropout tests (CPU only): the fp64 reference of the graph module with every dropout site
replaced by a mask rebuilt on the host, the per-step seeds of scl_amd/graph.py, the cases of tests/test_graph_dropout_gpu.py and their
inputs, the top-k gap of the reference's GraphPools, and the error measure with its bars.

The mask contract: the keep-factor of an element is csrc/common.h::dropout_scale(site seed, i, p) with i the element's
row-major index in the tensor the site receives — [B, N, D] at an input_drop or a GraphPool.drop, [B, K, D] / [B, 1, D] at a drop_way call,
[B, 5 * D] at the read-out drop — and an element is kept iff u >= p.  The hash is tests/attention_cases.py's numpy port; nothing of
csrc/graph.hip's index arithmetic is restated here."""
import contextlib

import torch
from torch import nn

from oracle import aasist_head as OH
from scl_amd.graph import _SEED_NAMES
from tests.attention_cases import keep_scale

NS = 42                                                   # spectral nodes
SHAPES = [(2, 33), (3, 67), (5, 66), (2, 80)]             # (B, nT); (5, 66) is the 199-frame training clip, 80 the largest graph.supported takes
STEPS = 3                                                 # steps 2 and 3 replay the plans step 1 recorded
HEAD_SEED = {(2, 33): 21, (3, 67): 22, (5, 66): 23, (2, 80): 24}         # tests/test_graph_gpu.py::_head(seed, ...)
STREAM_SEED = {(2, 33): 1001, (3, 67): 1002, (5, 66): 1003, (2, 80): 1004}      # graph.seed(v) before the first step
BACKEND = dict(B=3, frames=99, head_seed=31, stream_seed=2001, input_seed=77)  # the whole back-end: nT = 33
MIN_GAP = 2e-6                                            # tests/test_aasist_varlen_gpu.py's precondition on the top-k scores
BARS = {"out": 2e-4, "din": 2e-4, "param": 5e-4, "buf": 1e-5}      # tests/test_graph_gpu.py's bars, in relerr's measure
BN_BIASES = ("proj_with_att.bias", "proj_without_att.bias")       # in front of a BatchNorm on batch statistics: true gradient 0


def site_of(name):
    """Seed name of scl_amd/graph.py -> (attribute path of the dropout module in the reference's head, the module's call index)."""
    kind, tag = name.split("_") if "_" in name else (name, "")
    if kind == "in":
        return ("GAT_layer_" + tag if tag in ("S", "T") else "HtrgGAT_layer_ST" + tag) + ".input_drop", 0
    if kind == "pool":
        return ("pool_" + tag if len(tag) == 1 else "pool_h" + tag) + ".drop", 0
    if kind == "way":      # one module, six calls: the T calls inside the branch loop (branch 0, branch 1), then s1, s2, m1, m2
        return "drop_way", "TSM".index(tag[0]) * 2 + int(tag[1])
    assert name == "drop", name
    return "drop", 0


def step_seeds(value, steps):
    """The seeds scl_amd/graph.py draws in `steps` training calls after graph.seed(value): its 31-bit LCG over _SEED_NAMES, in order."""
    s, out = int(value) & 0x7FFFFFFF, []
    for _ in range(steps):
        seeds = {}
        for n in _SEED_NAMES:
            s = (s * 1664525 + 1013904223) & 0x7FFFFFFF
            seeds[n] = s
        out.append(seeds)
    return out


class _Mask(torch.autograd.Function):
    """y = x * mask(forward seed); dx = dy * mask(backward seed).  The two seeds are one in normal use; the sensitivity test alone sets
    them apart.  The backward seed is read when the backward runs."""

    @staticmethod
    def forward(ctx, x, site, name):
        m = site.mask(site.fwd[name], x)
        site.masks[name] = m
        ctx.site, ctx.name, ctx.like = site, name, x.detach()
        return x * m

    @staticmethod
    def backward(ctx, g):
        site, name = ctx.site, ctx.name
        m = site.masks[name] if site.bwd[name] == site.fwd[name] else site.mask(site.bwd[name], ctx.like)
        return g * m, None, None


class MaskSite(nn.Module):
    """Stands where an nn.Dropout stood: call i of a step uses the seed named names[i]."""

    def __init__(self, p, names):
        super().__init__()
        self.p, self.names = float(p), list(names)
        self.fwd, self.bwd, self.masks, self.calls = {}, {}, {}, 0

    def mask(self, seed, x):
        return keep_scale(seed, x.numel(), self.p).view(x.shape).to(x.dtype)

    def forward(self, x):
        if not self.training:
            return x
        name = self.names[self.calls]
        self.calls += 1
        return _Mask.apply(x, self, name)


def masked_reference(state_dict, p=None):
    """oracle.aasist_head.AasistHead in fp64 and train mode with `state_dict` loaded and every dropout site a MaskSite of the site's own
    probability (p: one probability for all of them instead)."""
    ref = OH.AasistHead().double()
    own = ref.state_dict()
    ref.load_state_dict({k: v.detach().cpu().to(own[k].dtype) for k, v in state_dict.items()})
    calls = {}
    for n in _SEED_NAMES:
        path, i = site_of(n)
        calls.setdefault(path, {})[i] = n
    sites = []
    for path, by_call in calls.items():
        parent = ref
        *mods, attr = path.split(".")
        for m in mods:
            parent = getattr(parent, m)
        old = getattr(parent, attr)
        assert isinstance(old, nn.Dropout), path
        site = MaskSite(old.p if p is None else p, [by_call[i] for i in range(len(by_call))])
        setattr(parent, attr, site)
        sites.append(site)
    assert not any(isinstance(m, nn.Dropout) for m in ref.modules()) and sum(len(s.names) for s in sites) == len(_SEED_NAMES) == 19
    ref.__dict__["mask_sites"] = sites
    return ref.train()


def set_seeds(ref, seeds, bwd=None):
    for site in ref.mask_sites:
        site.fwd = {n: seeds[n] for n in site.names}
        site.bwd = {n: (bwd or seeds)[n] for n in site.names}
        site.masks, site.calls = {}, 0


def masks_of(ref):
    """The masks of the last step, by seed name."""
    out = {}
    for site in ref.mask_sites:
        out.update(site.masks)
    return out


@contextlib.contextmanager
def topk_gaps(ref):
    """While open, every GraphPool call of `ref` appends the smallest gap, over its utterances, between the last kept and the first
    dropped score — in fp64 and behind the pool's own mask (the scores are read from the pool's projection)."""
    gaps, hooks = [], []

    def watch(pool):
        def hook(mod, inp, out):
            s = torch.sigmoid(out.detach())[:, :, 0].sort(dim=1, descending=True)[0]
            keep = max(int(s.shape[1] * pool.k), 1)
            if keep < s.shape[1]:
                gaps.append(float((s[:, keep - 1] - s[:, keep]).min()))
        return pool.proj.register_forward_hook(hook)
    for m in ref.modules():
        if isinstance(m, OH.GraphPool):
            hooks.append(watch(m))
    try:
        yield gaps
    finally:
        for h in hooks:
            h.remove()


def head_state(seed):
    """The state dict of tests/test_graph_gpu.py::_head(seed, ...) (built on the CPU)."""
    from tests.test_graph_gpu import _head
    return {k: v.clone() for k, v in _head(seed, torch.device("cpu"), True, drop0=False).state_dict().items()}


def step_inputs(B, nT, step):
    """Fresh inputs and fresh loss weights of one step: e_S, e_T, the weights on logits and on hidden (fp32, CPU)."""
    g = torch.Generator().manual_seed((B * 100 + nT) * 10 + step)
    return (torch.randn(B, NS, 64, generator=g), torch.randn(B, nT, 64, generator=g), torch.randn(B, 2, generator=g), torch.randn(B, 160, generator=g))


def backend_inputs():
    c = BACKEND
    g = torch.Generator().manual_seed(c["input_seed"])
    return torch.randn(c["B"], c["frames"], 128, generator=g), torch.randn(c["B"], 2, generator=g), torch.randn(c["B"], 160, generator=g)


def ref_step(ref, seeds, e_S, e_T, wl, wh, bwd=None, retain=False):
    """One step of the reference's graph module: zeroed gradients, masks of `seeds`, loss = sum(logits * wl) + sum(hidden * wh).
    In eval mode (no masks) the backward is left out."""
    ref.zero_grad(set_to_none=True)
    set_seeds(ref, seeds, bwd)
    xs, xt = e_S.double().requires_grad_(ref.training), e_T.double().requires_grad_(ref.training)
    with topk_gaps(ref) as gaps:
        logits, hidden = ref.graph(xs, xt)
    out = dict(logits=logits.detach(), hidden=hidden.detach(), gap=min(gaps), masks=masks_of(ref))
    if ref.training:
        loss = (logits * wl.double()).sum() + (hidden * wh.double()).sum()
        loss.backward(retain_graph=retain)
        out.update(deS=xs.grad.clone(), deT=xt.grad.clone(), grads={n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None},
                   loss=loss, leaves=(xs, xt))
    return out


def backend_step(ref, seeds, feats, wl, wh):
    """ref_step for the whole back-end: feats [B, T, 128] -> the reference's full forward with the masks of `seeds`."""
    ref.zero_grad(set_to_none=True)
    set_seeds(ref, seeds)
    x = feats.double().requires_grad_(True)
    with topk_gaps(ref) as gaps:
        logits, hidden = ref(x)
    ((logits * wl.double()).sum() + (hidden * wh.double()).sum()).backward()
    return dict(logits=logits.detach(), hidden=hidden.detach(), gap=min(gaps), masks=masks_of(ref), dfeats=x.grad.clone(),
                grads={n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None})


def relerr(got, want):
    """tests/test_graph_gpu.py::close's measure: the largest deviation over the largest magnitude of the reference tensor."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-9))


def param_errors(got, want):
    """Parameter gradients `got` (name -> tensor) against the reference's `want`: (largest relerr, its name, tensors compared).  The two
    biases in front of a BatchNorm on batch statistics have a true gradient of 0: there both sides must be round-off of the weight's
    gradient, as in tests/test_graph_gpu.py, and they are not counted."""
    worst, where, checked = 0.0, None, 0
    for n, w in want.items():
        assert got.get(n) is not None, n
        if n.endswith(BN_BIASES):
            wmax = float(want[n.replace(".bias", ".weight")].abs().max())
            assert float(got[n].abs().max()) < 1e-4 * wmax and float(w.abs().max()) < 1e-4 * wmax, n
            continue
        e = relerr(got[n], w)
        if e >= worst:
            worst, where = e, n
        checked += 1
    return worst, where, checked


def buffer_errors(got, want):
    """BatchNorm buffers of the graph layers: (largest relerr over the floating-point ones, its name); the step counts must be equal."""
    worst, where, seen = 0.0, None, 0
    for n, b in want.items():
        if not n.startswith(("GAT_", "HtrgGAT_")):
            continue
        if b.dtype.is_floating_point:
            e = relerr(got[n], b)
            if e >= worst:
                worst, where = e, n
        else:
            assert int(got[n]) == int(b), (n, int(got[n]), int(b))
        seen += 1
    assert seen == 18, seen      # six layers: running_mean, running_var, num_batches_tracked
    return worst, where
