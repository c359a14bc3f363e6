"""Dropout of the fused AASIST graph module (scl_amd/graph.py over csrc/graph.hip) with the reference's own probabilities, against the
fp64 oracle run through the SAME 19 masks, rebuilt on the host from the seeds (tests/graph_dropout_cases.py; numpy port of
csrc/common.h::hash_u32 in tests/attention_cases.py): outputs, both input gradients, every parameter gradient and the BatchNorm buffers, on
the recorded step and on two replayed plans, then eval mode; the two stand-alone drop kernels bit for bit; seeding; and the whole back-end
in train mode.  tests/test_graph_dropout_cpu.py shows on the reference alone that one mismatching mask at any single site moves a compared
gradient by more than 300 bars, and that the top-k scores of every case here are at least 2e-6 apart.

Bars, in tests/test_graph_gpu.py::close's measure (largest deviation over the reference tensor's largest magnitude): 2e-4 outputs and
input gradients, 5e-4 parameter gradients, 1e-5 buffers.  They are conditional: each test also runs the per-operation composition
(AasistHead.graph_unfused, the arm pinned to the reference's goldens) at p = 0 against the fp64 oracle on the same inputs, and where four
times that error exceeds a bar, four times the error is the bar of that tensor group for that shape (2 for the 1 / (1 - p) scale, 2 for
another summation order).  The fused kernels never enter the bar.  Measured values: each test's docstring and
profiles/graph_dropout.txt."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scl_amd import aasist_head as AH  # noqa: E402
from scl_amd import graph, ops  # noqa: E402
from scl_amd.graph import _SEED_NAMES  # noqa: E402
from tests import graph_dropout_cases as C  # noqa: E402
from tests.attention_cases import keep_scale  # noqa: E402
from tests.test_graph_gpu import _head  # noqa: E402

pytestmark = pytest.mark.gpu


def _stream():
    return graph._S()


# ---- a. the two stand-alone kernels of the first layers ------------------------------------------------------------------------------
SIZES = [(1, 255), (256, 257), (5 * 42 * 64, 5 * 66 * 64), (1023, 70001)]      # residues 1, 255, 0, 1, 128, 128, 255, 113 modulo the 256-thread block


@pytest.mark.parametrize("p", [0.2, 0.3, 0.0])
@pytest.mark.parametrize("n0,n1", SIZES)
def test_drop_kernels_apply_the_host_rebuilt_mask_exactly(dev, p, n0, n1):
    """scl_graph_drop: y == x * keep_scale(seed, n, p) bit for bit for both tensors of a launch, each with its own seed (p = 0: a copy);
    scl_graph_drop_bwd: de == (da + db) * keep_scale.  Nothing is written behind a tensor's end."""
    g = torch.Generator().manual_seed(n0 + n1)
    seeds = (0x1234567 + n0, 0x7654321 ^ n1)
    pad, mark = 300, -7.0
    xs = [torch.randn(n, generator=g) for n in (n0, n1)]
    das = [torch.randn(n, generator=g) for n in (n0, n1)]
    dbs = [torch.randn(n, generator=g) for n in (n0, n1)]
    ys = [torch.full((n + pad,), mark, device=dev) for n in (n0, n1)]
    des = [torch.full((n + pad,), mark, device=dev) for n in (n0, n1)]
    xd, dad, dbd = ([t.to(dev) for t in ts] for ts in (xs, das, dbs))
    ops._call("scl_graph_drop", xd[0].data_ptr(), ys[0].data_ptr(), n0, seeds[0], xd[1].data_ptr(), ys[1].data_ptr(), n1, seeds[1], p, _stream())
    ops._call("scl_graph_drop_bwd", dad[0].data_ptr(), dbd[0].data_ptr(), des[0].data_ptr(), n0, seeds[0],
              dad[1].data_ptr(), dbd[1].data_ptr(), des[1].data_ptr(), n1, seeds[1], p, _stream())
    torch.cuda.synchronize()
    for i, n in enumerate((n0, n1)):
        k = keep_scale(seeds[i], n, p)
        if p == 0.0:
            assert bool((k == 1).all())
        elif n >= 255:      # the other tensor's seed gives another mask
            assert not torch.equal(k, keep_scale(seeds[1 - i], n, p))
        assert torch.equal(ys[i][:n].cpu(), xs[i] * k), (i, n)
        assert torch.equal(des[i][:n].cpu(), (das[i] + dbs[i]) * k), (i, n)
        assert bool((ys[i][n:] == mark).all()) and bool((des[i][n:] == mark).all())


# ---- b. the fused module in train mode -----------------------------------------------------------------------------------------------
def _zero_grads(h):
    for p in h.parameters():
        if p.grad is not None:
            p.grad.zero_()      # in place: a new gradient tensor would make the plan record again instead of replaying


def _p0(h):
    h = copy.deepcopy(h)
    for m in h.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return h


def _gpu_step(h, fn, e_S, e_T, wl, wh, dev):
    _zero_grads(h)
    xs, xt = e_S.to(dev).requires_grad_(True), e_T.to(dev).requires_grad_(True)
    logits, hidden = fn(xs, xt)
    ((logits * wl.to(dev)).sum() + (hidden * wh.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), hidden=hidden.detach().clone(), deS=xs.grad.clone(), deT=xt.grad.clone(),
                grads={n: p.grad.clone() for n, p in h.named_parameters() if p.grad is not None})


def _errors(got, want, h, ref):
    """Largest error of each tensor group of one step against the reference's step."""
    ep, where, checked = C.param_errors(got["grads"], want["grads"])
    assert checked >= 110, checked      # the reference's 122 graph parameters but the 12 biases in front of a BatchNorm
    eb, _ = C.buffer_errors(dict(h.named_buffers()), dict(ref.named_buffers()))
    return {"out": max(C.relerr(got["logits"], want["logits"]), C.relerr(got["hidden"], want["hidden"])),
            "din": max(C.relerr(got["deS"], want["deS"]), C.relerr(got["deT"], want["deT"])), "param": ep, "buf": eb}, where


def _bars(floor):
    return {k: max(C.BARS[k], 4 * floor[k]) for k in C.BARS}


@pytest.mark.parametrize("B,nT", C.SHAPES)
def test_fused_graph_module_against_fp64_with_the_same_masks(dev, B, nT):
    """Three training steps on one head (steps 2 and 3 replay the plans step 1 recorded; fresh inputs and loss weights each step,
    gradients zeroed in place), then one eval call.  After each step the step's 19 masks are rebuilt from graph.seed's stream and the
    fp64 reference — BatchNorm buffers carried along — runs through them.  hidden is zero exactly where the reference's is: wherever the
    read-out mask is 0, and else only in a master column of which drop_way zeroed one branch (max(0, m) = 0 for m <= 0); a |max| or a
    mean over >= 8 nodes is never zero.

    Measured on an MI355X (profiles/graph_dropout.txt), largest error over the three steps, out / din / param / buf, against the bars
    2e-4 / 2e-4 / 5e-4 / 1e-5 — fused with masks, then the p = 0 per-operation arm:
      (2, 33)  8.5e-7 / 6.9e-7 / 1.2e-5 / 9.4e-8    5.1e-7 / 4.4e-7 / 2.8e-6 / 9.6e-8
      (3, 67)  5.6e-7 / 1.0e-6 / 3.3e-6 / 1.1e-7    4.9e-7 / 7.2e-7 / 2.7e-5 / 7.7e-8
      (5, 66)  6.2e-7 / 8.0e-7 / 7.2e-5 / 1.1e-7    8.8e-7 / 6.1e-7 / 7.4e-6 / 1.0e-7
      (2, 80)  4.8e-7 / 7.9e-7 / 3.5e-5 / 1.1e-7    5.6e-7 / 7.1e-7 / 4.4e-6 / 1.2e-7
    Four times the p = 0 arm's error stays below every bar, so no bar was raised; eval mode: 3.2e-7 .. 6.9e-7."""
    shape = (B, nT)
    graph._PLANS.clear()
    h = _head(C.HEAD_SEED[shape], dev, True, drop0=False)
    assert graph.supported(h, C.NS, nT)
    sd = {k: v.detach().cpu().clone() for k, v in h.state_dict().items()}
    h0 = _p0(h)                                   # the arm the bars rest on: per-operation composition, p = 0
    ref, ref0 = C.masked_reference(sd), C.masked_reference(sd, p=0.0)
    seeds = C.step_seeds(C.STREAM_SEED[shape], C.STEPS)
    graph.seed(C.STREAM_SEED[shape])
    errs, floors, recorded = [], [], None
    for step in range(C.STEPS):
        inputs = C.step_inputs(B, nT, step)
        got = _gpu_step(h, lambda a, b: graph.graph_module(a, b, h), *inputs, dev)
        pl = [p for p in graph._PLANS if p.key == (B, C.NS, nT)]
        assert len(pl) == 1 and pl[0].fwd_calls is not None and pl[0].bwd_calls is not None
        if step == 0:
            recorded = (pl[0].st, pl[0].fwd_calls, pl[0].bwd_calls)
        else:      # a replay: the same argument blocks and the same recorded calls, only patched
            assert pl[0].st is recorded[0] and pl[0].fwd_calls is recorded[1] and pl[0].bwd_calls is recorded[2]
        assert pl[0].seeds_used == seeds[step]
        want = C.ref_step(ref, seeds[step], *inputs)
        assert want["gap"] >= C.MIN_GAP, (step, want["gap"])
        e, where = _errors(got, want, h, ref)
        # the p = 0 arm on the same inputs
        got0 = _gpu_step(h0, lambda a, b: AH.AasistHead.graph_unfused(h0, a, b), *inputs, dev)
        want0 = C.ref_step(ref0, seeds[step], *inputs)
        f, _ = _errors(got0, want0, h0, ref0)
        print("graph_dropout B=%d nT=%d step %d  fused, masks on: %s (worst parameter %s)  |  per-operation, p=0: %s  |  top-k gap %.2e" % (
            B, nT, step + 1, " ".join("%s %.2e" % kv for kv in e.items()), where, " ".join("%s %.2e" % kv for kv in f.items()), want["gap"]))
        errs.append(e)
        floors.append(f)
        # the zeros of hidden
        m = want["masks"]
        zero, dropped = want["hidden"] == 0, m["drop"] == 0
        assert torch.equal(got["hidden"].cpu() == 0, zero), step
        extra = zero & ~dropped
        assert bool(zero[dropped].all()) and not bool(extra[:, :128].any())
        assert bool(((m["way_M0"] == 0) | (m["way_M1"] == 0)).view(B, 32)[extra[:, 128:]].all())
    floor = {k: max(f[k] for f in floors) for k in C.BARS}
    bars = _bars(floor)
    print("graph_dropout B=%d nT=%d bars: %s" % (B, nT, " ".join("%s %.2e" % kv for kv in bars.items())))
    for step, e in enumerate(errs):
        for k in C.BARS:
            assert e[k] < bars[k], (step + 1, k, e[k], bars[k])
    # eval mode on the same head: no masks, running statistics, repeatable
    inputs = C.step_inputs(B, nT, C.STEPS)
    h.eval(); ref.eval(); h0.eval(); ref0.eval()
    with torch.no_grad():
        want = C.ref_step(ref, seeds[-1], *inputs)
        want0 = C.ref_step(ref0, seeds[-1], *inputs)
        xs, xt = inputs[0].to(dev), inputs[1].to(dev)
        a = tuple(t.clone() for t in graph.graph_module(xs, xt, h))
        b = tuple(t.clone() for t in graph.graph_module(xs, xt, h))
        u = AH.AasistHead.graph_unfused(h0, xs, xt)
        torch.cuda.synchronize()
    assert want["gap"] >= C.MIN_GAP and want0["gap"] >= C.MIN_GAP
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    e = max(C.relerr(a[0], want["logits"]), C.relerr(a[1], want["hidden"]))
    f = max(C.relerr(u[0], want0["logits"]), C.relerr(u[1], want0["hidden"]))
    print("graph_dropout B=%d nT=%d eval  fused: out %.2e  |  per-operation: out %.2e  |  top-k gap %.2e" % (B, nT, e, f, want["gap"]))
    assert e < max(C.BARS["out"], 4 * f), (e, f)
    assert torch.equal(a[1].cpu() == 0, want["hidden"] == 0)      # no mask is left in the plan


# ---- c. seeding ----------------------------------------------------------------------------------------------------------------------
def test_reseeding_repeats_a_step_bit_for_bit(dev):
    B, nT = 2, 33
    graph._PLANS.clear()
    h = _head(C.HEAD_SEED[(B, nT)], dev, True, drop0=False)
    twin = copy.deepcopy(h)
    inputs = C.step_inputs(B, nT, 0)
    outs = []
    for head, v in ((h, 4242), (twin, 4242), (copy.deepcopy(twin), 4243)):
        graph.seed(v)
        outs.append(_gpu_step(head, lambda a, b: graph.graph_module(a, b, head), *inputs, dev))
    for k in ("logits", "hidden", "deS", "deT"):
        assert torch.equal(outs[0][k], outs[1][k]), k
        assert not torch.equal(outs[0][k], outs[2][k]), k
    assert all(torch.equal(g, outs[1]["grads"][n]) for n, g in outs[0]["grads"].items())


# ---- d. the whole back-end -----------------------------------------------------------------------------------------------------------
def test_whole_back_end_in_train_mode_against_fp64_with_the_same_masks(dev, monkeypatch):
    """AasistHead.forward on 3 clips of 99 frames (33 temporal nodes) in train mode against the oracle's full forward in fp64 through the
    same masks: logits, hidden, d feats and the gradients of pos_S, attention.0.weight and encoder.2.0.conv1.weight — the masked graph
    gradients reach the residual stack intact.  The bars' p = 0 arm is the same forward with the per-operation graph composition.
    Measured on an MI355X (profiles/graph_dropout.txt): out 1.1e-6, d feats 8.5e-7, parameters 1.8e-6; the p = 0 arm 9.3e-7, 3.4e-6,
    2.9e-6 — no bar raised."""
    c = C.BACKEND
    names = ("pos_S", "attention.0.weight", "encoder.2.0.conv1.weight")
    graph._PLANS.clear()
    h = _head(c["head_seed"], dev, True, drop0=False)
    sd = {k: v.detach().cpu().clone() for k, v in h.state_dict().items()}
    h0 = _p0(h)
    feats, wl, wh = C.backend_inputs()
    seeds = C.step_seeds(c["stream_seed"], 1)[0]

    def run(head):
        x = feats.to(dev).requires_grad_(True)
        logits, hidden = head(x)
        ((logits * wl.to(dev)).sum() + (hidden * wh.to(dev)).sum()).backward()
        torch.cuda.synchronize()
        params = dict(head.named_parameters())
        return dict(logits=logits.detach(), hidden=hidden.detach(), dfeats=x.grad, grads={n: params[n].grad for n in names})

    def errors(got, want):
        return {"out": max(C.relerr(got["logits"], want["logits"]), C.relerr(got["hidden"], want["hidden"])),
                "din": C.relerr(got["dfeats"], want["dfeats"]), "param": max(C.relerr(got["grads"][n], want["grads"][n]) for n in names)}

    assert AH.FUSED_GRAPH and graph.supported(h, C.NS, c["frames"] // 3)
    graph.seed(c["stream_seed"])
    got = run(h)
    assert [p.seeds_used for p in graph._PLANS] == [seeds]      # the fused graph module ran, on these seeds
    want = C.backend_step(C.masked_reference(sd), seeds, feats, wl, wh)
    assert want["gap"] >= C.MIN_GAP
    e = errors(got, want)
    monkeypatch.setattr(AH, "FUSED_GRAPH", False)
    got0 = run(h0)
    want0 = C.backend_step(C.masked_reference(sd, p=0.0), seeds, feats, wl, wh)
    f = errors(got0, want0)
    print("graph_dropout back-end B=%d frames=%d  fused, masks on: %s  |  per-operation graph, p=0: %s  |  top-k gap %.2e" % (
        c["B"], c["frames"], " ".join("%s %.2e" % kv for kv in e.items()), " ".join("%s %.2e" % kv for kv in f.items()), want["gap"]))
    for k in e:
        assert e[k] < max(C.BARS[k], 4 * f[k]), (k, e[k], f[k])
    assert sorted(_SEED_NAMES) == sorted(want["masks"])
