"""Training the ResNet back-end on zero-padded variable-length batches, the parts that need no GPU: the DEFINITION of the masked train-mode
network (tests/masked_train_cases.py::masked_train_forward, fp64, autograd) against oracle/resnet_head.forward in train mode where the two
must agree (every utterance of the padded batch has the same frame count) and against closed forms where they need not (ragged frames); the
closed-form references of the masked BatchNorm and the masked average against torch autograd on the compact tensors; the new entry points
refusing bad arguments before they touch a device."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import resnet_head as ORH
from scl_amd import lib
from scl_amd import resnet_head as RH
from tests import masked_train_cases as MC
from tests import nn_cases as NC

CFG = dict(RH.DEFAULT_RESNET, resnet_type="18")
RAGGED = [55, 56, 78, 79, 103]


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _clone_state(t):
    return {k: (v.detach().clone().requires_grad_(True) if v.requires_grad else v.clone()) for k, v in t.items()}


def _run(fn, t, feats, seed):
    """(logits, emb, {name: grad}, d_feats) of the scalar (logits * wl).sum() + (emb * we).sum()."""
    feats = feats.clone().requires_grad_(True)
    out, emb = fn(t, feats)
    wl, we = MC.loss_weights(feats.shape[0], seed)
    ((out * wl).sum() + (emb * we).sum()).backward()
    return out.detach(), emb.detach(), {k: v.grad for k, v in t.items() if v.requires_grad}, feats.grad


@pytest.mark.parametrize("width", [32])
def test_equal_frames_on_a_padded_batch_equal_the_oracle_in_train_mode_on_the_compact_batch(width):
    """Check (a): frames all n = 79 < T = 103, the padding of feats filled with junk of magnitude 1e6.  Logits, emb, every parameter gradient,
    d feats[:, :n] and the updated running statistics within 1e-12 relative (max |a - b| / max |b| per tensor) of
    oracle/resnet_head.forward(t, feats[:, :n], True); d feats beyond n exactly 0.  Measured: 1.1e-13 worst.
    resnet.bn1.bias is moved by +0.5: with fill_state's biases of ~0.05, bn1 -> ReLU -> layer1.0.bn1 is nearly invariant to bn1's scale, the
    gradient of resnet.bn1.weight is a cancellation to 3 % of its terms, and its relative error (1.6e-12 between torch's batch_norm and ANY
    other float64 spelling of it, with or without padding) measures float64 rounding, not the definition."""
    n, T, B = 79, 103, 4
    g = torch.Generator().manual_seed(21)
    base = MC.oracle_state(CFG, 5)
    with torch.no_grad():
        base["resnet.bn1.bias"] += 0.5
    clean = torch.randn(B, T, width, generator=g, dtype=torch.float64)
    feats = clean.clone()
    feats[:, n:] = 1e6 * torch.randn(B, T - n, width, generator=g, dtype=torch.float64)
    t_def, t_ref = _clone_state(base), _clone_state(base)
    out, emb, grads, dfe = _run(lambda t, f: MC.masked_train_forward(t, f, [n] * B), t_def, feats, 3)
    ro, re, rgrads, rdfe = _run(lambda t, f: ORH.forward(t, f, True), t_ref, clean[:, :n].contiguous(), 3)
    worst = max(_rel(out, ro), _rel(emb, re), _rel(dfe[:, :n], rdfe))
    assert (dfe[:, n:] == 0).all()
    for k, gr in rgrads.items():
        if k.startswith("first_bn1."):
            assert gr is None and grads[k] is None
            continue
        worst = max(worst, _rel(grads[k], gr))
    stats = [k for k in base if k.endswith(("running_mean", "running_var")) and not k.startswith("first_bn1.")]
    assert len(stats) == 2 * 19
    for k in stats:
        assert not torch.equal(t_ref[k], base[k])
        worst = max(worst, _rel(t_def[k], t_ref[k]))
    for k in base:
        if k.endswith("num_batches_tracked"):
            assert t_def[k].item() == t_ref[k].item() == (0 if k.startswith("first_bn1.") else 1)
    print("masked train definition against the oracle in train mode: worst relative difference %.2e" % worst)
    assert worst < 1e-12


def test_ragged_frames_statistics_are_those_of_the_valid_elements_and_the_padding_content_is_ignored():
    """Check (b): first_bn's mean / variance are the closed form over the concatenated valid elements of feats; two different junk fills of the
    padding give the same bits in every output, gradient and running statistic."""
    width, T, B = 16, max(RAGGED), len(RAGGED)
    g = torch.Generator().manual_seed(22)
    base = MC.oracle_state(CFG, 6)
    clean = torch.randn(B, T, width, generator=g, dtype=torch.float64) * 1.7 + 0.4
    results = []
    for fill in (1e6, -3e5):
        feats = clean.clone()
        for b, n in enumerate(RAGGED):
            feats[b, n:] = fill * torch.randn(T - n, width, generator=g, dtype=torch.float64)
        t, rec = _clone_state(base), {}
        results.append((_run(lambda tt, f: MC.masked_train_forward(tt, f, RAGGED, record=rec), t, feats, 4), t, rec))
    (out, emb, grads, dfe), t, rec = results[0]
    flat = torch.cat([clean[b, :n].reshape(-1) for b, n in enumerate(RAGGED)])
    mean, var, nv = rec["first_bn"]
    assert nv == flat.numel() == width * sum(RAGGED)
    assert abs(mean.item() - flat.mean().item()) < 1e-13 and abs(var.item() - flat.var(unbiased=False).item()) < 1e-13
    want_rv = 0.9 * base["first_bn.running_var"] + 0.1 * flat.var(unbiased=True)
    assert _rel(t["first_bn.running_var"], want_rv) < 1e-13
    assert rec["resnet.bn5"][2] == (width // 8) * sum(RH.batch_rows(RAGGED)[6])      # three stride-2 stages halve the width too
    for b, n in enumerate(RAGGED):
        assert (dfe[b, n:] == 0).all() and (dfe[b, :n] != 0).any()
    (out2, emb2, grads2, dfe2), t2, _ = results[1]
    assert torch.equal(out, out2) and torch.equal(emb, emb2) and torch.equal(dfe, dfe2)
    for k, gr in grads.items():
        assert (gr is None and grads2[k] is None) or torch.equal(gr, grads2[k]), k
    for k in t:
        if not t[k].requires_grad:
            assert torch.equal(t[k], t2[k]), k


@pytest.mark.parametrize("act", NC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
@pytest.mark.parametrize("case", MC.MASKED_BN_CASES, ids=lambda c: "B%d-H%d-W%d-C%d" % c[:4])
def test_masked_batch_norm_reference_is_torch_autograd_on_the_compact_tensor(case, act):
    """Check (c): the closed-form reference on the padded map (NaN in the padding) against F.batch_norm in train mode + the activation,
    differentiated by autograd, on the valid positions alone in float64."""
    B, H, W, C, valid = case
    inp = MC.masked_bn_inputs(B, H, W, C, valid, act)
    ref = MC.masked_bn_reference(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, valid, NC.BN_MOMENTUM, NC.BN_EPS, act, inp.dy)
    c = inp.compact
    x = c.x.double().requires_grad_(True)
    gm, bt = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    rm, rv = c.running_mean.double().clone(), c.running_var.double().clone()
    z = F.batch_norm(x, rm, rv, gm, bt, True, NC.BN_MOMENTUM, NC.BN_EPS)
    y = (z, torch.relu(z), torch.selu(z))[act]
    y.backward(c.dy.double())
    keep = MC.keep_rows(valid, H)
    assert ref.n_valid == x.shape[0] == W * sum(valid)
    worst = max(_rel(ref.y[keep].reshape(-1, C), y.detach()), _rel(ref.dx[keep].reshape(-1, C), x.grad), _rel(ref.dgamma, gm.grad),
                _rel(ref.dbeta, bt.grad), _rel(ref.running_mean, rm), _rel(ref.running_var, rv))
    print("masked BatchNorm reference against torch autograd: %.2e" % worst)
    assert worst < 1e-12
    assert (ref.y[~keep] == 0).all() and (ref.dx[~keep] == 0).all() and torch.isfinite(ref.y).all() and torch.isfinite(ref.dx).all()
    full = NC.bn_reference(c.x, c.gamma, c.beta, c.running_mean, c.running_var, True, NC.BN_MOMENTUM, NC.BN_EPS, act, c.dy)
    assert _rel(ref.sums, full.sums) < 1e-12 and _rel(ref.rstd, full.rstd) < 1e-12


def test_masked_average_reference_is_torch_autograd_on_each_slice():
    B, H, W, C, valid = MC.MASKED_AVG_CASE
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, H, W, C, generator=g)
    dy = torch.randn(B, C, generator=g)
    junk = x.clone()
    for b, v in enumerate(valid):
        junk[b, v:] = float("nan")
    y, dx = MC.masked_avg_reference(junk, valid, dy)
    for b, v in enumerate(valid):
        xs = x[b, :v].double().requires_grad_(True)
        ys = xs.mean((0, 1))
        ys.backward(dy[b].double())
        assert _rel(y[b], ys.detach()) < 1e-13 and _rel(dx[b, :v], xs.grad) < 1e-13 and (dx[b, v:] == 0).all()


def test_new_entry_points_refuse_null_and_bad_arguments_without_touching_the_gpu():
    """Check (d), after tests/test_resnet_varlen_cpu.py's test of the scoring entry points: a refused call never dereferences a device pointer."""
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    host = (ctypes.c_int32 * 2)(3, 1)
    none_valid = (ctypes.c_int32 * 2)(0, 0)
    fwd_args = (("x", p), ("B", 2), ("H", 3), ("W", 4), ("C", 16), ("gamma", p), ("beta", p), ("rm", p), ("rv", p), ("nbt", p), ("momentum", 0.1),
                ("eps", 1e-5), ("act", 1), ("valid", p), ("valid_host", host), ("part", p), ("mean", p), ("rstd", p), ("y", p), ("stream", None))
    fwd = lambda **kw: L.scl_bn_fwd_masked(*[kw.get(k, d) for k, d in fwd_args])
    for kw in (dict(x=None), dict(valid=None), dict(valid_host=None), dict(part=None), dict(mean=None), dict(rstd=None), dict(y=None)):
        assert fwd(**kw) == -1 and b"bn_fwd_masked" in L.scl_last_error(), kw
    for kw in (dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(C=0), dict(C=3), dict(C=1024), dict(act=3), dict(act=-1),
               dict(H=1 << 15, W=1 << 12)):      # H * W * C = 2^31
        assert fwd(**kw) == -1 and b"bn_fwd_masked" in L.scl_last_error(), kw
    assert fwd(x=odd) == -1 and b"16-byte" in L.scl_last_error()
    assert fwd(y=odd) == -1 and b"16-byte" in L.scl_last_error()
    assert fwd(valid_host=none_valid) == -1 and b"no valid position" in L.scl_last_error()

    bwd_args = (("dy", p), ("y", p), ("x", p), ("mean", p), ("rstd", p), ("gamma", p), ("B", 2), ("H", 3), ("W", 4), ("C", 16), ("act", 1),
                ("valid", p), ("valid_host", host), ("part", p), ("sums", p), ("dgamma", p), ("dbeta", p), ("dx", p), ("accumulate", 0),
                ("stream", None))
    bwd = lambda **kw: L.scl_bn_bwd_masked(*[kw.get(k, d) for k, d in bwd_args])
    for kw in (dict(dy=None), dict(x=None), dict(mean=None), dict(rstd=None), dict(valid=None), dict(valid_host=None), dict(part=None),
               dict(sums=None), dict(dx=None), dict(y=None)):      # y: the activation gradient needs it (act = 1)
        assert bwd(**kw) == -1 and b"bn_bwd_masked" in L.scl_last_error(), kw
    for kw in (dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(C=0), dict(C=3), dict(C=1024), dict(act=3), dict(act=-1),
               dict(H=1 << 15, W=1 << 12)):
        assert bwd(**kw) == -1 and b"bn_bwd_masked" in L.scl_last_error(), kw
    assert bwd(dx=odd) == -1 and b"16-byte" in L.scl_last_error()
    assert bwd(valid_host=none_valid) == -1 and b"no valid position" in L.scl_last_error()

    avg = lambda dy=p, valid=p, valid_host=host, B=2, H=3, W=4, C=256, dx=p: L.scl_avgpool_bwd_masked(dy, valid, valid_host, B, H, W, C, dx, None)
    for kw in (dict(dy=None), dict(valid=None), dict(valid_host=None), dict(dx=None), dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(C=0),
               dict(H=1 << 12, W=1 << 11), dict(valid_host=none_valid), dict(valid_host=(ctypes.c_int32 * 2)(3, 4)), dict(dx=odd)):
        assert avg(**kw) == -1 and b"avgpool_bwd_masked" in L.scl_last_error(), kw
    assert L.scl_bn_masked_nslabs(2, 300, 128) == 2 * 150 and L.scl_bn_masked_nslabs(3, 40, 16) == 3 * 5 and L.scl_bn_masked_nslabs(0, 1, 1) == 0
