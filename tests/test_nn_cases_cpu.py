"""tests/nn_cases.py where there is no GPU: the float64 references of the layer-kernel tests against torch's own float64 operators at every
case of the tables (F.batch_norm + activation and its autograd backward, F.max_pool2d(return_indices=True), strided slicing for the
padded / dilated maps), the properties the input builders promise, and the envelope of the kernels' variance formula E[x^2] - m^2."""
import pytest
import torch
import torch.nn.functional as F

from tests import nn_cases as NC

TIGHT = 1e-11          # two float64 evaluations of the same quantity


def _torch_bn(inp, act, training):
    x = inp.x.double().requires_grad_(True)
    g = None if inp.gamma is None else inp.gamma.double().requires_grad_(True)
    b = None if inp.beta is None else inp.beta.double().requires_grad_(True)
    rm, rv = inp.running_mean.double().clone(), inp.running_var.double().clone()
    z = F.batch_norm(x, rm, rv, g, b, training, NC.BN_MOMENTUM, NC.BN_EPS)
    y = {NC.ACT_NONE: lambda t: t, NC.ACT_RELU: F.relu, NC.ACT_SELU: F.selu}[act](z)
    y.backward(inp.dy.double())
    return y.detach(), rm, rv, x.grad, None if g is None else g.grad, None if b is None else b.grad


def _check_bn(inp, act, training):
    ref = NC.bn_reference(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, training, NC.BN_MOMENTUM, NC.BN_EPS, act, inp.dy)
    y, rm, rv, dx, dg, db = _torch_bn(inp, act, training)
    assert NC.maxrel(ref.y, y) < TIGHT and NC.maxrel(ref.dx, dx) < 1e-9          # dx cancels two sums against dz
    assert NC.maxabs(ref.running_mean, rm) < TIGHT and NC.maxabs(ref.running_var, rv) < TIGHT
    if inp.gamma is None:
        assert ref.dgamma is None and ref.dbeta is None
    else:
        assert NC.maxrel(ref.dgamma, dg) < 1e-9 and NC.maxrel(ref.dbeta, db) < 1e-9
        assert NC.maxrel(ref.sums[0], db) < 1e-9 and NC.maxrel(ref.sums[1], dg) < 1e-9          # (sum dz, sum dz xhat) ARE dbeta and dgamma
    if not training:
        assert torch.equal(ref.running_mean, inp.running_mean.double()) and torch.equal(ref.running_var, inp.running_var.double())
        assert torch.equal(ref.mean, inp.running_mean.double())
    return ref


@pytest.mark.parametrize("act", NC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=lambda s: "C%d-N%d" % s)
def test_bn_reference_matches_torch_fp64(shape, act):
    C, N = shape
    inp = NC.bn_inputs(C, N, act)
    ref = _check_bn(inp, act, True)
    z = NC.bn_preact64(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, True, NC.BN_EPS)
    if act == NC.ACT_RELU:
        assert z.abs().min().item() >= 1e-3
        assert 0.05 < (ref.y > 0).double().mean().item() < 0.95          # both sides of the mask are populated
    if act == NC.ACT_SELU:
        assert abs(z.min().item() + 20.0) < 1e-3 and z.max().item() > 1.0          # the exp branch down to -20, and the linear branch


@pytest.mark.parametrize("act", NC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
@pytest.mark.parametrize("shape", NC.BN_NO_AFFINE_SHAPES, ids=lambda s: "C%d-N%d" % s)
def test_bn_reference_without_affine(shape, act):
    C, N = shape
    _check_bn(NC.bn_inputs(C, N, act, affine=False), act, True)


@pytest.mark.parametrize("act", NC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
def test_bn_reference_eval_mode(act):
    C, N = NC.BN_EVAL_SHAPE
    inp = NC.bn_inputs(C, N, act, training=False)
    ref = _check_bn(inp, act, False)
    if act == NC.ACT_NONE:          # dx = gamma * rstd * dz, nothing subtracted
        assert NC.maxrel(ref.dx, inp.dy.double() * inp.gamma.double() * ref.rstd) < TIGHT
    if act == NC.ACT_RELU:
        assert NC.bn_preact64(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, False, NC.BN_EPS).abs().min().item() >= 1e-3


@pytest.mark.parametrize("act", NC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
@pytest.mark.parametrize("shape", NC.BN_OFFSET_SHAPES, ids=lambda s: "C%d-N%d" % s)
def test_bn_reference_offset_inputs(shape, act):
    C, N = shape
    inp = NC.bn_inputs(C, N, act, ratios=NC.BN_OFFSET_RATIOS)
    xd = inp.x.double()
    ratio = (xd.mean(0) / xd.std(0, unbiased=False)).abs()
    assert 10.0 < ratio.max().item() < 40.0          # the builder's 16 sigma, as the sample of N rows realises it
    _check_bn(inp, act, True)


def test_variance_formula_envelope():
    """E[x^2] - m^2 with float32 squares and float64 sums, mean / rstd stored as float32: at |mean| / std = 16 the normalised values stay
    within a tenth of the GPU tests' 2e-5 at every tested N; the error grows with the square of the ratio (the figures are printed)."""
    for C, N in NC.BN_OFFSET_SHAPES:
        e = NC.bn_formula_emulation(NC.bn_inputs(C, N, NC.ACT_NONE, ratios=NC.BN_OFFSET_RATIOS).x)
        print("E[x^2]-m^2 emulation, ratio <= 16, N = %d: %.2e" % (N, e))
        assert e < 2e-6, (N, e)
    for r in (64.0, 256.0):
        e = NC.bn_formula_emulation(NC.bn_inputs(8, 8, NC.ACT_NONE, ratios=(r,) * 8).x)
        print("E[x^2]-m^2 emulation, ratio %g, N = 8: %.2e" % (r, e))


@pytest.mark.parametrize("case", NC.PAD_CASES, ids=lambda c: "B%d-H%d-W%d-C%d-%s-%s" % (c[0], c[1], c[2], c[3], "bf16" if c[4] else "f32", c[5]))
def test_pad_reference_matches_strided_slicing(case):
    B, H, W, C, bf16, kind = case
    src, rowmap, dst = NC.pad_inputs(*case)
    got = NC.pad_reference(src, C, rowmap, dst)
    want = dst.clone()
    s4 = src.view(B, H, W, C).to(dst.dtype)
    if kind == "dilated":
        want[:B * (2 * H + 2) * (2 * W + 2) * C].view(B, 2 * H + 2, 2 * W + 2, C)[:, 1:1 + 2 * H:2, 1:1 + 2 * W:2] = s4
    else:
        o = 2 if kind == "base2" else 0
        want[o:o + B * (H + 2) * (W + 2) * C].view(B, H + 2, W + 2, C)[:, 1:1 + H, 1:1 + W] = s4
    assert got.dtype == dst.dtype and torch.equal(got, want)
    assert torch.equal(got[-NC.PAD_SLACK:], dst[-NC.PAD_SLACK:]) and not torch.equal(got, dst)
    if kind == "pad":          # on a zero-filled destination the map is F.pad of the source
        z = NC.pad_reference(src, C, rowmap, torch.zeros_like(dst))[:-NC.PAD_SLACK].view(B, H + 2, W + 2, C)
        assert torch.equal(z, F.pad(s4, (0, 0, 1, 1, 1, 1)))


@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("shape", NC.MAXPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool3_reference_matches_torch(shape, transposed):
    B, H, W = shape
    x, dy = NC.maxpool3_inputs(B, H, W, transposed)
    assert x.is_contiguous() != transposed
    y, idx = NC.maxpool3_reference(x)
    xr = x.double().contiguous().requires_grad_(True)
    yt, it = F.max_pool2d(xr[:, None], 3, return_indices=True)
    assert torch.equal(y, yt[:, 0].detach()) and torch.equal(idx, it[:, 0])
    ties = (x.double()[:, :H // 3 * 3, :W // 3 * 3].reshape(B, H // 3, 3, W // 3, 3) == y[:, :, None, :, None]).sum((2, 4)) > 1
    assert ties.double().mean().item() > 0.5          # most windows hold their maximum more than once
    yt.backward(dy.double()[:, None])
    dx = NC.maxpool3_backward_reference(dy, idx, H, W)
    assert torch.equal(dx, xr.grad)
    assert dx[:, H // 3 * 3:].abs().sum().item() == 0 and dx[:, :, W // 3 * 3:].abs().sum().item() == 0


@pytest.mark.parametrize("shape", NC.AVGPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avgpool_reference_matches_torch(shape):
    x, dy = NC.avgpool_inputs(*shape)
    y, dx = NC.avgpool_reference(x, dy)
    xr = x.double().requires_grad_(True)
    yt = xr.mean(1)
    yt.backward(dy.double())
    assert NC.maxrel(y, yt.detach()) < TIGHT and NC.maxrel(dx, xr.grad) < TIGHT


def test_linear_and_bmm_tables():
    """The references against F.linear / torch.bmm in float64, and the split-K factors the table is built around."""
    assert [NC.linear_splitk(M, K, N) for M, K, N, _ in NC.LINEAR_SHAPES] == [1, 1, 2, 32, 21, 2]
    for M, K, N, lead in NC.LINEAR_SHAPES:
        assert lead[0] * lead[1] == M
        x, w, b, dy = NC.linear_inputs(M, K, N)
        for bias in (b, None):
            y, dx, dw, db = NC.linear_reference(x, w, bias, dy)
            assert NC.maxrel(y, F.linear(x.double(), w.double(), None if bias is None else bias.double())) < TIGHT
            assert NC.maxrel(dx, dy.double() @ w.double()) < TIGHT and NC.maxrel(dw, dy.double().t() @ x.double()) < TIGHT
            assert (db is None) == (bias is None) and (db is None or NC.maxrel(db, dy.double().sum(0)) < TIGHT)
    for B, M, K, N, tr in NC.BMM_SHAPES:
        a, b, dc = NC.bmm_inputs(B, M, K, N, tr)
        assert a.shape == (B, M, K) and a.is_contiguous() != (tr and M > 1 and K > 1)
        c, da, db = NC.bmm_reference(a, b, dc)
        assert NC.maxrel(c, torch.bmm(a.double(), b.double())) < TIGHT
        assert NC.maxrel(da, torch.bmm(dc.double(), b.double().transpose(1, 2))) < TIGHT
        assert NC.maxrel(db, torch.bmm(a.double().transpose(1, 2), dc.double())) < TIGHT
