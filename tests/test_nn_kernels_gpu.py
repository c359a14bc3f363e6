"""The layer kernels of csrc/nn.hip (BatchNorm + activation forward / backward, the copy into padded maps, 3x3 max pool, average pool) and
hipnn.linear / hipnn.bmm, each against an independent float64 reference on the CPU (tests/nn_cases.py, pinned by tests/test_nn_cases_cpu.py)
at the smallest shapes that enter and leave every code path at its edge.  BatchNorm and pad_nhwc go through the C ABI (scl_amd.ops), the rest
through hipnn's autograd functions.

Error measure: max |got - ref| / max |ref| per tensor.  Bounds: 2e-5 for outputs and gradients, 1e-5 absolute for running statistics — the
ones tests/test_hipnn_gpu.py holds for exact-fp32 code.  Copies (pad_nhwc, the max pool and its backward) are compared bit for bit.
Every test prints its figures (`nn-err <kind> <value>`) before it asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import nn_cases as NC  # noqa: E402

TOL, TOL_STATS = 2e-5, 1e-5
ABS_KINDS = ("bn_running_mean", "bn_running_var")          # absolute error, bound TOL_STATS
_ACT_IDS = lambda a: NC.ACT_NAMES[a]          # noqa: E731
_CN_IDS = lambda s: "C%d-N%d" % s             # noqa: E731


@pytest.fixture(scope="module")
def dev():
    from scl_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _close(got, ref, kind, name, tol=TOL, failed=None):
    """Prints the figure, then asserts it — or, with `failed`, notes a miss there so that one wrong tensor does not hide the checks behind it."""
    err = NC.maxrel(got, ref) if kind not in ABS_KINDS else NC.maxabs(got, ref)
    print("nn-err %s %s %.3e" % (kind, name, err))
    if failed is None:
        assert err < tol, (kind, name, err)
    elif not err < tol:
        failed.append((kind, name, err))


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------------
def _check_bn(dev, inp, C, N, act, training):
    """scl_bn_fwd + scl_bn_bwd (plain and accumulating) on `inp` against bn_reference: y, mean, rstd, running mean / var,
    num_batches_tracked, dx, dgamma, dbeta, sums."""
    from scl_amd import ops
    ref = NC.bn_reference(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, training, NC.BN_MOMENTUM, NC.BN_EPS, act, inp.dy)
    up = lambda t: None if t is None else t.to(dev)          # noqa: E731
    x, gamma, beta, dy = up(inp.x), up(inp.gamma), up(inp.beta), up(inp.dy)
    rm, rv, nbt = up(inp.running_mean), up(inp.running_var), up(inp.nbt)
    nslab = ops.bn_nslabs(N)
    rows = NC.BN_SLAB if N <= NC.BN_SLAB * 512 else (((N + 511) // 512 + NC.BN_SLAB - 1) // NC.BN_SLAB) * NC.BN_SLAB
    assert nslab == (N + rows - 1) // rows
    part = torch.full((nslab * 2 * C,), float("nan"), dtype=torch.float64, device=dev)
    mean, rstd = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    y = torch.full((N, C), float("nan"), device=dev)
    ops.bn_fwd(x, N, C, gamma, beta, rm, rv, nbt, training, NC.BN_MOMENTUM, NC.BN_EPS, act, part, mean, rstd, y)
    tag = "C%d-N%d-%s" % (C, N, NC.ACT_NAMES[act])
    failed = []
    _close(y, ref.y, "bn_y", tag, failed=failed)
    _close(mean, ref.mean, "bn_mean", tag, failed=failed)
    _close(rstd, ref.rstd, "bn_rstd", tag, failed=failed)
    _close(rm, ref.running_mean, "bn_running_mean", tag, TOL_STATS, failed)
    _close(rv, ref.running_var, "bn_running_var", tag, TOL_STATS, failed)
    if training:
        assert nbt.item() == inp.nbt.item() + 1
    else:          # running statistics in, running statistics untouched
        assert torch.equal(rm.cpu(), inp.running_mean) and torch.equal(rv.cpu(), inp.running_var) and nbt.item() == inp.nbt.item()
        assert torch.equal(mean.cpu(), inp.running_mean)

    def backward(dg, db, accumulate):
        partb = torch.full_like(part, float("nan"))
        sums, dx = torch.full((2 * C,), float("nan"), device=dev), torch.full((N, C), float("nan"), device=dev)
        ops.bn_bwd(dy, y, x, mean, rstd, gamma, N, C, act, training, partb, sums, dg, db, dx, accumulate=accumulate)
        return sums, dx

    dg = None if gamma is None else torch.full((C,), float("nan"), device=dev)
    db = None if beta is None else torch.full((C,), float("nan"), device=dev)
    sums, dx = backward(dg, db, False)
    _close(dx, ref.dx, "bn_dx", tag, failed=failed)
    _close(sums.view(2, C), ref.sums, "bn_sums", tag, failed=failed)
    if gamma is not None:
        _close(dg, ref.dgamma, "bn_dgamma", tag, failed=failed)
        _close(db, ref.dbeta, "bn_dbeta", tag, failed=failed)
        ag, ab = up(inp.prior_dgamma), up(inp.prior_dbeta)          # earlier contents: the finishing kernel must ADD
        sums2, dx2 = backward(ag, ab, True)
        _close(ag, ref.dgamma + inp.prior_dgamma.double(), "bn_dgamma", tag + "-acc", failed=failed)
        _close(ab, ref.dbeta + inp.prior_dbeta.double(), "bn_dbeta", tag + "-acc", failed=failed)
        assert torch.equal(dx2, dx) and torch.equal(sums2, sums)
    assert not failed, failed
    return ref


@pytest.mark.parametrize("act", NC.ACTS, ids=_ACT_IDS)
@pytest.mark.parametrize("shape", NC.BN_SHAPES, ids=_CN_IDS)
def test_bn_train_forward_backward(dev, shape, act):
    """Train mode with gamma / beta and prior running statistics at the channel / row counts of NC.BN_SHAPES: the scalar and the 16-byte
    reduction, tail loop only and four-loads-in-flight loop, C = 512, and the change of slab size at 65536 rows.  SELU cases reach a
    pre-activation of -20, ReLU cases keep |pre-activation| >= 1e-3 (NC.bn_inputs)."""
    C, N = shape
    _check_bn(dev, NC.bn_inputs(C, N, act), C, N, act, True)


@pytest.mark.parametrize("act", NC.ACTS, ids=_ACT_IDS)
@pytest.mark.parametrize("shape", NC.BN_NO_AFFINE_SHAPES, ids=_CN_IDS)
def test_bn_train_without_gamma_and_beta(dev, shape, act):
    C, N = shape
    _check_bn(dev, NC.bn_inputs(C, N, act, affine=False), C, N, act, True)


@pytest.mark.parametrize("act", NC.ACTS, ids=_ACT_IDS)
def test_bn_eval_mode_both_directions(dev, act):
    """training = 0 in scl_bn_fwd and scl_bn_bwd: the running statistics normalise and stay as they were, dx = gamma * rstd * dz."""
    C, N = NC.BN_EVAL_SHAPE
    inp = NC.bn_inputs(C, N, act, training=False)
    ref = _check_bn(dev, inp, C, N, act, False)
    if act == NC.ACT_NONE:
        assert NC.maxrel(ref.dx, inp.dy.double() * inp.gamma.double() * ref.rstd) < 1e-11


@pytest.mark.parametrize("act", NC.ACTS, ids=_ACT_IDS)
@pytest.mark.parametrize("shape", NC.BN_OFFSET_SHAPES, ids=_CN_IDS)
def test_bn_train_offset_inputs(dev, shape, act):
    """Per-channel means of up to 16 standard deviations.  The kernels form the variance as E[x^2] - m^2 with the squares rounded to
    float32 before the float64 sum, which is sensitive to |mean| / std.  Known envelope of that formula, emulated on the CPU (float32
    squares, float64 sums, float32 apply) in units of the output scale: at a ratio of 16, <= 4e-7 (5.8e-7 / 2.7e-7 / 1.8e-7 on this
    file's N = 8 / 189 / 4096 inputs, NC.bn_formula_emulation), the same as torch's float32 CPU BatchNorm, so the 2e-5 bound keeps its
    margin here; at a ratio of 64 with N = 8, 3.4e-5 (2.1e-5 with this builder); at a ratio of 256, 1.3e-3 (4.7e-4).  Ratios beyond 16
    are outside what this test asks of the kernel."""
    C, N = shape
    _check_bn(dev, NC.bn_inputs(C, N, act, ratios=NC.BN_OFFSET_RATIOS), C, N, act, True)


# ---- pad_nhwc --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.PAD_CASES, ids=lambda c: "B%d-H%d-W%d-C%d-%s-%s" % (c[0], c[1], c[2], c[3], "bf16" if c[4] else "f32", c[5]))
def test_pad_nhwc_writes_the_interior_and_nothing_else(dev, case):
    """The whole destination, pre-filled with a random sentinel, bit-equal to the row-map scatter: interior = source (rounded to bf16 for a
    bf16 map), border, gaps of the dilated map and the elements behind the last map untouched — hipnn's pool of zero-filled staging maps
    relies on exactly that.  Grid: one thread per element (16-byte path: per four), capped at 8192 blocks of 256; only the two cases with
    more than 2^21 elements / vectors reach the cap and make a second trip of the grid-stride loop, every other case makes one."""
    from scl_amd import ops
    B, H, W, C, bf16, kind = case
    src, rowmap, dst = NC.pad_inputs(*case)
    want = NC.pad_reference(src, C, rowmap, dst)
    n = B * H * W * C
    vec = C % 4 == 0 and not bf16 and all(v % 4 == 0 for v in rowmap[2:])
    assert vec == (kind != "base2" and C % 4 == 0 and not bf16)
    assert ((n // 4 if vec else n) > 8192 * 256) == (H >= 730)
    got = dst.to(dev)
    ops.pad_nhwc(src.to(dev), B * H * W, C, got, rowmap)
    got = got.cpu()
    assert got.dtype == want.dtype
    assert torch.equal(got.view(torch.int16 if bf16 else torch.int32), want.view(torch.int16 if bf16 else torch.int32))
    if bf16:
        interior = got[:-NC.PAD_SLACK].view(B, H + 2, W + 2, C)[:, 1:1 + H, 1:1 + W]
        assert torch.equal(interior, src.view(B, H, W, C).to(torch.bfloat16))


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "transposed"])
@pytest.mark.parametrize("shape", NC.MAXPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_max_pool3_ties_strides_and_floor(dev, shape, transposed):
    """Inputs from {-1, 0, 1}: most windows hold ties, so y alone cannot tell the argmax rule — the saved index must be the FIRST maximum
    in row-major window order, for a contiguous map and for the transposed view the AASIST head passes; dx is dy scattered there and
    exactly 0 elsewhere, the rows / columns the floor drops included."""
    from scl_amd import hipnn
    B, H, W = shape
    x, dy = NC.maxpool3_inputs(B, H, W, transposed)
    y_ref, idx_ref = NC.maxpool3_reference(x)
    xd = x.to(dev)
    if transposed:
        xd = x.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
    assert xd.is_contiguous() != transposed
    xd.requires_grad_(True)
    y = hipnn.max_pool3(xd)
    idx = y.grad_fn.saved_tensors[0]
    assert torch.equal(y.detach().cpu().double(), y_ref)
    assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), idx_ref)
    y.backward(dy.to(dev))
    dx_ref = NC.maxpool3_backward_reference(dy, idx_ref, H, W)
    assert torch.equal(xd.grad.cpu().double(), dx_ref)
    OH, OW = H // 3, W // 3
    assert xd.grad[:, 3 * OH:].abs().sum().item() == 0 and xd.grad[:, :, 3 * OW:].abs().sum().item() == 0


def test_max_pool3_propagates_a_nan(dev):
    """One NaN in one window: y is NaN there (and the index points at it), every other output and index is what it was without it."""
    from scl_amd import hipnn
    B, H, W = NC.MAXPOOL_SHAPES[0]
    x, _ = NC.maxpool3_inputs(B, H, W, False)
    y0, idx0 = NC.maxpool3_reference(x)
    xn = x.clone()
    xn[1, 4, 5] = float("nan")          # window (oh, ow) = (1, 1) of map 1, its centre
    xd = xn.to(dev).requires_grad_(True)
    y = hipnn.max_pool3(xd)
    idx = y.grad_fn.saved_tensors[0].cpu().long()
    y = y.detach().cpu().double()
    hit = torch.zeros_like(y0, dtype=torch.bool)
    hit[1, 1, 1] = True
    assert torch.isnan(y[hit]).all() and idx[hit].item() == 4 * W + 5
    assert torch.equal(y[~hit], y0[~hit]) and torch.equal(idx[~hit], idx0[~hit])


@pytest.mark.parametrize("shape", NC.AVGPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_avg_pool_rows(dev, shape):
    from scl_amd import hipnn
    x, dy = NC.avgpool_inputs(*shape)
    y_ref, dx_ref = NC.avgpool_reference(x, dy)
    xd = x.to(dev).requires_grad_(True)
    y = hipnn.avg_pool_rows(xd)
    y.backward(dy.to(dev))
    tag = "x".join(map(str, shape))
    _close(y.detach(), y_ref, "avgpool_y", tag)
    _close(xd.grad, dx_ref, "avgpool_dx", tag)


# ---- Linear / bmm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", NC.LINEAR_SHAPES, ids=lambda s: "M%d-K%d-N%d" % s[:3])
def test_linear(dev, shape, bias, three_d):
    """y, dx, dW, db of hipnn.linear: K / N padded to multiples of 4 and sliced, the weight gradient's split-K factors 1, 2 (ragged), 21
    (ragged) and 32, the bias gradient through the HIP column sum (N % 8 == 0) and through torch's (otherwise)."""
    from scl_amd import hipnn
    M, K, N, lead = shape
    x, w, b, dy = NC.linear_inputs(M, K, N)
    if not bias:
        b = None
    if three_d:
        x, dy = x.view(*lead, K), dy.view(*lead, N)
    y_ref, dx_ref, dw_ref, db_ref = NC.linear_reference(x, w, b, dy)
    xd = x.to(dev).requires_grad_(True)
    wd = torch.nn.Parameter(w.to(dev))
    bd = None if b is None else torch.nn.Parameter(b.to(dev))
    y = hipnn.linear(xd, wd, bd)
    assert y.shape == y_ref.shape
    y.backward(dy.to(dev))
    tag = "M%d-K%d-N%d" % (M, K, N)
    _close(y.detach(), y_ref, "linear_y", tag)
    _close(xd.grad, dx_ref, "linear_dx", tag)
    _close(wd.grad, dw_ref, "linear_dw", tag)
    if b is not None:
        _close(bd.grad, db_ref, "linear_db", tag)


@pytest.mark.parametrize("shape", NC.BMM_SHAPES, ids=lambda s: "B%d-M%d-K%d-N%d%s" % (s[0], s[1], s[2], s[3], "-aT" if s[4] else ""))
def test_bmm(dev, shape):
    """c, da, db of hipnn.bmm with K and N zero-padded to multiples of 4 (42-, 66- and 67-node graphs) and a transposed view as `a`."""
    from scl_amd import hipnn
    B, M, K, N, tr = shape
    a, b, dc = NC.bmm_inputs(B, M, K, N, tr)
    c_ref, da_ref, db_ref = NC.bmm_reference(a, b, dc)
    ad = (a.transpose(1, 2).contiguous().to(dev).transpose(1, 2) if tr else a.to(dev)).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True)
    c = hipnn.bmm(ad, bd)
    assert c.shape == (B, M, N)
    c.backward(dc.to(dev))
    tag = "B%d-M%d-K%d-N%d" % (B, M, K, N)
    _close(c.detach(), c_ref, "bmm_c", tag)
    _close(ad.grad, da_ref, "bmm_da", tag)
    _close(bd.grad, db_ref, "bmm_db", tag)
