"""Shared pieces of the layer-kernel tests of csrc/nn.hip and hipnn.linear / hipnn.bmm (CPU only, no scl_amd import): the case tables, input
builders with fixed seeds, and plain float64 references that share no formula with the kernels — BatchNorm + activation with its backward by
autograd, the row-map scatter of pad_nhwc as an index computation, the 3x3 max pool with the first-maximum rule through numpy's argmax.
tests/test_nn_cases_cpu.py pins the references against torch's own float64 operators at every case of the tables."""
from collections import namedtuple

import numpy as np
import torch

ACT_NONE, ACT_RELU, ACT_SELU = 0, 1, 2          # hipnn.ACT_*
ACTS = (ACT_NONE, ACT_RELU, ACT_SELU)
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_SELU: "selu"}

BN_SLAB = 128            # csrc/nn.hip: rows per statistics slab up to 65536 rows, 256 from 65537 on
BN_EPS, BN_MOMENTUM = 1e-5, 0.1

# (C, N): every reduction path and loop of slab_reduce / slab_reduce4 entered and left at its edge
BN_SHAPES = (
    [(C, N) for C in (1, 2) for N in (127, 128, 129, 300)]       # scalar path: a slab minus a row, exactly one, one plus a row, ragged third
    + [(C, N) for C in (4, 8, 16) for N in (129, 1000)]          # 16-byte path, tail loop only (a 128-row slab holds <= 2048 elements)
    + [(C, N) for C in (32, 64, 256) for N in (128, 385)]        # four-loads-in-flight loop entered (>= 4096 elements per slab)
    + [(512, 128), (512, 300)]                                   # two rows per trip
    + [(4, 65536), (4, 65537)]                                   # the slab size changes: 512 slabs of 128 rows / 257 of 256, the last with one row
    + [(16, 70000)]                                              # 256-row slabs with a ragged last slab
)
BN_NO_AFFINE_SHAPES = [(2, 129), (8, 1000), (64, 385), (512, 300)]       # gamma = beta = None, one per path
BN_EVAL_SHAPE = (64, 385)
BN_OFFSET_SHAPES = [(8, 8), (8, 189), (8, 4096)]                         # (C, N) with |mean| / std up to 16
BN_OFFSET_RATIOS = (16.0, -16.0, 8.0, -12.0, 4.0, -2.0, 1.0, 0.5)        # per channel, C = 8

# (B, H, W, C, bf16 destination, kind): kind "pad" = zero border of 1 around every map, "dilated" = the stride-2 data gradient's map (rows and
# columns doubled inside a border of 1), "base2" = "pad" shifted by 2 elements
PAD_CASES = [
    (3, 5, 7, 8, False, "pad"),          # 16-byte path
    (3, 5, 7, 6, False, "pad"),          # element path
    (3, 5, 7, 1, False, "pad"),          # element path: the encoder input map
    (3, 5, 7, 8, True, "pad"),           # element path, bf16 destination
    (3, 5, 7, 8, False, "dilated"),      # 16-byte path
    (3, 5, 7, 4, False, "base2"),        # offsets not all multiples of 4: the element path
    (2, 40, 33, 64, False, "pad"),       # 165 blocks of the 16-byte path
    (2, 1050, 1050, 1, False, "pad"),    # 2.2e6 elements: the 8192-block cap is reached, some threads of the element path make two trips
    (2, 730, 730, 8, False, "pad"),      # 2.13e6 vectors: the same for the 16-byte path
]
PAD_SLACK = 64           # destination elements behind the last map: they must stay untouched too

MAXPOOL_SHAPES = [(2, 7, 10), (3, 9, 9), (2, 128, 67)]
AVGPOOL_SHAPES = [(3, 1, 5), (2, 37, 257), (2, 700, 256)]
LINEAR_SHAPES = [          # M, K, N, leading dimensions of the 3-D form of x
    (7, 6, 2, (7, 1)),             # K and N padded to 8 / 4 and sliced; bias gradient by torch's column sum
    (32, 256, 2, (2, 16)),         # the ResNet back-end's fc
    (335, 64, 64, (5, 67)),        # odd M; split-K factor 2 over 335 rows (ragged)
    (4224, 64, 32, (4, 1056)),     # split-K factor 32
    (2691, 128, 128, (3, 897)),    # split-K factor 21, M = 21 * 128 + 3
    (300, 64, 12, (3, 100)),       # N % 8 != 0 with N > 4
]
BMM_SHAPES = [             # B, M, K, N, a passed as the transpose(1, 2) view of a [B, K, M] tensor
    (3, 42, 42, 64, False),
    (2, 66, 66, 32, False),
    (2, 67, 67, 64, False),
    (4, 1, 42, 64, True),          # aasist_head.py's attention-weighted sum
    (2, 5, 7, 3, False),
]


def linear_splitk(M, K, N):
    """hipnn._LinearFn.backward's split-K factor for the weight gradient (K and N already padded to multiples of 4)."""
    K, N = (K + 3) // 4 * 4, (N + 3) // 4 * 4
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    return max(1, min(32, 256 // tiles, M // 128))


def maxrel(got, ref):
    """The project's error measure: max |got - ref| / max |ref| over one tensor."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def maxabs(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return (got - ref).abs().max().item()


def _gen(*key):
    seed = 0x5C1
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---- BatchNorm + activation -----------------------------------------------------------------------------------------------------------
BNRef = namedtuple("BNRef", "y running_mean running_var dx dgamma dbeta mean rstd sums")


def _act64(act, z):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_SELU:
        return torch.selu(z)          # torch's own alpha / scale
    return z


def bn_reference(x, gamma, beta, running_mean, running_var, training, momentum, eps, act, dy):
    """BatchNorm over all rows of a channels-last x [N, C] followed by `act`, in float64: batch statistics (biased variance for y, unbiased
    for the running variance) when training, the running statistics otherwise.  gamma / beta may be None.  The backward comes from autograd
    on this float64 graph.  -> BNRef(y, new running mean, new running var, dx, dgamma, dbeta, mean, rstd, sums) with sums [2, C] =
    (sum dz, sum dz * xhat), dz the gradient at the activation's input; dgamma / dbeta are None where gamma / beta are."""
    x = x.detach().double().clone().requires_grad_(True)
    N, C = x.shape
    g = None if gamma is None else gamma.detach().double().clone().requires_grad_(True)
    b = None if beta is None else beta.detach().double().clone().requires_grad_(True)
    rm, rv = running_mean.detach().double(), running_var.detach().double()
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        with torch.no_grad():
            unb = var * N / (N - 1) if N > 1 else var
            new_rm, new_rv = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb
    else:
        mean, var, new_rm, new_rv = rm, rv, rm.clone(), rv.clone()
    rstd = (var + eps) ** -0.5
    xhat = (x - mean) * rstd
    z = xhat if g is None else xhat * g
    z = z if b is None else z + b
    z.retain_grad()
    y = _act64(act, z)
    y.backward(dy.detach().double())
    dz, xh = z.grad, xhat.detach()
    sums = torch.stack([dz.sum(0), (dz * xh).sum(0)])
    return BNRef(y.detach(), new_rm.detach(), new_rv.detach(), x.grad, None if g is None else g.grad, None if b is None else b.grad,
                 mean.detach(), rstd.detach(), sums)


def bn_preact64(x, gamma, beta, running_mean, running_var, training, eps):
    """The activation's input in float64 for float32 operands, as bn_reference forms it."""
    x = x.double()
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = running_mean.double(), running_var.double()
    z = (x - mean) * (var + eps) ** -0.5
    if gamma is not None:
        z = z * gamma.double()
    if beta is not None:
        z = z + beta.double()
    return z


BNInputs = namedtuple("BNInputs", "x gamma beta running_mean running_var nbt dy prior_dgamma prior_dbeta")


def bn_inputs(C, N, act, affine=True, training=True, ratios=None):
    """float32 operands of one BatchNorm case.  x has a per-channel standard deviation in [0.5, 2] and a mean of 0.25 - 0.75 of it (either
    sign), or `ratios[c]` standard deviations with `ratios`; gamma takes both signs; the running statistics, num_batches_tracked = 7 and the
    prior dgamma / dbeta hold earlier contents.  dy = randn + 0.5 + 0.3 xhat, so that neither of the two backward sums is a cancellation to
    ~0 whose relative error would measure the seed.
      SELU: channel 0 gets gamma = 6 and the beta that puts its smallest pre-activation at -20 (training, affine): y there is within an ulp
            of -scale * alpha, which is where a derivative taken from y = scale * alpha * (exp(z) - 1) is most exposed, and z < -17 is past
            the point where exp(z) - 1 rounds to -1.
      ReLU: no |pre-activation| below 1e-3 (float64, on the float32 operands): elements closer than 2e-3 are moved 6e-3 outwards and the
            statistics recomputed until none is left.  The kernel's float32 pre-activation is then ~1e-6 from the reference's and no mask
            sits on a rounding edge."""
    gen = _gen(C, N, act, affine, training, 0 if ratios is None else 1)
    sigma = 0.5 + 1.5 * torch.rand(C, generator=gen, dtype=torch.float64)
    if ratios is None:
        mu = (0.25 + 0.5 * torch.rand(C, generator=gen, dtype=torch.float64)) * sigma
        mu = mu * (1 - 2 * (torch.arange(C) % 2)).double()
    else:
        mu = torch.tensor(ratios, dtype=torch.float64)[:C] * sigma
    x = (torch.randn(N, C, generator=gen, dtype=torch.float64) * sigma + mu).float()
    gamma = beta = None
    if affine:
        gamma = ((0.5 + 1.5 * torch.rand(C, generator=gen)) * (1 - 2 * ((torch.arange(C) // 2) % 2)).float())
        beta = 0.5 * torch.randn(C, generator=gen)
    rmean = 0.5 * torch.randn(C, generator=gen)
    rvar = 0.5 + 1.5 * torch.rand(C, generator=gen)
    if act == ACT_SELU and affine and training:
        xd = x[:, 0].double()
        xh = (xd - xd.mean()) / (((xd - xd.mean()) ** 2).mean() + BN_EPS).sqrt()
        gamma[0] = 6.0
        beta[0] = float(-20.0 - 6.0 * xh.min().item())
    if act == ACT_RELU:
        for _ in range(32):
            z = bn_preact64(x, gamma, beta, rmean, rvar, training, BN_EPS)
            bad = z.abs() < 2e-3
            if not bool(bad.any()):
                break
            xd = x.double()
            var = ((xd - xd.mean(0)) ** 2).mean(0) if training else rvar.double()
            slope = (var + BN_EPS) ** -0.5 * (1.0 if gamma is None else gamma.double())
            away = torch.where(z >= 0, 1.0, -1.0) * torch.sign(slope) * 6e-3 / slope.abs()
            x = torch.where(bad, xd + away, xd).float()
        assert bn_preact64(x, gamma, beta, rmean, rvar, training, BN_EPS).abs().min().item() >= 1e-3
    xd = x.double()
    xh = (xd - xd.mean(0)) / (((xd - xd.mean(0)) ** 2).mean(0) + BN_EPS).sqrt()
    dy = (torch.randn(N, C, generator=gen, dtype=torch.float64) + 0.5 + 0.3 * xh).float()
    return BNInputs(x, gamma, beta, rmean, rvar, torch.tensor([7], dtype=torch.int64), dy, torch.randn(C, generator=gen), torch.randn(C, generator=gen))


def bn_formula_emulation(x, eps=BN_EPS):
    """The kernels' statistics formula on the CPU: squares rounded to float32, float64 sums, var = E[x^2] - m^2, mean and rstd stored as
    float32, xhat = (x - mean) * rstd in float32.  -> max |xhat - float64 xhat| / max |float64 xhat|: the envelope of that formula, which is
    sensitive to |mean| / std."""
    xd = x.double()
    N = x.shape[0]
    m = xd.sum(0) / N
    var = ((x * x).double().sum(0) / N - m * m).clamp_min(0.0)
    mean32, rstd32 = m.float(), ((var + eps) ** -0.5).float()
    got = (x - mean32) * rstd32
    ref = (xd - xd.mean(0)) * (((xd - xd.mean(0)) ** 2).mean(0) + eps) ** -0.5
    return maxrel(got, ref)


# ---- copy into padded / dilated maps ---------------------------------------------------------------------------------------------------
def pad_geometry(B, H, W, C, kind):
    """-> (rowmap (W, HW, bs, rs, cs, base) in elements, number of destination elements the maps span)."""
    if kind in ("pad", "base2"):
        Hp, Wp = H + 2, W + 2
        base = (Wp + 1) * C + (2 if kind == "base2" else 0)
        return (W, H * W, Hp * Wp * C, Wp * C, C, base), B * Hp * Wp * C + (2 if kind == "base2" else 0)
    if kind == "dilated":          # hipnn._Conv2dFn.backward's dyp for a 3x3 / stride-2 / pad-1 convolution whose output is [H, W]
        Hd, Wd = 2 * H + 2, 2 * W + 2
        return (W, H * W, Hd * Wd * C, 2 * Wd * C, 2 * C, (Wd + 1) * C), B * Hd * Wd * C
    raise ValueError(kind)


def pad_inputs(B, H, W, C, bf16, kind):
    """-> (src f32 [B * H * W, C], rowmap, destination pre-filled with a NaN-free random sentinel, PAD_SLACK elements longer than the maps)."""
    gen = _gen(B, H, W, C, bf16, len(kind))
    rowmap, span = pad_geometry(B, H, W, C, kind)
    src = torch.randn(B * H * W, C, generator=gen)
    dst = (torch.rand(span + PAD_SLACK, generator=gen) + 2.0).to(torch.bfloat16 if bf16 else torch.float32)
    return src, rowmap, dst


def pad_reference(src, C, rowmap, dst_before):
    """src [rows, C] scattered by the row map (W, HW, bs, rs, cs, base): row r = (b, i, j) with b = r // HW, i = (r % HW) // W, j = r % W
    goes to the elements base + b * bs + i * rs + j * cs + (0 .. C-1) of the flat destination, converted to its type; every other element
    keeps what it held.  Returns the whole destination."""
    W, HW, bs, rs, cs, base = rowmap
    rows = src.shape[0]
    r = np.arange(rows, dtype=np.int64)
    b, ij = r // HW, r % HW
    i, j = ij // W, ij % W
    off = base + b * bs + i * rs + j * cs
    idx = torch.from_numpy((off[:, None] + np.arange(C, dtype=np.int64)[None, :]).reshape(-1))
    assert idx.unique().numel() == idx.numel(), "row map sends two source elements to one place"
    out = dst_before.clone().view(-1)
    out[idx] = src.reshape(-1).to(out.dtype)
    return out


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------
def maxpool3_inputs(B, H, W, transposed):
    """x [B, H, W] f32 drawn from {-1, 0, 1} (most 3x3 windows hold ties) — contiguous, or the transpose(1, 2) view of a [B, W, H] tensor."""
    gen = _gen(B, H, W)
    x = torch.randint(-1, 2, (B, H, W), generator=gen).float()
    dy = torch.randn(B, H // 3, W // 3, generator=gen)
    if transposed:
        x = x.transpose(1, 2).contiguous().transpose(1, 2)
    return x, dy


def maxpool3_reference(x):
    """3x3 / stride-3 max pool of x [B, H, W] in floor mode, float64 -> (y [B, H//3, W//3], flat argmax h * W + w inside x[b], int64) with the
    FIRST maximum in row-major window order (numpy's argmax returns the first occurrence; a NaN counts as the maximum)."""
    B, H, W = x.shape
    OH, OW = H // 3, W // 3
    win = x.double()[:, :3 * OH, :3 * OW].reshape(B, OH, 3, OW, 3).permute(0, 1, 3, 2, 4).reshape(B, OH, OW, 9).numpy()
    k = torch.from_numpy(np.argmax(win, axis=-1))
    y = torch.from_numpy(np.take_along_axis(win, k.numpy()[..., None], axis=-1)[..., 0].copy())
    oh = torch.arange(OH).view(1, OH, 1)
    ow = torch.arange(OW).view(1, 1, OW)
    idx = (3 * oh + k // 3) * W + 3 * ow + k % 3
    return y, idx


def maxpool3_backward_reference(dy, idx, H, W):
    """dx [B, H, W] float64: dy scattered to the argmax of its window, exactly 0 elsewhere (windows do not overlap)."""
    B = dy.shape[0]
    dx = torch.zeros(B, H * W, dtype=torch.float64)
    dx.scatter_(1, idx.reshape(B, -1), dy.double().reshape(B, -1))
    return dx.view(B, H, W)


def avgpool_inputs(B, R, C):
    gen = _gen(B, R, C)
    return torch.randn(B, R, C, generator=gen) + 0.5, torch.randn(B, C, generator=gen)


def avgpool_reference(x, dy):
    """-> (mean over the rows of x [B, R, C], dx = dy / R on every row), float64."""
    B, R, C = x.shape
    return x.double().sum(1) / R, (dy.double() / R).view(B, 1, C).expand(B, R, C).contiguous()


# ---- Linear / bmm ------------------------------------------------------------------------------------------------------------------------
def linear_inputs(M, K, N):
    gen = _gen(M, K, N)
    return (torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) * K ** -0.5, torch.randn(N, generator=gen),
            torch.randn(M, N, generator=gen))


def linear_reference(x, w, b, dy):
    """-> (y, dx, dw, db or None) of y = x w^T + b in float64 by autograd; x [..., K]."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    y = xr @ wr.t()
    if br is not None:
        y = y + br
    y.backward(dy.double())
    return y.detach(), xr.grad, wr.grad, None if br is None else br.grad


def bmm_inputs(B, M, K, N, a_transposed):
    gen = _gen(B, M, K, N)
    a = torch.randn(B, K, M, generator=gen).transpose(1, 2) if a_transposed else torch.randn(B, M, K, generator=gen)
    return a, torch.randn(B, K, N, generator=gen), torch.randn(B, M, N, generator=gen)


def bmm_reference(a, b, dc):
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    c = torch.einsum("bmk,bkn->bmn", ar, br)
    c.backward(dc.double())
    return c.detach(), ar.grad, br.grad
