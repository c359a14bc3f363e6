"""float64 references for training on zero-padded variable-length batches (tests/test_resnet_varlen_train_cpu.py pins them, the GPU tests of
tests/test_resnet_varlen_train_gpu.py use them): the masked train-mode BatchNorm + activation and the masked average written out in closed
form on the padded map [B, H, W, C] (utterance b owns the rows h < valid[b]), and the DEFINITION of the masked train-mode ResNet back-end
on the oracle's state-dict names with autograd.  Nothing here imports product code except the row-count table resnet_head.batch_rows."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import nn_cases as NC

SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946

# (B, H, W, C, valid) of the kernel tests: every path of the masked kernels at its edge
#   C = 1 scalar path / C % 4 == 0 16-byte path / C = 512 (one block quad per 512 channels); an utterance without rows, with one row, full;
#   a valid region that ends inside a 128-row slab and utterances longer than a slab; more than 65536 rows of the padded batch, where
#   bn_slab_rows goes from 128 to 256 rows
MASKED_BN_CASES = [
    (4, 9, 16, 1, [0, 1, 5, 9]),
    (4, 9, 16, 16, [0, 1, 5, 9]),
    (4, 9, 16, 64, [0, 1, 5, 9]),
    (2, 5, 4, 512, [5, 2]),
    (3, 40, 16, 16, [40, 9, 33]),
    (2, 300, 128, 4, [300, 17]),
]
MASKED_AVG_CASE = (4, 7, 16, 256, [1, 2, 7, 4])


def keep_rows(valid, H):
    """bool [B, H]: row h belongs to utterance b."""
    return torch.arange(H)[None, :] < torch.as_tensor(valid)[:, None]


def _act_and_grad(act, z):
    """(act(z), act'(z)) in float64, written out (not torch's operators)."""
    if act == NC.ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z)), (z > 0).to(z.dtype)
    if act == NC.ACT_SELU:
        e = SELU_SCALE * SELU_ALPHA * torch.exp(z)
        return torch.where(z > 0, SELU_SCALE * z, e - SELU_SCALE * SELU_ALPHA), torch.where(z > 0, torch.full_like(z, SELU_SCALE), e)
    return z, torch.ones_like(z)


MaskedBNRef = namedtuple("MaskedBNRef", "y running_mean running_var dx dgamma dbeta mean rstd sums n_valid")


def masked_bn_reference(x, gamma, beta, running_mean, running_var, valid, momentum, eps, act, dy):
    """The issue's formulas in float64, closed form (no autograd): statistics over the N_v = W * sum valid positions, y and dx exactly 0
    beyond.  x / dy [B, H, W, C] may hold anything (NaN included) in the padding: it is selected away before any arithmetic."""
    B, H, W, C = x.shape
    keep = keep_rows(valid, H)[:, :, None, None].expand(B, H, W, C)
    zero = torch.zeros((), dtype=torch.float64)
    xv = torch.where(keep, x.double(), zero)
    dyv = torch.where(keep, dy.double(), zero)
    n = int(W * sum(valid))
    mean = xv.sum((0, 1, 2)) / n
    var = torch.where(keep, (xv - mean) ** 2, zero).sum((0, 1, 2)) / n
    unb = var * n / (n - 1) if n > 1 else var
    new_rm = (1 - momentum) * running_mean.double() + momentum * mean
    new_rv = (1 - momentum) * running_var.double() + momentum * unb
    rstd = (var + eps) ** -0.5
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    xhat = (xv - mean) * rstd
    yv, slope = _act_and_grad(act, xhat * g + b)
    y = torch.where(keep, yv, zero)
    dz = torch.where(keep, dyv * slope, zero)
    s0, s1 = dz.sum((0, 1, 2)), torch.where(keep, dz * xhat, zero).sum((0, 1, 2))
    dx = torch.where(keep, g * rstd * (dz - (s0 + xhat * s1) / n), zero)
    return MaskedBNRef(y, new_rm, new_rv, dx, None if gamma is None else s1, None if beta is None else s0, mean, rstd, torch.stack([s0, s1]), n)


MaskedBNInputs = namedtuple("MaskedBNInputs", "x gamma beta running_mean running_var nbt dy prior_dgamma prior_dbeta compact")


def masked_bn_inputs(B, H, W, C, valid, act, fill=float("nan")):
    """NC.bn_inputs on the N_v valid positions (its conditioning: no ReLU pre-activation on a rounding edge, SELU down to -20), scattered into
    the padded map in (b, h, w) order; the padding of x and dy holds `fill`.  compact: the BNInputs the valid positions came from."""
    n = W * sum(valid)
    inp = NC.bn_inputs(C, n, act)
    x, dy = torch.full((B, H, W, C), fill), torch.full((B, H, W, C), fill)
    o = 0
    for b, v in enumerate(valid):
        x[b, :v] = inp.x[o:o + v * W].view(v, W, C)
        dy[b, :v] = inp.dy[o:o + v * W].view(v, W, C)
        o += v * W
    return MaskedBNInputs(x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, inp.nbt.clone(), dy, inp.prior_dgamma, inp.prior_dbeta, inp)


def masked_avg_reference(x, valid, dy):
    """y[b] = mean over h < valid[b] and W; dx[b, h, w, c] = dy[b, c] / (valid[b] * W) for h < valid[b], 0 beyond.  float64."""
    B, H, W, C = x.shape
    keep = keep_rows(valid, H)[:, :, None, None].expand(B, H, W, C)
    zero = torch.zeros((), dtype=torch.float64)
    cnt = (torch.as_tensor(valid).double() * W)[:, None]
    y = torch.where(keep, x.double(), zero).sum((1, 2)) / cnt
    dx = torch.where(keep, (dy.double() / cnt)[:, None, None, :].expand(B, H, W, C), zero)
    return y, dx


# ---- the definition of the masked train-mode network ------------------------------------------------------------------------------------
def masked_train_forward(t, feats, frames, resnet_type="18", num_nodes=3, record=None):
    """tests/test_resnet_varlen_cpu.py::_masked_forward with every eval-mode BatchNorm replaced by batch statistics over the valid positions
    of its map (N_v = W * sum_b rows[level][b]): mean and biased variance there, the output 0 beyond by selection, the running statistics of
    `t` updated in place (momentum 0.1, unbiased variance N_v / (N_v - 1)), num_batches_tracked + 1.  t: {oracle state-dict name: tensor}
    (parameters may require grad: autograd differentiates this), feats [B, T, width].  record: a dict that receives (mean, biased variance,
    N_v) per BatchNorm name.  -> (logits, emb)."""
    from scl_amd import resnet_head as RH
    rows = torch.tensor(RH.batch_rows(frames, resnet_type, num_nodes))      # [levels, B]
    dt = feats.dtype
    zero = torch.zeros((), dtype=dt)

    def bn(x, name, level, act):      # x [B, C, H, W]
        keep = (torch.arange(x.shape[2])[None, :] < rows[level][:, None])[:, None, :, None].expand_as(x)
        n = int(rows[level].sum()) * x.shape[3]
        xv = torch.where(keep, x, zero)      # the padding is selected away before any arithmetic (and gets an exact 0 gradient)
        mean = xv.sum((0, 2, 3)) / n
        var = torch.where(keep, (xv - mean[None, :, None, None]) ** 2, zero).sum((0, 2, 3)) / n
        with torch.no_grad():
            unb = var * n / (n - 1) if n > 1 else var
            t[name + ".running_mean"].mul_(0.9).add_(0.1 * mean)
            t[name + ".running_var"].mul_(0.9).add_(0.1 * unb)
            t[name + ".num_batches_tracked"] += 1
        if record is not None:
            record[name] = (mean.detach(), var.detach(), n)
        z = (xv - mean[None, :, None, None]) * ((var + 1e-5) ** -0.5)[None, :, None, None] * t[name + ".weight"][None, :, None, None] \
            + t[name + ".bias"][None, :, None, None]
        return torch.where(keep, act(z), zero)

    x = bn(feats.unsqueeze(1), "first_bn", 0, F.selu)
    x = bn(F.conv2d(x, t["resnet.conv1.weight"], None, (3, 1), (1, 1)), "resnet.bn1", 1, F.relu)
    for s in (1, 2, 3, 4):
        j = 0
        while "resnet.layer%d.%d.bn1.weight" % (s, j) in t:
            p = "resnet.layer%d.%d." % (s, j)
            stride = 2 if (s > 1 and j == 0) else 1
            lin, lout = (s if j == 0 else s + 1), s + 1
            a = bn(x, p + "bn1", lin, F.relu)
            skip = F.conv2d(a, t[p + "shortcut.0.weight"], None, stride) if (p + "shortcut.0.weight") in t else x
            h = F.conv2d(a, t[p + "conv1.weight"], None, stride, 1)
            h = F.conv2d(bn(h, p + "bn2", lout, F.relu), t[p + "conv2.weight"], None, 1, 1)
            x = h + skip
            j += 1
    x = bn(F.conv2d(x, t["resnet.conv5.weight"], None, 1, (0, 1)), "resnet.bn5", 6, F.relu)
    emb = x.sum(dim=(2, 3)) / (rows[6][:, None] * x.shape[3]).to(dt)
    return F.linear(emb, t["resnet.fc.weight"], t["resnet.fc.bias"]), emb


def oracle_state(cfg, seed, dtype=torch.float64):
    """{name: tensor} of a ResNet back-end filled by oracle.aasist.fill_state; float parameters (not buffers) require grad."""
    from oracle.aasist import fill_state
    from scl_amd import resnet_head as RH
    head = RH.ResNetHead(cfg)
    params = {k for k, _ in head.named_parameters()}
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    out = {}
    for k, v in fill_state(shapes, seed=seed).items():
        tt = torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v)
        out[k] = tt.requires_grad_(True) if k in params and k.split(".")[0] != "first_bn1" else tt
    return out


def loss_weights(B, seed):
    """Fixed cotangents for (logits [B, 2], emb [B, 256]): the scalar the head tests differentiate is (logits * wl).sum() + (emb * we).sum()."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 2, generator=g, dtype=torch.float64), torch.randn(B, 256, generator=g, dtype=torch.float64) / 16
