"""`wav2vec2_resnet_nll` back-end on HIP kernels, channels-last.

What the reference computes (model/wav2vec2_resnet_nll.py:51-74 glue, model/resnet.py:47-191 network): the LL features as a one-channel
[bz, 1, T, 128] map -> BatchNorm2d(1) -> SELU -> conv 9x3 / stride (3,1) -> BN -> ReLU -> four stages of pre-activation blocks
(64 / 128 / 256 / 512 channels, strides 1 / 2 / 2 / 2) -> conv (num_nodes x 3) -> BN -> ReLU -> global average -> 256-d embedding ->
Linear -> 2 raw logits.  Here the map lives as [bz, T, 128, C] (channels last) from start to end; every convolution is an implicit
GEMM on the matrix cores (hipnn.conv2d: the exact-fp32 kernel by default — the reference's precision; `SCL_RESNET_CONV=bf16` selects
bf16 operands with fp32 accumulation: forward within 1.5e-2 of the reference on tests/golden/resnet.npz, but the gradients of the
early layers come out 10-28 % off there, so it stays opt-in), every BatchNorm + activation one fused HIP kernel pair (hipnn.batch_norm), pooling / Linear likewise.  Modules here are
parameter and buffer CONTAINERS named like the reference's state dict (resnet.layer2.0.shortcut.0.weight, ...), so its checkpoints
load; none of their torch forwards is ever called.

Variable-length batches (ResNetHead.forward(feats, frames)).  Scoring, eval mode under torch.no_grad(): only the time axis H shrinks through the
network, so an utterance of T frames owns the first layer_rows(T) rows of every map.  In eval mode a BatchNorm is a per-element map and every
convolution but conv5 reads BatchNorm outputs only: each BatchNorm + activation that feeds a convolution writes exact zeros (selected, not
multiplied) at and beyond the utterance's own row count — what the convolution's zero border holds for the utterance alone — and the
average runs over the utterance's own conv5 rows.  Training, train mode with autograd on: the same masks, with every
BatchNorm's batch statistics, running-statistics update and backward sums taken over the valid positions only (scl_bn_fwd_masked /
scl_bn_bwd_masked) and the masked average differentiated; every convolution's output gradient is then zero at the padded rows, so the weight
gradients sum valid positions only.  Basic-block networks only.

Reference details kept: a block's shortcut convolution reads the block's BN+ReLU output (resnet.py:64-66); `_make_layer` builds a
`downsample` module that is swallowed by *args and never registered (resnet.py:150-157) — no such keys here either; first_bn1 is
defined and unused (wav2vec2_resnet_nll.py:38).
"""
import math
import os

import torch
from torch import nn

from . import hipnn

DEFAULT_RESNET = {"num_nodes": 3, "enc_dim": 256, "resnet_type": "18", "nclasses": 2}
# (blocks per stage, bottleneck?) per resnet_type — model/resnet.py:116-120
STAGES = {"18": ((2, 2, 2, 2), False), "28": ((3, 4, 6, 3), False), "34": ((3, 4, 6, 3), False), "50": ((3, 4, 6, 3), True),
          "101": ((3, 4, 23, 3), True)}


# backward products of the convolutions in the bf16-pair form of the f32 kernel (hipnn.conv2d x3_bwd: 43.5 -> 40.5 ms per step at batch 32,
# the reference goldens' gradient bounds unchanged); SCL_RESNET_X3BWD=0: exact f32 products in the backward too
X3_BWD = os.environ.get("SCL_RESNET_X3BWD", "1") != "0"


def _conv_dtype():
    return torch.bfloat16 if os.environ.get("SCL_RESNET_CONV", "f32") == "bf16" else torch.float32


class ConvWeight(nn.Module):
    """Holds `weight` [Co, Ci, kh, kw] (and optionally `bias`) under nn.Conv2d's state-dict names and default initialisation."""

    def __init__(self, cin, cout, kernel, stride=(1, 1), padding=(0, 0), bias=False):
        super().__init__()
        kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
        self.stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
        self.padding = (padding, padding) if isinstance(padding, int) else tuple(padding)
        self.weight = nn.Parameter(torch.empty(cout, cin, kh, kw))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(cin * kh * kw)
            self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        else:
            self.bias = None

    def conv(self, x, dtype, residual=None, pooled=True):
        """x [B, H, W, Ci] channels-last -> [B, OH, OW, Co] (+ residual, the block's skip connection, in the GEMM epilogue).
        pooled=False: a variable-length scoring batch, whose staging map is not kept per geometry (hipnn.conv2d)."""
        return hipnn.conv2d(x, self.weight, self.bias, self.stride, self.padding, dtype, x3_bwd=X3_BWD, grad_in_place=True, residual=residual,
                            pooled=pooled)


class _Shortcut(nn.Module):
    """`shortcut.0.weight`: the 1x1 (strided) projection of a block whose shape changes."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.add_module("0", ConvWeight(cin, cout, 1, stride))


class PreActBlock(nn.Module):
    """out = conv2(relu(bn2(conv1(a)))) + (shortcut(a) or x), a = relu(bn1(x))     (resnet.py:47-70)."""
    expansion = 1

    def __init__(self, cin, planes, stride):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = ConvWeight(cin, planes, 3, stride, 1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = ConvWeight(planes, planes, 3, 1, 1)
        if stride != 1 or cin != planes:
            self.shortcut = _Shortcut(cin, planes, stride)

    def run(self, x, dt, vin=None, vout=None, pooled=None):
        """vin / vout: valid rows per utterance of the block's input / output map as (int32 [B] on the GPU, the same counts on the host), or
        None for a fixed-length batch.  pooled: whether the convolutions keep their staging maps per geometry (default: fixed-length only)."""
        pooled = vin is None if pooled is None else pooled
        (vi, ci), (vo, co) = vin or (None, None), vout or (None, None)
        a = hipnn.batch_norm(x, self.bn1, hipnn.ACT_RELU, grad_in_place=True, valid=vi, counts=ci)
        skip = getattr(self.shortcut, "0").conv(a, dt, pooled=pooled) if hasattr(self, "shortcut") else x
        h = hipnn.batch_norm(self.conv1.conv(a, dt, pooled=pooled), self.bn2, hipnn.ACT_RELU, grad_in_place=True, valid=vo, counts=co)
        return self.conv2.conv(h, dt, residual=skip, pooled=pooled)


class PreActBottleneck(nn.Module):
    """1x1 -> 3x3 (strided) -> 1x1 (x4) pre-activation bottleneck (resnet.py:73-101)."""
    expansion = 4

    def __init__(self, cin, planes, stride):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = ConvWeight(cin, planes, 1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv2 = ConvWeight(planes, planes, 3, stride, 1)
        self.bn3 = nn.BatchNorm2d(planes)
        self.conv3 = ConvWeight(planes, 4 * planes, 1)
        if stride != 1 or cin != 4 * planes:
            self.shortcut = _Shortcut(cin, 4 * planes, stride)

    def run(self, x, dt, vin=None, vout=None, pooled=None):
        """vin / vout as PreActBlock.run's: bn2 sits behind the 1x1 conv1 (input rows), bn3 behind the strided conv2 (output rows)."""
        pooled = vin is None if pooled is None else pooled
        (vi, ci), (vo, co) = vin or (None, None), vout or (None, None)
        a = hipnn.batch_norm(x, self.bn1, hipnn.ACT_RELU, grad_in_place=True, valid=vi, counts=ci)
        skip = getattr(self.shortcut, "0").conv(a, dt, pooled=pooled) if hasattr(self, "shortcut") else x
        h = hipnn.batch_norm(self.conv1.conv(a, dt, pooled=pooled), self.bn2, hipnn.ACT_RELU, grad_in_place=True, valid=vi, counts=ci)
        h = hipnn.batch_norm(self.conv2.conv(h, dt, pooled=pooled), self.bn3, hipnn.ACT_RELU, grad_in_place=True, valid=vo, counts=co)
        return self.conv3.conv(h, dt, residual=skip, pooled=pooled)


class _Stage(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        for i, b in enumerate(blocks):
            self.add_module(str(i), b)


class ResNet(nn.Module):
    def __init__(self, num_nodes=3, enc_dim=256, resnet_type="18", nclasses=2):
        super().__init__()
        counts, bottleneck = STAGES[str(resnet_type)]
        block = PreActBottleneck if bottleneck else PreActBlock
        self.conv1 = ConvWeight(1, 16, (9, 3), (3, 1), (1, 1))
        self.bn1 = nn.BatchNorm2d(16)
        cin = 16
        for s, (planes, n, stride) in enumerate(zip((64, 128, 256, 512), counts, (1, 2, 2, 2)), start=1):
            blocks = []
            for j in range(n):
                blocks.append(block(cin, planes, stride if j == 0 else 1))
                cin = planes * block.expansion
            self.add_module("layer%d" % s, _Stage(blocks))
        self.num_nodes, self.resnet_type = int(num_nodes), str(resnet_type)
        self.conv5 = ConvWeight(cin, 256, (num_nodes, 3), (1, 1), (0, 1))
        self.bn5 = nn.BatchNorm2d(256)
        self.fc = nn.Linear(256, nclasses)          # container for fc.weight / fc.bias

    def run(self, x, dt, rows=None, counts=None, pooled=None):
        """x [bz, T, 128, 1] -> (logits [bz, nclasses], emb [bz, 256]).
        rows: int32 [N_LEVELS, bz] on the GPU, layer_rows() of every utterance of a zero-padded variable-length batch (level 0, the frames, is
        the caller's: x is masked already), and counts: the same table on the host; None for a fixed-length batch.
        pooled: the convolutions' staging maps stay in the per-geometry pool — fixed-length batches and padded TRAINING batches (one padded
        shape per run); a scoring batch, whose every padded length is a geometry of its own, leaves it off."""
        lv = (lambda i: None) if rows is None else (lambda i: (rows[i], None if counts is None else counts[i]))
        pooled = rows is None if pooled is None else pooled
        v1 = lv(1) or (None, None)
        x = hipnn.batch_norm(self.conv1.conv(x, dt, pooled=pooled), self.bn1, hipnn.ACT_RELU, grad_in_place=True, valid=v1[0], counts=v1[1])
        for s in (1, 2, 3, 4):
            for j, blk in enumerate(getattr(self, "layer%d" % s).children()):
                x = blk.run(x, dt, lv(s if j == 0 else s + 1), lv(s + 1), pooled)      # a stage's first block takes the map of the stage before
        v6 = lv(6) or (None, None)
        x = hipnn.batch_norm(self.conv5.conv(x, dt, pooled=pooled), self.bn5, hipnn.ACT_RELU, grad_in_place=True, valid=v6[0], counts=v6[1])          # [bz, H', W', 256]
        if rows is None:
            emb = hipnn.avg_pool_rows(x.reshape(x.shape[0], -1, x.shape[-1]))
        else:
            emb = hipnn.avg_pool_rows_masked(x, rows[6], v6[1])
        return hipnn.linear(emb, self.fc.weight, self.fc.bias), emb


N_LEVELS = 7      # frames, conv1, layer1 .. layer4, conv5
_STAGE_STRIDES = (1, 2, 2, 2)


def layer_rows(frames, resnet_type="18", num_nodes=3):
    """Rows (the time axis) of every map of the network for an utterance of `frames` LL frames: [frames, conv1, layer1, layer2, layer3, layer4,
    conv5].  conv1 is 9 tall with stride 3 and padding 1; a stage's first block is 3 tall with its stage's stride and padding 1 (the 1x1
    strided shortcut gives the same count), every other convolution of a stage keeps the rows — whatever the block kind and the block
    counts, so `resnet_type` only has to name a network; conv5 is num_nodes tall without padding.  The last count is < 1 for an utterance
    the network cannot take."""
    if str(resnet_type) not in STAGES:
        raise ValueError("resnet_type %r: one of %s" % (resnet_type, sorted(STAGES)))
    t = int(frames)
    h = (t + 2 - 9) // 3 + 1 if t >= 7 else 0
    out = [t, h]
    for stride in _STAGE_STRIDES:
        h = (h - 1) // stride + 1 if h >= 1 else 0
        out.append(h)
    out.append(h - int(num_nodes) + 1)
    return out


def min_frames(resnet_type="18", num_nodes=3):
    """The fewest LL frames that leave conv5 an output row (55 for num_nodes 3): the row counts never decrease with the frames."""
    t = 7
    while layer_rows(t, resnet_type, num_nodes)[-1] < 1:
        t += 1
    return t


def batch_rows(frames, resnet_type="18", num_nodes=3):
    """Host-side frame counts of a batch -> [N_LEVELS][B] row counts (one small int32 upload holds them all).  ValueError below min_frames."""
    lo = min_frames(resnet_type, num_nodes)
    frames = [int(t) for t in frames]
    if not frames or min(frames) < lo:
        raise ValueError("ResNet back-end: every utterance needs at least %d frames (conv5 has no output row below), got %r" % (lo, frames))
    per = [layer_rows(t, resnet_type, num_nodes) for t in frames]
    return [[p[i] for p in per] for i in range(N_LEVELS)]


class ResNetHead(nn.Module):
    """feats [bz, T, 128] (LL output) -> (logits [bz, nclasses], emb [bz, 256])."""

    def __init__(self, cfg=None):
        super().__init__()
        self.first_bn = nn.BatchNorm2d(1)
        self.first_bn1 = nn.BatchNorm2d(64)      # defined, never used (wav2vec2_resnet_nll.py:38): state-dict compatibility
        self.resnet = ResNet(**(cfg or DEFAULT_RESNET))

    def forward(self, feats, frames=None):
        """frames: host-side frame counts (a list of ints, one per row of a zero-padded batch, each in min_frames()..T); feats rows at or
        beyond an utterance's frames are not interpreted.  Two modes: scoring (eval under torch.no_grad(): every utterance gets what it
        gets alone) and training (train mode with autograd on: every BatchNorm takes its batch statistics over the valid positions only,
        hipnn.batch_norm, and the gradient of feats is exactly 0 beyond the frames); the mixed combinations are refused.
        None: a fixed-length batch."""
        rows = counts = None
        train = False
        if frames is not None:
            train = self.training and torch.is_grad_enabled()
            if not train and (self.training or torch.is_grad_enabled()):
                raise NotImplementedError("ResNetHead.forward(feats, frames) is a scoring mode: model.eval() under torch.no_grad() "
                                          "(or a training mode: model.train() with autograd on)")
            if train and STAGES[self.resnet.resnet_type][1]:
                raise NotImplementedError("ResNetHead.forward(feats, frames): training on zero-padded batches is built for the basic-block "
                                          "networks (resnet_type 18 / 28 / 34); the bottleneck types' 1024 / 2048-channel BatchNorms have no "
                                          "train-mode kernel (scl_bn_fwd: C divides 256 or is 512), got resnet_type %r" % self.resnet.resnet_type)
            frames = [int(t) for t in frames]
            if len(frames) != feats.shape[0] or max(frames) > feats.shape[1]:
                raise ValueError("frames: need one count in %d..%d per row of the %r batch, got %r"
                                 % (min_frames(self.resnet.resnet_type, self.resnet.num_nodes), feats.shape[1], tuple(feats.shape), frames))
            counts = batch_rows(frames, self.resnet.resnet_type, self.resnet.num_nodes)
            host = torch.tensor(counts, dtype=torch.int32)
            rows = host.pin_memory().to(feats.device, non_blocking=True)
        x = hipnn.batch_norm(feats.unsqueeze(-1), self.first_bn, hipnn.ACT_SELU, grad_in_place=True,       # the [bz, 1, T, 128] map, channels last
                             valid=None if rows is None else rows[0], counts=None if rows is None else counts[0])
        # a training batch has one padded shape (trim_length): its staging maps stay pooled, as the fixed-length step's
        return self.resnet.run(x, _conv_dtype(), rows, counts if train else None, pooled=True if train else None)
