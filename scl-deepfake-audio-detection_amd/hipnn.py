"""Autograd-visible building blocks of the AASIST / ResNet back-ends, every one of them a HIP kernel behind the C ABI.

The two back-ends (model/wav2vec2_aasist.py:62-604, model/resnet.py:47-191) are a few hundred small layers; what they need from a
device library is: 2-D convolution, BatchNorm (+ReLU / SELU), Linear, a batched matrix product, a 3x3 max pool and global average
pooling — forward and backward.  Here those are

  * convolutions as IMPLICIT GEMMs over channels-last maps: the input is copied once into a zero-padded [B, Hp, Wp, C] map and the
    GEMM kernel addresses the sliding windows in place (rows = output positions with overlapping windows, K = (kh; kw*C + c)
    through the operand's 2-level contiguous index, one batch entry per utterance) — forward, backward-data (a stride-1
    correlation of the zero-dilated, padded output gradient with the flipped weights) and backward-weights (both operands
    transposed, one slab per utterance + a deterministic reduce).  fp32 operands run on the exact-fp32 matrix-core kernel
    (csrc/gemm_f32.hip), bf16 operands on the bf16 kernels (csrc/gemm.hip);
  * BatchNorm + activation, pooling: csrc/nn.hip;  Linear / bmm: the same GEMM entry point.

torch is the tensor container and the autograd tape; no torch.nn.functional compute op of those kinds is called.
Maps are channels-last throughout ([B, H, W, C]); the callers (aasist_head.py, resnet_head.py) are written for that layout.
"""
import weakref

import torch

from . import ops
from .lib import FLAT
from .ops import Op

ACT_NONE, ACT_RELU, ACT_SELU = 0, 1, 2

# Everything here runs on the EXACT f32 matrix-core kernel unless a caller asks otherwise.  With the bf16-pair form (ops.F32X3,
# csrc/gemm_f32.hip, 1.3 - 1.8 x faster per launch) in the FORWARD the reference goldens' outputs still hold 2e-4, but a 5e-6 perturbation of
# the pre-activations flips ReLU / SELU masks and the ResNet's earliest gradients drift to 4e-3 (eval) / 1.5e-2 (train) of their scale
# through 18 layers (bound 2e-3).  The BACKWARD products of a convolution (data and weight gradient: two thirds of the work) are linear maps
# GIVEN the forward's masks: conv2d(..., x3_bwd=True) runs them in the pair form — the masks stay the reference's, the gradients move by
# ~1e-5 (the ResNet back-end asks for it; the per-layer AASIST composition, whose small bias gradients sit at 8e-4 with it, does not).
def _gemm(*a, **kw):
    return ops.gemm(*a, x3=False, **kw)


# Re-laid-out copies of the convolution weights ([Co][kh][kw][Cp] for the forward / wgrad, flipped [Ci][kh][kw][Cop] for the dgrad) are
# pure functions of the weights: they are rebuilt once per optimizer step (the model bumps the epoch), not once per call.
_WEIGHT_EPOCH = 0


def weights_changed():
    """Called by the model after every optimizer step / load_state_dict (the fused AdamW kernel writes through raw pointers, which
    torch's per-tensor version counter does not see)."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1


def _packed(weight, kind, dtype, build):
    if torch.cuda.is_current_stream_capturing():
        return build()          # inside a hipGraph capture the re-layout must be part of the graph: every replay reads the live weights
    cache = weight.__dict__.setdefault("_scl_packed", {})        # lives and dies with the parameter object
    hit = cache.get((kind, dtype))
    if hit is None or hit[0] != (_WEIGHT_EPOCH, weight._version):
        hit = ((_WEIGHT_EPOCH, weight._version), build())
        cache[(kind, dtype)] = hit
    return hit[1]


def _packed_conv(weight, dtype, Co, Ci, kh, kw, Cp, Cop):
    """(forward / weight-gradient operand [Co, kh*kw*Cp], data-gradient operand [Ci, kh*kw*Cop]) of a Conv2d weight: one HIP launch per
    convolution and optimizer step (scl_conv_pack_weights) instead of two fills, a flip and two strided copies."""
    def build():
        w = weight.detach()
        if w.dtype != torch.float32 or not w.is_contiguous():
            w = w.float().contiguous()
        fwd = torch.empty(Co, kh * kw * Cp, dtype=torch.float32, device=w.device)
        bwd = torch.empty(Ci, kh * kw * Cop, dtype=torch.float32, device=w.device)
        ops.conv_pack_weights(w, fwd, bwd, Co, Ci, kh, kw, Cp, Cop)
        return fwd.to(dtype), bwd.to(dtype)
    return _packed(weight, "conv", dtype, build)


# Zero-bordered / zero-dilated staging maps are written in their interior only (pad_nhwc), so a buffer that was zero-filled ONCE can serve
# every later call with the same geometry: 93 torch fills per ResNet step (0.6 ms at batch 32) disappear.  A forward's padded input lives
# until its backward (busy flag, released there or when the node dies); the backward's own maps are free again as soon as their GEMMs
# are queued (stream order).  Inside a hipGraph capture the fill stays part of the graph.
_ZERO_POOL = {}


def _zeros_acquire(key, numel, dtype, dev, pooled=True):
    """-> entry [tensor, busy, generation].  The generation is bumped on every hand-out: whoever releases (or reads, in a backward) passes
    the generation it was given, so a stale owner — the finaliser of a graph whose backward already released the entry, after a later
    forward took it — can neither free nor silently read a buffer that now belongs to someone else (round-5 advisory).
    pooled=False: a buffer of the caller's own, zero-filled now and back with the allocator when the caller lets go of it — the
    variable-length scoring batches (conv2d pooled=False), whose every padded length is a geometry of its own: pooled, each length met
    would pin a set of staging maps for the life of the process."""
    if not pooled or torch.cuda.is_current_stream_capturing():
        return [torch.zeros(numel, dtype=dtype, device=dev), True, 1]
    lst = _ZERO_POOL.setdefault((key, numel, dtype, dev.index, torch.cuda.current_stream(dev).cuda_stream), [])
    for ent in lst:
        if not ent[1]:
            ent[1] = True
            ent[2] += 1
            return ent
    ent = [torch.zeros(numel, dtype=dtype, device=dev), True, 1]
    if len(lst) < 8:
        lst.append(ent)
    return ent


def _zeros_release(ent, gen=None):
    if gen is None or ent[2] == gen:
        ent[1] = False


def _ceil(v, m):
    return (v + m - 1) // m * m


def _colsum(x2d, M, N):
    """Column sums of a contiguous f32 [M, N] (bias gradients): the self-finishing HIP reduction when its 8-column vectors fit."""
    if N % 8:
        return x2d.view(M, N).sum(0)          # the 2-class / 1-score layers (computed 4 wide): a handful of columns
    out = torch.empty(N, device=x2d.device)
    part = torch.empty(ops.colsum_reduce_nparts(M, N) * N, device=x2d.device)
    ops.colsum_reduce(x2d, part, out, M, N)
    return out


# ---- convolution ---------------------------------------------------------------------------------------------------------------------
class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dtype, x3_bwd=False, grad_in_place=False, residual=None, pooled=True):
        """x [B, H, W, Ci] f32; weight [Co, Ci, kh, kw] (torch layout); bias [Co] or None -> y [B, OH, OW, Co] f32 (+ residual, same shape)."""
        B, H, W, Ci = x.shape
        Co, _, kh, kw = weight.shape
        sh, sw = stride
        ph, pw = padding
        vec = 8 if dtype == torch.bfloat16 else 4
        Cp = _ceil(Ci, vec)
        Hp, Wp = H + 2 * ph, W + 2 * pw
        OH, OW = (Hp - kh) // sh + 1, (Wp - kw) // sw + 1
        dev = x.device
        rowmap = (W, H * W, Hp * Wp * Cp, Wp * Cp, Cp, (ph * Wp + pw) * Cp)
        ent = _zeros_acquire(("xp", id(weight), Ci) + rowmap, B * Hp * Wp * Cp + 4096, dtype, dev, pooled)        # tail slack: tile rows past the map are masked, not skipped
        xp = ent[0]
        xc = x.contiguous()
        ops.pad_nhwc(xc, B * H * W, Ci, xp, rowmap)
        ctx.xp_ent, ctx.xp_gen = ent, ent[2]
        weakref.finalize(ctx, _zeros_release, ent, ent[2])
        wk = _packed_conv(weight, dtype, Co, Ci, kh, kw, Cp, _ceil(Co, vec))[0]
        K = kh * kw * Cp
        y = torch.empty(B, OH, OW, Co, dtype=torch.float32, device=dev)
        _gemm(Op(xp, sw * Cp, rpb=OW, rbstride=sh * Wp * Cp, cin=kw * Cp, cout=Wp * Cp, bs1=Hp * Wp * Cp), Op(wk, K), y, OH * OW, Co, K,
                 nb1=B, c_bs1=OH * OW * Co, bias=None if bias is None else bias.detach().float().contiguous(),
                 **({} if residual is None else dict(R=residual.detach().contiguous().float(), rmode=1)))       # the block's skip connection in the epilogue
        ctx.save_for_backward(xp, weight)
        ctx.geom = (B, H, W, Ci, Co, kh, kw, sh, sw, ph, pw, Cp, Hp, Wp, OH, OW, dtype, bias is not None)
        ctx.x3_bwd = bool(x3_bwd)
        ctx.grad_in_place = weight if grad_in_place else None      # the Parameter itself: saved_tensors hands back a fresh tensor object without .grad
        return y

    @staticmethod
    def backward(ctx, dy):
        xp, weight = ctx.saved_tensors
        if ctx.xp_ent[2] != ctx.xp_gen:
            raise RuntimeError("hipnn.conv2d: this node's padded input was handed to a later forward (generation %d, node holds %d) — "
                               "a second backward through a graph whose first backward already released it" % (ctx.xp_ent[2], ctx.xp_gen))
        B, H, W, Ci, Co, kh, kw, sh, sw, ph, pw, Cp, Hp, Wp, OH, OW, dtype, has_bias = ctx.geom
        x3_bwd = ctx.x3_bwd
        dev = dy.device
        dy = dy.contiguous().float()
        vec = 8 if dtype == torch.bfloat16 else 4
        Cop = _ceil(Co, vec)
        K = kh * kw * Cp
        db = None
        if has_bias and ctx.needs_input_grad[2]:
            db = _colsum(dy, B * OH * OW, Co)
        dx = dw = None
        need_dw, need_dx = ctx.needs_input_grad[1], ctx.needs_input_grad[0]
        # A stride-1 "same" convolution (k - 1 = 2 p: every 3x3 / 1x1 of the ResNet body) has a padded output-gradient map dyp of exactly
        # the padded input's geometry, and the weight gradient is then ONE long reduction over the flat padded grid of the whole batch:
        #   dW[co][(r,s,c)] = sum_q dyp[q + off][co] * xp[q + r*Wp + s][c],   off = (k-1-p) * (Wp + 1)
        # (border positions contribute dyp = 0).  Split-K slabs replace the per-utterance slabs: 2-8 partial [Co, K] images instead of
        # 32-256, and hundreds of K steps per block instead of 5 on the deep layers' 9 x 16 maps.  Measured at batch 32 (same box, kernel trace):
        # weight-gradient GEMMs 2.47 -> 2.46 ms, their finishing kernel 0.85 -> 0.68 ms per step.
        flat = need_dw and sh == 1 and sw == 1 and kh - 1 == 2 * ph and kw - 1 == 2 * pw and dtype == torch.float32
        ent_p = dyp = None
        Hd, Wd = H + kh - 1, W + kw - 1
        if need_dx or flat:
            rm = (OW, OH * OW, Hd * Wd * Cop, sh * Wd * Cop, sw * Cop, ((kh - 1 - ph) * Wd + (kw - 1 - pw)) * Cop)
            ent_p = _zeros_acquire(("dyp", Co) + rm, B * Hd * Wd * Cop + 4096, dtype, dev)
            dyp = ent_p[0]
            ops.pad_nhwc(dy, B * OH * OW, Co, dyp, rm)
        if need_dw:
            tile = 64 if dtype == torch.float32 else 128
            ent_c = None
            if flat:
                off = (kh - 1 - ph) * Wp + (kw - 1 - pw)
                R = B * Hp * Wp - (kh - 1) * Wp - (kw - 1)          # the last window that still holds an output position
                # the f32 kernel takes 128 x 128 tiles (2 blocks per CU) once 512 of them exist, 64 x 64 (4 per CU) otherwise: aim at
                # ~1024 blocks, two rounds of the former or one of the latter
                t = 128 if (Co >= 128 and K >= 128) else 64
                tiles = ((Co + t - 1) // t) * ((K + t - 1) // t)
                nslab = max(1, min(128, (1024 + tiles // 2) // tiles, (R // 32) // 8))
                slabs = torch.empty(nslab, Co, K, dtype=torch.float32, device=dev)
                ops.gemm(Op(dyp[off * Cop:], Cop), Op(xp, Cp, cin=kw * Cp, cout=Wp * Cp), slabs, Co, K, R, a_t=True, b_t=True, splitk=nslab,
                         c_split_stride=Co * K if nslab > 1 else 0, x3=x3_bwd)
            else:
                # dW[co][(kh,kw,c)] = sum_b sum_(oh,ow) dy[b,oh,ow,co] * xp[b, oh*sh+kh, ow*sw+kw, c]: both operands transposed (rows = the
                # reduction index), one [Co, K] slab per utterance, summed in a fixed order
                dyc = dy if (dtype == torch.float32 and Cop == Co) else None
                if dyc is None:
                    rmc = (OW, OH * OW, OH * OW * Cop, OW * Cop, Cop, 0)
                    ent_c = _zeros_acquire(("dyc", Co) + rmc, B * OH * OW * Cop + 4096, dtype, dev)
                    dyc = ent_c[0]
                    ops.pad_nhwc(dy, B * OH * OW, Co, dyc, rmc)
                tiles = ((Co + tile - 1) // tile) * ((K + tile - 1) // tile) * B
                sk = max(1, min(8, 1024 // max(tiles, 1), (OH * OW) // 256))          # enough blocks to hide the single-stage prefetch
                nslab = B * sk
                slabs = torch.empty(nslab, Co, K, dtype=torch.float32, device=dev)
                ops.gemm(Op(dyc, Cop, bs1=OH * OW * Cop), Op(xp, sw * Cp, rpb=OW, rbstride=sh * Wp * Cp, cin=kw * Cp, cout=Wp * Cp, bs1=Hp * Wp * Cp),
                         slabs, Co, K, OH * OW, a_t=True, b_t=True, nb1=B, c_bs1=sk * Co * K, splitk=sk, c_split_stride=Co * K if sk > 1 else 0, x3=x3_bwd)
            # slab sum (fixed order) + [Co][kh][kw][Cp] -> torch layout in one kernel; with grad_in_place (parameters whose .grad is an
            # attached flat-buffer view: the model plugins) also autograd's accumulation, and no gradient is handed back to the engine
            g = ctx.grad_in_place.grad if ctx.grad_in_place is not None else None
            if g is not None and g.dtype == torch.float32 and g.is_contiguous() and not torch.cuda.is_current_stream_capturing():
                ops.conv_wgrad_finish(slabs, g, nslab, Co, Ci, kh, kw, Cp, accumulate=True)
            else:
                dw = torch.empty(Co, Ci, kh, kw, dtype=torch.float32, device=dev)
                ops.conv_wgrad_finish(slabs, dw, nslab, Co, Ci, kh, kw, Cp, accumulate=False)
            if ent_c is not None:
                _zeros_release(ent_c)
        if need_dx:
            # dx = stride-1 correlation of the zero-dilated output gradient (padded by k-1-p) with the flipped, transposed weights
            Kd = kh * kw * Cop
            wd = _packed_conv(weight, dtype, Co, Ci, kh, kw, Cp, Cop)[1]
            dx = torch.empty(B, H, W, Ci, dtype=torch.float32, device=dev)
            ops.gemm(Op(dyp, Cop, rpb=W, rbstride=Wd * Cop, cin=kw * Cop, cout=Wd * Cop, bs1=Hd * Wd * Cop), Op(wd, Kd), dx, H * W, Ci, Kd,
                     nb1=B, c_bs1=H * W * Ci, x3=x3_bwd)
        if ent_p is not None:
            _zeros_release(ent_p)
        _zeros_release(ctx.xp_ent, ctx.xp_gen)
        return dx, dw, db, None, None, None, None, None, (dy if ctx.needs_input_grad[8] else None), None


def conv2d(x, weight, bias=None, stride=(1, 1), padding=(0, 0), dtype=torch.float32, x3_bwd=False, grad_in_place=False, residual=None,
           pooled=True):
    """Channels-last 2-D convolution (cross-correlation, as nn.Conv2d): x [B, H, W, Ci] -> [B, OH, OW, Co] (+ residual [B, OH, OW, Co], added in
    the GEMM epilogue; its gradient is the output gradient).  grad_in_place: the weight
    gradient is ADDED into `weight.grad` by the finishing kernel (when that tensor exists) instead of being returned to autograd — for
    `.backward()` callers whose parameters carry attached .grad views (the plugins' flat gradient buffer); torch.autograd.grad callers
    leave it off.  pooled=False (no-grad callers only): the zero-bordered staging map is not kept in the per-geometry pool (_zeros_acquire)."""
    if not pooled and torch.is_grad_enabled():
        raise ValueError("hipnn.conv2d: pooled=False is for forward-only callers (torch.no_grad())")
    return _Conv2dFn.apply(x, weight, bias, tuple(stride), tuple(padding), dtype, x3_bwd, grad_in_place, residual, pooled)


# ---- BatchNorm (+ activation) --------------------------------------------------------------------------------------------------------
def _bn_param_grads(ctx, C, dev, has_w, has_b):
    """Where a BatchNorm backward's finishing kernel puts dgamma / dbeta: (dg, db, accumulate).  accumulate: both parameters carry an
    attached, contiguous f32 .grad (the plugins' flat gradient buffer) and nothing is being captured - the kernel adds into them (what
    AccumulateGrad would do with two more launches) and autograd gets no parameter gradient back.  Otherwise fresh buffers to hand back."""
    if ctx.in_place is not None and has_w and has_b and not torch.cuda.is_current_stream_capturing():
        gw, gb = ctx.in_place[0].grad, ctx.in_place[1].grad
        if all(g is not None and g.dtype == torch.float32 and g.is_contiguous() for g in (gw, gb)):
            return gw, gb, True
    return (torch.empty(C, device=dev) if has_w else None), (torch.empty(C, device=dev) if has_b else None), False


class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, nbt, training, momentum, eps, act, grad_in_place=False):
        C = x.shape[-1]
        xc = x.contiguous().float()
        N = xc.numel() // C
        dev = x.device
        part = torch.empty(ops.bn_nslabs(N) * 2 * C, dtype=torch.float64, device=dev)
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        y = torch.empty_like(xc)
        ops.bn_fwd(xc, N, C, weight, bias, running_mean, running_var, nbt, training, momentum, eps, act, part, mean, rstd, y)
        ctx.save_for_backward(xc, y, mean, rstd, weight)
        ctx.cfg = (N, C, act, training, weight is not None, bias is not None)
        ctx.in_place = (weight, bias) if grad_in_place else None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, y, mean, rstd, weight = ctx.saved_tensors
        N, C, act, training, has_w, has_b = ctx.cfg
        dev = dy.device
        dyc = dy.contiguous().float()
        part = torch.empty(ops.bn_nslabs(N) * 2 * C, dtype=torch.float64, device=dev)
        sums = torch.empty(2 * C, device=dev)
        dx = torch.empty_like(xc)
        dg, db, acc = _bn_param_grads(ctx, C, dev, has_w, has_b)
        ops.bn_bwd(dyc, y, xc, mean, rstd, weight, N, C, act, training, part, sums, dg, db, dx, accumulate=acc)
        return (dx,) + ((None, None) if acc else (dg, db)) + (None,) * 8


class _BatchNormOwnFn(torch.autograd.Function):
    """Train-mode BatchNorm + activation over the own positions of a zero-padded variable-length batch x [B, H, W, C]: the rows
    h < own[b] (scl_bn_fwd_masked / scl_bn_bwd_masked), or with `cols` the columns w < own[b] (scl_bn_fwd_cols / scl_bn_bwd_cols)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, nbt, momentum, eps, act, grad_in_place, cols, own, counts):
        B, H, W, C = x.shape
        xc = x.contiguous().float()
        dev = x.device
        part = torch.empty(ops.bn_masked_nslabs(B, H, W) * 2 * C, dtype=torch.float64, device=dev)
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        y = torch.empty_like(xc)
        fwd = ops.bn_fwd_cols if cols else ops.bn_fwd_masked
        fwd(xc, B, H, W, C, weight, bias, running_mean, running_var, nbt, momentum, eps, act, own, counts, part, mean, rstd, y)
        ctx.save_for_backward(xc, y, mean, rstd, weight, own)
        ctx.cfg = (B, H, W, C, act, weight is not None, bias is not None, cols, counts)
        ctx.in_place = (weight, bias) if grad_in_place else None
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, y, mean, rstd, weight, own = ctx.saved_tensors
        B, H, W, C, act, has_w, has_b, cols, counts = ctx.cfg
        dev = dy.device
        dyc = dy.contiguous().float()
        part = torch.empty(ops.bn_masked_nslabs(B, H, W) * 2 * C, dtype=torch.float64, device=dev)
        sums = torch.empty(2 * C + 4, device=dev)
        dx = torch.empty_like(xc)
        dg, db, acc = _bn_param_grads(ctx, C, dev, has_w, has_b)
        bwd = ops.bn_bwd_cols if cols else ops.bn_bwd_masked
        bwd(dyc, y, xc, mean, rstd, weight, B, H, W, C, act, own, counts, part, sums, dg, db, dx, accumulate=acc)
        return (dx,) + ((None, None) if acc else (dg, db)) + (None,) * 10


def _batch_norm_own(x, bn, act, grad_in_place, cols, own, counts):
    if counts is None:
        counts = own.tolist()
    momentum = 0.1 if bn.momentum is None else bn.momentum
    return _BatchNormOwnFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, momentum, bn.eps, act,
                                 grad_in_place, cols, own, tuple(int(v) for v in counts))


def batch_norm(x, bn, act=ACT_NONE, grad_in_place=False, valid=None, counts=None):
    """nn.BatchNorm1d / 2d semantics over the LAST dimension of x (channels-last), fused with `act`; `bn` supplies weight, bias, the
    running statistics and the training flag (its forward is never called).  grad_in_place: as conv2d's.
    valid: int32 [B] on the GPU with x [B, H, W, C], the rows h < valid[b] that utterance b of a zero-padded variable-length batch owns
    (0 <= valid[b] <= H, validated by the caller on the host).  Two modes.  Eval mode under torch.no_grad(): a BatchNorm is a per-element
    map, so the valid rows get the bits they get without `valid`, and the rest is exactly 0 whatever x holds there.  Train mode with
    autograd on: batch statistics (and the running statistics' update) over the valid positions only, exactly 0 beyond, and a backward whose
    sums run over the valid positions and whose dx is exactly 0 beyond.  counts: the same counts on the host (a list of ints: the entry
    points refuse a batch without any valid position before they launch); left out, they are read back from `valid`.  The mixed
    combinations (eval mode with autograd on, train mode under torch.no_grad()) are refused."""
    training = bn.training or bn.running_mean is None
    if valid is not None:
        if x.dim() != 4:
            raise ValueError("hipnn.batch_norm: `valid` needs a [B, H, W, C] map, got %r" % (tuple(x.shape),))
        if training and torch.is_grad_enabled():
            return _batch_norm_own(x, bn, act, grad_in_place, False, valid, counts)
        if training or torch.is_grad_enabled():
            raise NotImplementedError("hipnn.batch_norm: `valid` is a scoring mode (a BatchNorm in eval mode under torch.no_grad()); "
                                      "batch statistics over the valid positions and a backward are not implemented")
        B, H, W, C = x.shape
        xc = x.contiguous().float()
        mean, rstd = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
        y = torch.empty_like(xc)
        ops.bn_eval_masked(xc, B, H, W, C, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, act, valid, mean, rstd, y)
        return y
    momentum = 0.1 if bn.momentum is None else bn.momentum
    return _BatchNormFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked if training else None, training,
                              momentum, bn.eps, act, grad_in_place)


def batch_norm_cols(x, bn, act, widths):
    """Eval-mode BatchNorm + `act` of x [B, H, W, C] under torch.no_grad() with the mask on the COLUMNS: utterance b owns w < widths[b]
    (int32 [B] on the GPU) of every row and gets there the bits batch_norm gives without a mask; everything at and beyond is exactly 0,
    whatever x holds (selected: not read).  The AASIST stack's ragged axis (aasist_long.py); `valid` of batch_norm masks the rows h."""
    if bn.training or bn.running_mean is None or torch.is_grad_enabled() or x.dim() != 4:
        raise NotImplementedError("hipnn.batch_norm_cols: a scoring mode (a BatchNorm in eval mode under torch.no_grad()) on a [B, H, W, C] map")
    B, H, W, C = x.shape
    xc = x.contiguous().float()
    mean, rstd = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    y = torch.empty_like(xc)
    ops.bn_eval_cols(xc, B, H, W, C, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, act, widths, mean, rstd, y)
    return y


def batch_norm_cols_train(x, bn, act, widths, counts=None, grad_in_place=False):
    """Train-mode BatchNorm + `act` of x [B, H, W, C] with autograd on and the mask on the COLUMNS: utterance b owns w < widths[b] (int32 [B]
    on the GPU) of every row.  Mean and biased variance over the batch's own positions only (N_v = H * sum widths), the running statistics
    moved with the unbiased variance, num_batches_tracked + 1; y exactly 0 at and beyond widths[b] whatever x holds there (not read), and a
    backward whose sums run over the own positions and whose dx is exactly 0 at and beyond.  counts: the same widths on the host (the entry
    points refuse a batch without any own position before they launch); left out, they are read back from `widths`.
    Batch statistics couple the rows of the batch: unlike batch_norm_cols (scoring), an utterance's result depends on its batch.
    Eval mode and torch.no_grad() are batch_norm_cols' business and are refused here."""
    training = bn.training or bn.running_mean is None
    if not training or not torch.is_grad_enabled() or x.dim() != 4:
        raise NotImplementedError("hipnn.batch_norm_cols_train: a BatchNorm in train mode with autograd on, on a [B, H, W, C] map "
                                  "(scoring: hipnn.batch_norm_cols)")
    return _batch_norm_own(x, bn, act, grad_in_place, True, widths, counts)


class _ZeroColsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, widths):
        y = x.float().clone(memory_format=torch.contiguous_format)
        ops.zero_cols(y, *y.shape, widths)
        ctx.save_for_backward(widths)
        return y

    @staticmethod
    def backward(ctx, dy):
        (widths,) = ctx.saved_tensors
        dx = dy.float().clone(memory_format=torch.contiguous_format)
        ops.zero_cols(dx, *dx.shape, widths)
        return dx, None


def zero_cols(x, widths):
    """Out of place and differentiable: a copy of x [B, H, W, C] with exact zeros stored at the columns w >= widths[b] (scl_zero_cols); the
    backward stores exact zeros at the same columns of the gradient (selected: a NaN gradient there reaches nothing upstream)."""
    if x.dim() != 4:
        raise ValueError("hipnn.zero_cols: a [B, H, W, C] map, got %r" % (tuple(x.shape),))
    return _ZeroColsFn.apply(x, widths)


def zero_cols_(x, widths):
    """In place, under torch.no_grad(): x [B, H, W, C] (contiguous f32) gets exact zeros stored at the columns w >= widths[b]."""
    if torch.is_grad_enabled() or x.dim() != 4 or not x.is_contiguous() or x.dtype != torch.float32:
        raise NotImplementedError("hipnn.zero_cols_: a contiguous f32 [B, H, W, C] map under torch.no_grad()")
    ops.zero_cols(x, *x.shape, widths)
    return x


# ---- Linear / bmm ----------------------------------------------------------------------------------------------------------------------
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        N, K = weight.shape
        xc = x.contiguous().float().view(-1, K)
        M = xc.shape[0]
        wc = weight.detach().contiguous().float()
        y = torch.empty(M, N, device=x.device)
        _gemm(Op(xc, K), Op(wc, K), y, M, N, K, bias=None if bias is None else bias.detach().contiguous().float())
        ctx.save_for_backward(xc, wc)
        ctx.meta = (x.shape, bias is not None)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        xshape, has_b = ctx.meta
        N, K = wc.shape
        M = xc.shape[0]
        dev = dy.device
        dyc = dy.contiguous().float().view(M, N)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=dev)
            _gemm(Op(dyc, N), Op(wc, K), dx, M, K, N, b_t=True)
            dx = dx.view(xshape)
        if ctx.needs_input_grad[1]:
            dw = torch.empty(N, K, device=dev)
            # a [<= 128, <= 128] output is one or two tiles: split the reduction over the rows so that the launch is not a single
            # block walking M / 32 steps at HBM latency, then sum the slabs in a fixed order
            tiles = ((N + 63) // 64) * ((K + 63) // 64)
            sk = max(1, min(32, 256 // tiles, M // 128))
            if sk > 1:
                slabs = torch.empty(sk, N, K, device=dev)
                _gemm(Op(dyc, N), Op(xc, K), slabs, N, K, M, a_t=True, b_t=True, splitk=sk, c_split_stride=N * K)
                ops.reduce_slabs(slabs, dw, N * K, sk, N * K)
            else:
                _gemm(Op(dyc, N), Op(xc, K), dw, N, K, M, a_t=True, b_t=True)
        if has_b and ctx.needs_input_grad[2]:
            db = _colsum(dyc, M, N)
        return dx, dw, db


def linear(x, weight, bias=None):
    """nn.Linear on the exact-fp32 GEMM.  16-byte operand vectors need in_features % 4 == 0 and out_features % 4 == 0: narrower outputs
    (the 2-class and 1-score layers) are computed 4 wide with zero rows and sliced."""
    N, K = weight.shape
    if K % 4:
        pad = 4 - K % 4
        x = torch.nn.functional.pad(x, (0, pad))
        weight = torch.nn.functional.pad(weight, (0, pad))
    if N % 4:
        pad = 4 - N % 4
        weight = torch.nn.functional.pad(weight, (0, 0, 0, pad))
        bias = None if bias is None else torch.nn.functional.pad(bias, (0, pad))
        return _LinearFn.apply(x, weight, bias)[..., :N]
    return _LinearFn.apply(x, weight, bias)


class _BmmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        """a [B, M, K] @ b [B, K, N] -> [B, M, N]   (K % 4 == 0 and N % 4 == 0)."""
        B, M, K = a.shape
        N = b.shape[2]
        ac, bc = a.contiguous().float(), b.contiguous().float()
        c = torch.empty(B, M, N, device=a.device)
        _gemm(Op(ac, K, bs1=M * K), Op(bc, N, bs1=K * N), c, M, N, K, b_t=True, nb1=B, c_bs1=M * N)
        ctx.save_for_backward(ac, bc)
        return c

    @staticmethod
    def backward(ctx, dc):
        ac, bc = ctx.saved_tensors
        B, M, K = ac.shape
        N = bc.shape[2]
        dcc = dc.contiguous().float()
        da = db = None
        if ctx.needs_input_grad[0]:          # dA[m][k] = sum_n dC[m][n] B[k][n]
            da = torch.empty(B, M, K, device=dc.device)
            _gemm(Op(dcc, N, bs1=M * N), Op(bc, N, bs1=K * N), da, M, K, N, nb1=B, c_bs1=M * K)
        if ctx.needs_input_grad[1]:          # dB[k][n] = sum_m A[m][k] dC[m][n]
            db = torch.empty(B, K, N, device=dc.device)
            _gemm(Op(ac, K, bs1=M * K), Op(dcc, N, bs1=M * N), db, K, N, M, a_t=True, b_t=True, nb1=B, c_bs1=K * N)
        return da, db


def bmm(a, b):
    """torch.bmm on the exact-fp32 GEMM; the contraction and the output width are zero-padded to multiples of 4 (graph sizes such as 42
    or 66 nodes are not)."""
    K, N = a.shape[2], b.shape[2]
    pk, pn = (-K) % 4, (-N) % 4
    if pk:
        a = torch.nn.functional.pad(a, (0, pk))
        b = torch.nn.functional.pad(b, (0, 0, 0, pk))
    if pn:
        b = torch.nn.functional.pad(b, (0, pn))
    c = _BmmFn.apply(a, b)
    return c[..., :N] if pn else c


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------
class _MaxPool3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        """x [B, H, W] f32 (any strides) -> [B, H // 3, W // 3]  (F.max_pool2d(x, (3, 3)) of a single-channel map)."""
        B, H, W = x.shape
        y = torch.empty(B, H // 3, W // 3, device=x.device)
        idx = torch.empty(B, H // 3, W // 3, dtype=torch.int32, device=x.device)
        xf = x.float()
        ops.maxpool3_fwd(xf, xf.stride(1), xf.stride(2), xf.stride(0), H, W, B, y, idx)
        ctx.save_for_backward(idx)
        ctx.shape = (B, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        B, H, W = ctx.shape
        dx = torch.zeros(B, H, W, device=dy.device)
        ops.maxpool3_bwd(dy.contiguous().float(), idx, H, W, B, dx, W, 1, H * W)
        return dx


def max_pool3(x):
    return _MaxPool3Fn.apply(x)


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        """x [B, R, C] -> [B, C] mean over R."""
        B, R, C = x.shape
        y = torch.empty(B, C, device=x.device)
        ops.avgpool_fwd(x.contiguous().float(), B, R, C, y)
        ctx.shape = (B, R, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, R, C = ctx.shape
        dx = torch.empty(B, R, C, device=dy.device)
        ops.avgpool_bwd(dy.contiguous().float(), B, R, C, dx)
        return dx


def avg_pool_rows(x):
    return _AvgPoolFn.apply(x)


class _AvgPoolMaskedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, valid, counts):
        B, H, W, C = x.shape
        y = torch.empty(B, C, device=x.device)
        ops.avgpool_fwd_masked(x.contiguous().float(), valid, B, H, W, C, y)
        ctx.save_for_backward(valid)
        ctx.cfg = (B, H, W, C, counts)
        return y

    @staticmethod
    def backward(ctx, dy):
        (valid,) = ctx.saved_tensors
        B, H, W, C, counts = ctx.cfg
        dx = torch.empty(B, H, W, C, device=dy.device)
        ops.avgpool_bwd_masked(dy.contiguous().float(), valid, counts, B, H, W, C, dx)
        return dx, None, None


def avg_pool_rows_masked(x, valid, counts=None):
    """x [B, H, W, C] of a zero-padded variable-length batch -> [B, C]: the mean over the rows h < valid[b] (int32 [B] on the GPU) and all of
    W, the bits avg_pool_rows gives for the utterance's [1, valid[b] * W, C] slice alone.  counts: the same counts on the host, checked to be
    in 1..H before anything is launched (a forward-only caller that validated them already leaves it out).  Under autograd the backward
    spreads dy[b] / (valid[b] * W) over the utterance's own rows and writes exact zeros beyond; its entry point takes the host counts, which
    are read back from `valid` when the caller gave none."""
    B, H, W, C = x.shape
    if counts is not None:
        counts = tuple(ops.check_lengths(counts, H))
    if torch.is_grad_enabled() and x.requires_grad:
        if counts is None:
            counts = tuple(ops.check_lengths(valid.tolist(), H))
        return _AvgPoolMaskedFn.apply(x, valid, counts)
    y = torch.empty(B, C, device=x.device)
    ops.avgpool_fwd_masked(x.contiguous().float(), valid, B, H, W, C, y)
    return y
