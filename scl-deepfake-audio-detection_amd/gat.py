"""Autograd wrapper of the fused AASIST pairwise attention score (csrc/gat.hip).

    gat_score(x [B,N,D] f32, att_proj.weight [Do,D], att_proj.bias [Do], a [3,Do] or [1,Do], n1) -> s [B,N,N] f32

replaces `tanh(att_proj(x_i * x_j)) @ att_weight` of GraphAttentionLayer / HtrgGraphAttentionLayer
(model/wav2vec2_aasist.py:107-135, 259-291); the temperature and the softmax stay torch ops on the [B,N,N] result.

For zero-padded batches of graphs of different sizes (node counts per utterance in device tables), both differentiable:

    gat_score_var(x [B,Nmax,D], W, bias, a, nodes, n1) -> s [B, Nmax*Nmax]: the utterance's own [N_b][N_b] at the start of its block
    gat_softmax_agg_var(s, x, nodes, temp, one_row)    -> softmax(s / temp, -1) @ x over the own nodes, no [N,N] matrix in HBM

Nothing beyond an utterance's own nodes is read in either direction, and the rows beyond of every result and gradient are exact zeros.
"""
import torch

from . import ops

# The backward's only N * N * D tensor, dP [B, N, N, D] f32 (4.1 GB at B = 64, N = 500; 16.4 GB at B = 64 and the 999 nodes of a
# 960,000-sample clip): beyond this it is a ValueError, not an allocator failure in the middle of a backward.
MAX_DP_BYTES = 16 << 30


def _score_backward(x, W, ds, na, who, n, launch):
    """What the two pair-score backwards share around their one launch: the refusal of a scratch beyond MAX_DP_BYTES (`who`, `n`: the
    message's own words), the scratch, launch(ds, dP, part, dx, B, N, D, Do), the column reduce -> (dx, dW, db, da[:na])."""
    B, N, D = x.shape
    Do = W.shape[0]
    nb = ops.gat_score_nblocks(N) * B
    ncol = Do * D + 4 * Do
    if B * N * N * D * 4 > MAX_DP_BYTES:
        raise ValueError("%s backward: the pair-gradient scratch dP [B=%d, %s=%d, %s, D=%d] f32 is %.1f GiB, above the %d GiB bound "
                         "(MAX_DP_BYTES); use a smaller batch" % (who, B, n, N, n, D, B * N * N * D * 4 / 2 ** 30, MAX_DP_BYTES >> 30))
    dP = torch.empty(B * N * N * D, device=x.device, dtype=torch.float32)
    part = torch.empty(nb, ncol, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    launch(ds.contiguous().float(), dP, part, dx, B, N, D, Do)
    red = torch.empty(ncol, device=x.device, dtype=torch.float32)
    ops.colreduce(part, red, nb, ncol)
    return dx, red[: Do * D].view(Do, D), red[Do * D: Do * D + Do], red[Do * D + Do:].view(3, Do)[:na]


class _GatScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, bias, a, n1):
        B, N, D = x.shape
        Do = W.shape[0]
        xc, Wc, bc = x.contiguous().float(), W.contiguous().float(), bias.contiguous().float()
        a3 = torch.zeros(3, Do, device=x.device, dtype=torch.float32)
        a3[: a.shape[0]] = a
        s = torch.empty(B, N, N, device=x.device, dtype=torch.float32)
        ops.gat_score_fwd(xc, Wc, bc, a3, s, B, N, D, Do, n1)
        ctx.save_for_backward(xc, Wc, bc, a3)
        ctx.n1, ctx.na = n1, a.shape[0]
        return s

    @staticmethod
    def backward(ctx, ds):
        x, W, bias, a3 = ctx.saved_tensors
        return _score_backward(x, W, ds, ctx.na, "gat_score", "N", lambda ds, dP, part, dx, *dims: ops.gat_score_bwd(
            x, W, bias, a3, ds, dP, part, dx, *dims, ctx.n1)) + (None,)


class _GatScoreVarFn(torch.autograd.Function):
    """gat_score for graphs of different sizes in one zero-padded batch (scl_gat_score_fwd_var / scl_gat_score_bwd_var)."""

    @staticmethod
    def forward(ctx, x, W, bias, a, nodes, n1):
        B, N, D = x.shape
        Do = W.shape[0]
        xc, Wc, bc = x.contiguous().float(), W.contiguous().float(), bias.contiguous().float()
        a3 = torch.zeros(3, Do, device=x.device, dtype=torch.float32)
        a3[: a.shape[0]] = a
        s = torch.empty(B, N * N, device=x.device, dtype=torch.float32)
        ops.gat_score_fwd_var(xc, Wc, bc, a3, s, nodes, n1, B, N, D, Do)
        ctx.save_for_backward(xc, Wc, bc, a3, nodes, n1)
        ctx.na = a.shape[0]
        return s

    @staticmethod
    def backward(ctx, ds):
        x, W, bias, a3, nodes, n1 = ctx.saved_tensors
        return _score_backward(x, W, ds, ctx.na, "gat_score_var", "Nmax", lambda ds, dP, part, dx, *dims: ops.gat_score_bwd_var(
            x, W, bias, a3, ds, dP, part, dx, nodes, n1, *dims)) + (None, None)


def gat_score_var(x, W, bias, a, nodes, n1=None):
    """gat_score on a zero-padded batch x [B, Nmax, D] of graphs of nodes[b] nodes each (int32 [B] on the GPU; n1: the first-type counts of
    a heterogeneous layer, None: homogeneous) -> s [B, Nmax * Nmax]: utterance b's own [nodes[b]][nodes[b]] matrix, contiguous at the start
    of its block (what gat_softmax_agg_var reads).  Differentiable in x, W, bias and a; rows of x and entries of the incoming gradient beyond
    the own graph are never read, and the rows >= nodes[b] of x's gradient are exact zeros.  (D, Do) among the matrix-core kernels' pairs,
    Nmax <= 1024."""
    return _GatScoreVarFn.apply(x, W, bias, a, nodes, n1)


class _GatSoftmaxAggVarFn(torch.autograd.Function):
    """Masked soft-max + aggregation in one kernel and its backward (scl_gat_softmax_agg_var / scl_gat_softmax_agg_var_bwd)."""

    @staticmethod
    def forward(ctx, s, x, nodes, temp, one_row):
        B, N, D = x.shape
        sc, xc = s.contiguous().float(), x.contiguous().float()
        out = torch.empty((B, D) if one_row else (B, N, D), device=x.device, dtype=torch.float32)
        ops.gat_softmax_agg_var(sc, xc, nodes, out, B, N, D, temp, one_row)
        ctx.save_for_backward(sc, xc, nodes)
        ctx.cfg = (float(temp), bool(one_row))
        return out

    @staticmethod
    def backward(ctx, dout):
        s, x, nodes = ctx.saved_tensors
        temp, one_row = ctx.cfg
        B, N, D = x.shape
        # one_row: the score row comes from torch glue, whose backward reads all of ds - zeros beyond the own nodes.  The matrix form's ds
        # goes to gat_score_var's backward, which reads the own [N_b][N_b] only.
        ds, dx = (torch.zeros_like(s) if one_row else torch.empty_like(s)), torch.empty_like(x)
        stats = torch.empty(B * (1 if one_row else N) * 2, device=x.device, dtype=torch.float32)
        ops.gat_softmax_agg_var_bwd(s, x, nodes, dout.contiguous().float(), ds, dx, stats, B, N, D, temp, one_row)
        return ds, dx, None, None, None


def gat_softmax_agg_var(s, x, nodes, temp, one_row=False):
    """softmax(s / temp, -1) @ x over each utterance's own nodes without the [N, N] attention matrix in HBM, differentiable in s and x.
    s: gat_score_var's layout (one_row: [B, Nmax], the master node's single score row -> [B, D]); x [B, Nmax, D]; rows >= nodes[b] of the
    result and of x's gradient are exact zeros; the gradient of s is written in the layout of s (its entries beyond the own graph mean nothing
    and are never read by gat_score_var's backward)."""
    return _GatSoftmaxAggVarFn.apply(s, x, nodes, temp, one_row)


def gat_score(x, W, bias, a, n1=None):
    """a: [1, Do] (homogeneous layer) or [3, Do] = (a11, a22, a12) with n1 = number of first-type nodes."""
    return _GatScoreFn.apply(x, W, bias, a, x.shape[1] if n1 is None else n1)
