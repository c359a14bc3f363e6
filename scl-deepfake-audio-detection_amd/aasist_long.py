"""AASIST back-end on zero-padded batches of different lengths, beyond the fused kernels' 242 frames: one per-layer composition with count
tables (_compose), entered in one of two modes.

  forward_frames_long   scoring (SCL_AASIST_LENGTHS=long): eval mode under torch.no_grad().  Row b of the result is what AasistHead.forward
                        gives feats[b:b+1, :frames[b]] alone.
  forward_frames_train  training (SCL_AASIST_TRAIN_LENGTHS=1): train mode with autograd on.  Batch statistics over the batch's own positions
                        couple the rows; the backward is the exact gradient of the forward.

Both take feats [B, T, 128] zero-padded and host-side frame counts, and in both nothing at or beyond an utterance's frames, columns or nodes
reaches a bit of any result, gradient or buffer (NaN there included).  The walk is the fixed-length forward's beyond the fused kernels
(Residual_block.run, the torch attention pooling, graph_unfused), with every size that follows the utterance taken from count tables:

  stack      every convolution input is exact zeros at and beyond the utterance's columns W_b = frames // 3, selected and not multiplied:
             the BatchNorm + SELU that feed a convolution mask the columns, and so does a block's output (scl_zero_cols).
  pooling    the soft-max along time runs over the utterance's own columns (the padded logits are replaced by -inf, selected); e_T rows at
             and beyond W_b are replaced by zeros and never reach a result.
  graph      node counts per utterance (node_counts).  The pair scores are gat.gat_score_var (up to 1024 nodes), soft-max and att @ x one
             kernel (gat.gat_softmax_agg_var: the [N, N] attention matrix never reaches HBM), also for the master node's single score row.
             A heterogeneous layer's nodes are the ragged [kT_b temporal | kS spectral], packed at the front of the utterance's block by a
             gather through long_tables' index tables, n1 = kT_b.  GraphPool keeps k_b of N_b own nodes: the padded scores are replaced by
             -1 (below every sigmoid) and torch.topk returns descending order, so the first k_b kept nodes and their order are the
             utterance's own.  The read-out's abs-max and mean run over rows that are zero beyond the own kT2_b nodes, the mean divided by
             kT2_b.  GAT_layer_S, spectral side alone, is the fixed-length layer.

What the mode decides is bound once at the top of _compose:

                                        scoring                                       training
  BatchNorm + SELU in the stack         hipnn.batch_norm_cols (eval, columns masked)  hipnn.batch_norm_cols_train: statistics over w < W_b
  first_bn1, attention.2                hipnn.batch_norm: a per-element map           the same column-masked train form
  BatchNorm + SELU on the node side     hipnn.batch_norm                              hipnn.batch_norm(valid=): statistics over p < N_b
  convolutions' staging maps            not pooled                                    pooled, keyed by the run's padded length
  a block's output                      hipnn.zero_cols_ in place                     hipnn.zero_cols, differentiable
  the map's width                       the batch's widest utterance                  T // 3; e_T is cut to the widest utterance behind it
  a non-first block's bn1               not run                                       run for its running statistics (its output is discarded)

In training the masked statistics are mean and biased variance, the running statistics move with the unbiased N_v / (N_v - 1) and
num_batches_tracked goes up by 1; every mask is a selection in front of the op whose backward multiplies by its input, so the rows of
d(feats) at and beyond 3 * W_b are exact zeros.  The dropout sites are the torch modules of the fixed-length per-layer path: identities that
launch nothing in eval mode.  torch stays the glue for top-k, gathers and the read-out, as in graph_unfused.  No fused kernel is involved
and nothing is kept between calls.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import gat, hipnn
from .aasist_head import POOL, _lin, check_frames, node_counts

GAT_CAP = 1024                          # csrc/gat.hip: nodes per graph of the tiled pair-score kernels
MAX_FRAMES = POOL * GAT_CAP + POOL - 1  # 3074: GAT_CAP temporal nodes of POOL frames each, plus a partial pool window
GAT_WIDTHS = ((64, 64), (64, 32), (32, 32))      # (D, Do) of the matrix-core pair-score kernels


def long_tables(frames, cfg=None):
    """The host-side count and index tables of a batch of utterances of `frames` LL frames each: node_counts' entries, the batch's padded
    sizes (Wmax, kTmax, kT2max, N1max = kTmax + kS, N2max = kT2max + kS2), and per heterogeneous stage g in (1, 2)
      cat<g>  int64 [B, N<g>max]: node p of utterance b's packed block is row cat[b, p] of torch.cat([temporal [B, k*max, D], spectral], 1);
              -1 at and beyond N<g>_b
      spec<g> int64 [B, kS or kS2]: where the utterance's spectral nodes sit in its block (kT_b .. kT_b + kS - 1)
    A pure function of its arguments (numpy only): what the device tables are uploaded from, and what the CPU tests read."""
    c = dict(node_counts(frames, cfg))
    B = len(c["W"])
    c.update(Wmax=max(c["W"]), kTmax=max(c["kT"]), kT2max=max(c["kT2"]), N1max=max(c["N1"]), N2max=max(c["N2"]))
    for tag, kt, ks in (("1", c["kT"], c["kS"]), ("2", c["kT2"], c["kS2"])):
        ktm = max(kt)
        cat = np.full((B, ktm + ks), -1, dtype=np.int64)
        spec = np.empty((B, ks), dtype=np.int64)
        for b, k in enumerate(kt):
            cat[b, :k] = np.arange(k)
            cat[b, k:k + ks] = ktm + np.arange(ks)
            spec[b] = k + np.arange(ks)
        c["cat" + tag], c["spec" + tag] = cat, spec
    return c


def widths_supported(head):
    """Whether every graph-attention layer of this configuration has one of the matrix-core kernels' (D, Do) pairs."""
    layers = (head.GAT_layer_T, head.HtrgGAT_layer_ST11, head.HtrgGAT_layer_ST12, head.HtrgGAT_layer_ST21, head.HtrgGAT_layer_ST22)
    return all(tuple(m.att_proj.weight.shape[::-1]) in GAT_WIDTHS for m in layers)


def _rows(count, n):
    """bool [B, n]: the rows below each utterance's count (int32 [B] on the GPU)."""
    return torch.arange(n, device=count.device).unsqueeze(0) < count.unsqueeze(1)


def _gat_var(mod, x, nodes, counts, bn):
    """GraphAttentionLayer.forward on x [B, Nmax, D], rows at and beyond nodes[b] zero; bn: the mode's node-side BatchNorm + SELU (in
    scoring the rows beyond of the result mean nothing, in training they are zeros)."""
    x = mod.input_drop(x).contiguous()
    agg = gat.gat_softmax_agg_var(gat.gat_score_var(x, mod.att_proj.weight, mod.att_proj.bias, mod.att_weight.t(), nodes), x, nodes, mod.temp)
    return bn(_lin(mod.proj_with_att, agg) + _lin(mod.proj_without_att, x), mod.bn, nodes, counts)


def _pool_var(pool, h, valid, keep, kmax):
    """GraphPool.forward keeping keep[b] of the utterance's own nodes (valid [B, Nmax]) -> [B, kmax, D], zeros at and beyond keep[b].  The
    scores come from pool.drop(h), the kept rows from h itself."""
    scores = torch.sigmoid(_lin(pool.proj, pool.drop(h)))
    own = torch.where(valid.unsqueeze(-1), scores, scores.new_full((), -1.0))      # below every sigmoid: a padded node is never among the first keep[b]
    idx = torch.topk(own.detach(), kmax, dim=1)[1].expand(-1, -1, h.size(2))
    out = torch.gather(h * scores, 1, idx)
    return torch.where(_rows(keep, kmax).unsqueeze(-1), out, out.new_zeros(()))      # selected: the gradient of a padded slot is an exact 0


def _htrg_var(mod, x1, x2, master, stage, bn):
    """HtrgGraphAttentionLayer.forward (master given) on the ragged [n1[b] rows of x1 | x2] -> (temporal [B, k1max, Do] zero at and beyond
    n1[b], spectral [B, nS, Do], master [B, 1, Do]).  stage: the layer's tables (cat, spec, nodes, n1, k1max, host-side node counts)."""
    cat, spec, nodes, n1, k1max, counts = stage
    both = torch.cat([_lin(mod.proj_type1, x1), _lin(mod.proj_type2, x2)], dim=1)
    D = both.size(2)
    x = torch.gather(both, 1, cat.clamp_min(0).unsqueeze(-1).expand(-1, -1, D))
    x = mod.input_drop(torch.where((cat >= 0).unsqueeze(-1), x, x.new_zeros(()))).contiguous()
    a = torch.cat([mod.att_weight11, mod.att_weight22, mod.att_weight12], dim=1).t()
    agg = gat.gat_softmax_agg_var(gat.gat_score_var(x, mod.att_proj.weight, mod.att_proj.bias, a, nodes, n1), x, nodes, mod.temp)
    am = (torch.tanh(_lin(mod.att_projM, x * master)) * mod.att_weightM.t()).sum(-1)      # [B, Nmax]: one score row per utterance
    agg_m = gat.gat_softmax_agg_var(am, x, nodes, mod.temp, one_row=True).unsqueeze(1)
    master = _lin(mod.proj_with_attM, agg_m) + _lin(mod.proj_without_attM, master)
    y = bn(_lin(mod.proj_with_att, agg) + _lin(mod.proj_without_att, x), mod.bn, nodes, counts)
    t = torch.where(_rows(n1, k1max).unsqueeze(-1), y[:, :k1max], y.new_zeros(()))
    return t, torch.gather(y, 1, spec.unsqueeze(-1).expand(-1, -1, y.size(2))), master


def _compose(head, feats, frames, train):
    """The back-end on a validated batch -> (logits, last_hidden); see the module docstring.  head: an AasistHead, or the plugin that carries
    its sub-modules and pool_cfg."""
    tb = long_tables(frames, head.pool_cfg)
    dev = feats.device
    cnt = torch.tensor([tb["W"], tb["kT"], tb["kT2"], tb["N1"], tb["N2"]], dtype=torch.int32).to(dev)
    W, kT, kT2, N1, N2 = (cnt[i].contiguous() for i in range(5))
    idx = {k: torch.from_numpy(tb[k]).to(dev) for k in ("cat1", "cat2", "spec1", "spec2")}
    w_max, wl, dt, selu = tb["Wmax"], tb["W"], torch.float32, hipnn.ACT_SELU
    # the mode, bound once (the table in the module docstring)
    if train:
        w_map = feats.shape[1] // POOL
        bn_stack = bn_map = lambda t, bn, act: hipnn.batch_norm_cols_train(t, bn, act, W, counts=wl)          # noqa: E731
        bn_nodes = lambda y, bn, nodes, counts: hipnn.batch_norm(y.unsqueeze(2), bn, selu, valid=nodes, counts=counts).squeeze(2)          # noqa: E731
        conv = lambda c, t: c.conv(t, dt)          # noqa: E731
        zero = lambda t: hipnn.zero_cols(t, W)          # noqa: E731
    else:
        w_map = w_max
        bn_stack = lambda t, bn, act: hipnn.batch_norm_cols(t, bn, act, W)          # noqa: E731
        bn_map = hipnn.batch_norm                                                                     # finite everywhere: not masked
        bn_nodes = lambda y, bn, nodes, counts: hipnn.batch_norm(y, bn, selu)          # noqa: E731
        conv = lambda c, t: c.conv(t, dt, pooled=False)          # noqa: E731
        zero = lambda t: hipnn.zero_cols_(t.contiguous(), W)          # noqa: E731

    # the stack: Residual_block.run's arithmetic, every convolution input exact zeros at and beyond the utterance's columns
    x = bn_stack(hipnn.max_pool3(feats[:, :POOL * w_map].transpose(1, 2)).unsqueeze(-1), head.first_bn, selu)
    for blk in (b[0] for b in head.encoder):
        if train and not blk.first:
            bn_stack(x.detach(), blk.bn1, selu)                                                       # running statistics only
        h = bn_stack(conv(blk.conv1, x), blk.bn2, selu)
        skip = conv(blk.conv_downsample, x) if blk.downsample else x
        x = zero(conv(blk.conv2, h) + skip)
    x = bn_map(x, head.first_bn1, selu)                                                               # [B, 42, w_map, 64]
    a0, a2, a3 = head.attention[0], head.attention[2], head.attention[3]
    w = hipnn.linear(x, a0.weight.view(a0.weight.shape[0], -1), a0.bias)
    w = bn_map(F.selu(w), a2, hipnn.ACT_NONE)
    w = hipnn.linear(w, a3.weight.view(a3.weight.shape[0], -1), a3.bias)
    cols = _rows(W, w_map)
    w_own = torch.where(cols[:, None, :, None], w, w.new_full((), float("-inf")))                     # the soft-max along time: own columns only
    e_S = (x * F.softmax(w_own, dim=2)).sum(2) + head.pos_S
    e_T = (x * F.softmax(w, dim=1)).sum(1)
    e_T = torch.where(cols.unsqueeze(-1), e_T, e_T.new_zeros(()))[:, :w_max]                          # [B, Wmax, 64]
    cols = cols[:, :w_max]

    # the graph module: graph_unfused with per-utterance node counts on the temporal side
    st1 = (idx["cat1"], idx["spec1"], N1, kT, tb["kTmax"], tb["N1"])
    st2 = (idx["cat2"], idx["spec2"], N2, kT2, tb["kT2max"], tb["N2"])
    out_S = head.pool_S(head.GAT_layer_S(e_S))                                                        # 42 -> kS spectral nodes: the same for every utterance
    out_T = _pool_var(head.pool_T, _gat_var(head.GAT_layer_T, e_T, W, wl, bn_nodes), cols, kT, tb["kTmax"])
    res = []
    for l1, l2, pS, pT, m in ((head.HtrgGAT_layer_ST11, head.HtrgGAT_layer_ST12, head.pool_hS1, head.pool_hT1, head.master1),
                              (head.HtrgGAT_layer_ST21, head.HtrgGAT_layer_ST22, head.pool_hS2, head.pool_hT2, head.master2)):
        t, s, mm = _htrg_var(l1, out_T, out_S, m, st1, bn_nodes)
        s, t = pS(s), _pool_var(pT, t, _rows(kT, tb["kTmax"]), kT2, tb["kT2max"])
        t_aug, s_aug, m_aug = _htrg_var(l2, t, s, mm, st2, bn_nodes)
        res.append((head.drop_way(t + t_aug), mm + m_aug, s + s_aug))
    (t1, m1, s1), (t2, m2, s2) = res
    s1, s2, m1, m2 = head.drop_way(s1), head.drop_way(s2), head.drop_way(m1), head.drop_way(m2)
    o_T, o_S, master = torch.max(t1, t2), torch.max(s1, s2), torch.max(m1, m2)                        # o_T: zeros at and beyond kT2_b
    last_hidden = torch.cat([o_T.abs().max(dim=1)[0], o_T.sum(dim=1) / kT2.unsqueeze(1).to(o_T.dtype), o_S.abs().max(dim=1)[0], o_S.mean(dim=1),
                             master.squeeze(1)], dim=1)
    last_hidden = head.drop(last_hidden)
    return _lin(head.out_layer, last_hidden), last_hidden


def _check_frames(head, feats, frames, who, takes):
    if not widths_supported(head):
        raise NotImplementedError("AasistHead.%s: graph-attention widths (in, out) must be among %r (the matrix-core pair-score "
                                  "kernels of csrc/gat.hip)" % (who, GAT_WIDTHS))
    return check_frames(feats, frames, MAX_FRAMES, "%s: the pair-score kernels take at most %d temporal nodes (%d frames each) per utterance"
                        % (takes, GAT_CAP, POOL))


def forward_frames_train(head, feats, frames):
    """Train mode with autograd on: the composition's training column (module docstring) at every length from min_frames() to MAX_FRAMES.
    Batch statistics couple the rows: unlike scoring, row b is NOT what the utterance gets alone, only what it gets in this batch."""
    if not head.training or not torch.is_grad_enabled():
        raise NotImplementedError("AasistHead.forward_frames_train is a training mode: model.train() with autograd on (scoring: forward_frames / "
                                  "forward_frames_long)")
    return _compose(head, feats, _check_frames(head, feats, frames, "forward_frames_train", "forward_frames_train takes"), True)


def forward_frames_long(head, feats, frames):
    """Eval mode under torch.no_grad(): the composition's scoring column (module docstring), up to MAX_FRAMES frames per utterance."""
    if head.training or torch.is_grad_enabled():
        raise NotImplementedError("AasistHead.forward_frames is a scoring mode: model.eval() under torch.no_grad() (training with lengths "
                                  "needs masked batch statistics inside the fused stack)")
    return _compose(head, feats, _check_frames(head, feats, frames, "forward_frames_long", "forward(x, lengths) takes under SCL_AASIST_LENGTHS=long"),
                    False)
