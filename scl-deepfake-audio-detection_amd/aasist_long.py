"""AASIST back-end: variable-length scoring beyond the fused kernels' 242 frames (AasistHead.forward_frames_long, SCL_AASIST_LENGTHS=long).

The contract is forward_frames': feats [B, T, 128] zero-padded, host-side frame counts, eval mode under torch.no_grad(); row b of the result
is what AasistHead.forward gives feats[b:b+1, :frames[b]] alone, and nothing at or beyond an utterance's frames, columns or nodes reaches a
bit of any result (NaN there included).  The execution is the per-layer composition of the fixed-length forward beyond the fused kernels
(Residual_block.run, the torch attention pooling, graph_unfused), with every size that follows the utterance taken from count tables:

  stack      every convolution input is exact zeros at and beyond the utterance's columns W_b = frames // 3, selected and not multiplied:
             hipnn.batch_norm_cols (scl_bn_eval_cols) for the BatchNorm + SELU that feed a convolution, hipnn.zero_cols_ (scl_zero_cols)
             for a block's output.  The map is as wide as the batch's widest utterance; the convolutions' staging maps are not pooled.
  pooling    the soft-max along time runs over the utterance's own columns (the padded logits are replaced by -inf, selected); e_T rows at
             and beyond W_b are replaced by zeros and never reach a result.
  graph      node counts per utterance (node_counts).  The pair scores are scl_gat_score_fwd_var (up to 1024 nodes), soft-max and
             att @ x one kernel (scl_gat_softmax_agg_var: the [N, N] attention matrix never reaches HBM), also for the master node's single
             score row.  A heterogeneous layer's nodes are the ragged [kT_b temporal | kS spectral], packed at the front of the utterance's
             block by a gather through long_tables' index tables, n1 = kT_b.  GraphPool keeps k_b of N_b own nodes: the padded scores are
             replaced by -1 (below every sigmoid) and torch.topk returns descending order, so the first k_b kept nodes and their order
             are the utterance's own.  The read-out's abs-max and mean run over rows that are zero beyond the own kT2_b nodes, the mean
             divided by kT2_b.
torch stays the glue for top-k, gathers and the read-out, as in graph_unfused.  Nothing is kept between calls.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import hipnn, ops
from .aasist_head import POOL, _lin, min_frames, node_counts

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


def _score(x, mod, a, nodes, n1):
    B, N, D = x.shape
    W = mod.att_proj.weight.contiguous().float()
    a3 = torch.zeros(3, W.shape[0], device=x.device, dtype=torch.float32)
    a3[: a.shape[0]] = a
    s = torch.empty(B, N * N, device=x.device, dtype=torch.float32)
    ops.gat_score_fwd_var(x, W, mod.att_proj.bias.contiguous().float(), a3, s, nodes, n1, B, N, D, W.shape[0])
    return s


def _agg(s, x, nodes, temp, one_row=False):
    B, N, D = x.shape
    out = torch.empty((B, D) if one_row else (B, N, D), device=x.device, dtype=torch.float32)
    ops.gat_softmax_agg_var(s, x, nodes, out, B, N, D, temp, one_row)
    return out


def _gat_var(mod, x, nodes):
    """GraphAttentionLayer.forward (eval) on x [B, Nmax, D], rows at and beyond nodes[b] zero; the rows beyond of the result mean nothing."""
    x = x.contiguous()
    agg = _agg(_score(x, mod, mod.att_weight.t(), nodes, None), x, nodes, mod.temp)
    y = _lin(mod.proj_with_att, agg) + _lin(mod.proj_without_att, x)
    return hipnn.batch_norm(y, mod.bn, hipnn.ACT_SELU)


def _pool_var(pool, h, valid, keep, kmax):
    """GraphPool.forward (eval) keeping keep[b] of the utterance's own nodes (valid [B, Nmax]) -> [B, kmax, D], zeros at and beyond keep[b]."""
    scores = torch.sigmoid(_lin(pool.proj, h))
    own = torch.where(valid.unsqueeze(-1), scores, scores.new_full((), -1.0))      # below every sigmoid: a padded node is never among the first keep[b]
    idx = torch.topk(own, kmax, dim=1)[1].expand(-1, -1, h.size(2))
    out = torch.gather(h * scores, 1, idx)
    return torch.where(_rows(keep, kmax).unsqueeze(-1), out, out.new_zeros(()))


def _htrg_var(mod, x1, x2, master, cat, spec, nodes, n1, k1max):
    """HtrgGraphAttentionLayer.forward (eval, master given) on the ragged [n1[b] rows of x1 | x2] -> (temporal [B, k1max, Do] zero at and
    beyond n1[b], spectral [B, nS, Do], master [B, 1, Do])."""
    both = torch.cat([_lin(mod.proj_type1, x1), _lin(mod.proj_type2, x2)], dim=1)
    D = both.size(2)
    x = torch.gather(both, 1, cat.clamp_min(0).unsqueeze(-1).expand(-1, -1, D))
    x = torch.where((cat >= 0).unsqueeze(-1), x, x.new_zeros(())).contiguous()
    a = torch.cat([mod.att_weight11, mod.att_weight22, mod.att_weight12], dim=1).t()
    agg = _agg(_score(x, mod, a, nodes, n1), x, nodes, mod.temp)
    am = (torch.tanh(_lin(mod.att_projM, x * master)) * mod.att_weightM.t()).sum(-1)      # [B, Nmax]: one score row per utterance
    agg_m = _agg(am.contiguous(), x, nodes, mod.temp, one_row=True).unsqueeze(1)
    master = _lin(mod.proj_with_attM, agg_m) + _lin(mod.proj_without_attM, master)
    y = hipnn.batch_norm(_lin(mod.proj_with_att, agg) + _lin(mod.proj_without_att, x), mod.bn, hipnn.ACT_SELU)
    Do = y.size(2)
    t = torch.where(_rows(n1, k1max).unsqueeze(-1), y[:, :k1max], y.new_zeros(()))
    return t, torch.gather(y, 1, spec.unsqueeze(-1).expand(-1, -1, Do)), master


def _check_frames(head, feats, frames, who):
    if not widths_supported(head):
        raise NotImplementedError("AasistHead.%s: graph-attention widths (in, out) must be among %r (the matrix-core pair-score "
                                  "kernels of csrc/gat.hip)" % (who, GAT_WIDTHS))
    frames = [int(t) for t in frames]
    lo = min_frames()
    if len(frames) != feats.shape[0] or not frames or min(frames) < lo or max(frames) > feats.shape[1]:
        raise ValueError("frames: need one count in %d..%d per row of the %r batch, got %r" % (lo, feats.shape[1], tuple(feats.shape), frames))
    if max(frames) > MAX_FRAMES:
        raise ValueError("AASIST back-end: an utterance of %d frames exceeds the %d frames %s takes: the pair-score kernels take at most %d "
                         "temporal nodes (%d frames each) per utterance" % (max(frames), MAX_FRAMES, who, GAT_CAP, POOL))
    return frames


# ---- training on zero-padded batches: the same composition in train mode, with a backward ---------------------------------------------------
def _bn_nodes(y, bn, nodes, counts):
    """Train-mode BatchNorm1d + SELU over the own nodes (b, p < nodes[b]) of y [B, Nmax, D]; zeros beyond."""
    return hipnn.batch_norm(y.unsqueeze(2), bn, hipnn.ACT_SELU, valid=nodes, counts=counts).squeeze(2)


def _gat_var_train(mod, x, nodes, counts):
    from . import gat
    x = mod.input_drop(x).contiguous()
    s = gat.gat_score_var(x, mod.att_proj.weight, mod.att_proj.bias, mod.att_weight.t(), nodes)
    agg = gat.gat_softmax_agg_var(s, x, nodes, mod.temp)
    return _bn_nodes(_lin(mod.proj_with_att, agg) + _lin(mod.proj_without_att, x), mod.bn, nodes, counts)


def _pool_var_train(pool, h, valid, keep, kmax):
    """_pool_var in train mode: the scores come from pool.drop(h), the kept rows from h itself (GraphPool.forward)."""
    scores = torch.sigmoid(_lin(pool.proj, pool.drop(h)))
    own = torch.where(valid.unsqueeze(-1), scores, scores.new_full((), -1.0))
    idx = torch.topk(own.detach(), kmax, dim=1)[1].expand(-1, -1, h.size(2))
    out = torch.gather(h * scores, 1, idx)
    return torch.where(_rows(keep, kmax).unsqueeze(-1), out, out.new_zeros(()))      # selected: the gradient of a padded slot is an exact 0


def _htrg_var_train(mod, x1, x2, master, cat, spec, nodes, n1, k1max, counts):
    from . import gat
    both = torch.cat([_lin(mod.proj_type1, x1), _lin(mod.proj_type2, x2)], dim=1)
    D = both.size(2)
    x = torch.gather(both, 1, cat.clamp_min(0).unsqueeze(-1).expand(-1, -1, D))
    x = mod.input_drop(torch.where((cat >= 0).unsqueeze(-1), x, x.new_zeros(()))).contiguous()
    a = torch.cat([mod.att_weight11, mod.att_weight22, mod.att_weight12], dim=1).t()
    agg = gat.gat_softmax_agg_var(gat.gat_score_var(x, mod.att_proj.weight, mod.att_proj.bias, a, nodes, n1), x, nodes, mod.temp)
    am = (torch.tanh(_lin(mod.att_projM, x * master)) * mod.att_weightM.t()).sum(-1)
    agg_m = gat.gat_softmax_agg_var(am, x, nodes, mod.temp, one_row=True).unsqueeze(1)
    master = _lin(mod.proj_with_attM, agg_m) + _lin(mod.proj_without_attM, master)
    y = _bn_nodes(_lin(mod.proj_with_att, agg) + _lin(mod.proj_without_att, x), mod.bn, nodes, counts)
    t = torch.where(_rows(n1, k1max).unsqueeze(-1), y[:, :k1max], y.new_zeros(()))
    return t, torch.gather(y, 1, spec.unsqueeze(-1).expand(-1, -1, y.size(2))), master


def forward_frames_train(head, feats, frames):
    """Train mode with autograd on: feats [B, T, 128] zero-padded, host-side frame counts -> (logits, last_hidden).  The forward is
    forward_frames_long's with every BatchNorm in train mode: a BatchNorm whose input has a ragged axis takes its mean and biased variance over
    the batch's own positions only (hipnn.batch_norm_cols_train over (b, h, w < W_b) in the stack, first_bn1 and attention.2 included;
    hipnn.batch_norm(valid=) over (b, p < N_b) on the node side, temporal and spectral nodes of a heterogeneous layer together), its running
    statistics move with the unbiased N_v / (N_v - 1) and num_batches_tracked goes up by 1; each non-first block's bn1 moves its running
    statistics only (the reference discards its output); GAT_layer_S, spectral side alone, is unmasked.  Dropout sites are the torch modules
    of the fixed-length per-layer path.  The backward is the exact gradient of that forward: every mask is a selection in front of the op
    whose backward multiplies by its input, so nothing at or beyond an utterance's frames, columns or nodes (NaN included) reaches a bit of
    any output, gradient or buffer, and the rows of d(feats) at and beyond 3 * W_b are exact zeros.
    Batch statistics couple the rows: unlike scoring, row b is NOT what the utterance gets alone, only what it gets in this batch.
    Runs at every length from min_frames() to MAX_FRAMES on the per-layer composition; no fused kernel is involved.  The stack's maps are as
    wide as the padded batch (T // 3 columns), so the convolutions' pooled staging maps are keyed by the run's padded length, not by each
    batch's longest utterance; the graph is as large as the batch's longest utterance."""
    if not head.training or not torch.is_grad_enabled():
        raise NotImplementedError("AasistHead.forward_frames_train is a training mode: model.train() with autograd on (scoring: forward_frames / "
                                  "forward_frames_long)")
    frames = _check_frames(head, feats, frames, "forward_frames_train")
    tb = long_tables(frames, head.pool_cfg)
    dev = feats.device
    cnt = torch.tensor([tb["W"], tb["kT"], tb["kT2"], tb["N1"], tb["N2"]], dtype=torch.int32).to(dev)
    W, kT, kT2, N1, N2 = (cnt[i].contiguous() for i in range(5))
    idx = {k: torch.from_numpy(tb[k]).to(dev) for k in ("cat1", "cat2", "spec1", "spec2")}
    w_map, w_max, wl = feats.shape[1] // POOL, tb["Wmax"], tb["W"]
    bnc = lambda t, bn, act: hipnn.batch_norm_cols_train(t, bn, act, W, counts=wl)          # noqa: E731

    x = bnc(hipnn.max_pool3(feats[:, :POOL * w_map].transpose(1, 2)).unsqueeze(-1), head.first_bn, hipnn.ACT_SELU)
    dt = torch.float32
    for blk in (b[0] for b in head.encoder):
        if not blk.first:
            bnc(x.detach(), blk.bn1, hipnn.ACT_SELU)                                              # running statistics only
        h = bnc(blk.conv1.conv(x, dt), blk.bn2, hipnn.ACT_SELU)
        skip = blk.conv_downsample.conv(x, dt) if blk.downsample else x
        x = hipnn.zero_cols(blk.conv2.conv(h, dt) + skip, W)
    x = bnc(x, head.first_bn1, hipnn.ACT_SELU)                                                    # zeros at and beyond W_b
    a0, a2, a3 = head.attention[0], head.attention[2], head.attention[3]
    w = hipnn.linear(x, a0.weight.view(a0.weight.shape[0], -1), a0.bias)
    w = bnc(F.selu(w), a2, hipnn.ACT_NONE)
    w = hipnn.linear(w, a3.weight.view(a3.weight.shape[0], -1), a3.bias)
    cols = _rows(W, w_map)
    w_own = torch.where(cols[:, None, :, None], w, w.new_full((), float("-inf")))
    e_S = (x * F.softmax(w_own, dim=2)).sum(2) + head.pos_S
    e_T = (x * F.softmax(w, dim=1)).sum(1)
    e_T = torch.where(cols.unsqueeze(-1), e_T, e_T.new_zeros(()))[:, :w_max]                      # [B, Wmax, 64]
    cols = cols[:, :w_max]

    out_S = head.pool_S(head.GAT_layer_S(e_S))
    out_T = _pool_var_train(head.pool_T, _gat_var_train(head.GAT_layer_T, e_T, W, wl), cols, kT, tb["kTmax"])
    res = []
    for l1, l2, pS, pT, m in ((head.HtrgGAT_layer_ST11, head.HtrgGAT_layer_ST12, head.pool_hS1, head.pool_hT1, head.master1),
                              (head.HtrgGAT_layer_ST21, head.HtrgGAT_layer_ST22, head.pool_hS2, head.pool_hT2, head.master2)):
        t, s, mm = _htrg_var_train(l1, out_T, out_S, m, idx["cat1"], idx["spec1"], N1, kT, tb["kTmax"], tb["N1"])
        s, t = pS(s), _pool_var_train(pT, t, _rows(kT, tb["kTmax"]), kT2, tb["kT2max"])
        t_aug, s_aug, m_aug = _htrg_var_train(l2, t, s, mm, idx["cat2"], idx["spec2"], N2, kT2, tb["kT2max"], tb["N2"])
        res.append((head.drop_way(t + t_aug), mm + m_aug, s + s_aug))
    (t1, m1, s1), (t2, m2, s2) = res
    s1, s2, m1, m2 = head.drop_way(s1), head.drop_way(s2), head.drop_way(m1), head.drop_way(m2)
    o_T, o_S, master = torch.max(t1, t2), torch.max(s1, s2), torch.max(m1, m2)
    last_hidden = torch.cat([o_T.abs().max(dim=1)[0], o_T.sum(dim=1) / kT2.unsqueeze(1).to(o_T.dtype), o_S.abs().max(dim=1)[0], o_S.mean(dim=1),
                             master.squeeze(1)], dim=1)
    last_hidden = head.drop(last_hidden)
    return _lin(head.out_layer, last_hidden), last_hidden


def forward_frames_long(head, feats, frames):
    """See the module docstring.  head: an AasistHead, or the plugin that carries its sub-modules and pool_cfg."""
    if head.training or torch.is_grad_enabled():
        raise NotImplementedError("AasistHead.forward_frames is a scoring mode: model.eval() under torch.no_grad() (training with lengths "
                                  "needs masked batch statistics inside the fused stack)")
    if not widths_supported(head):
        raise NotImplementedError("AasistHead.forward_frames_long: graph-attention widths (in, out) must be among %r (the matrix-core pair-score "
                                  "kernels of csrc/gat.hip)" % (GAT_WIDTHS,))
    frames = [int(t) for t in frames]
    lo = min_frames()
    if len(frames) != feats.shape[0] or not frames or min(frames) < lo or max(frames) > feats.shape[1]:
        raise ValueError("frames: need one count in %d..%d per row of the %r batch, got %r" % (lo, feats.shape[1], tuple(feats.shape), frames))
    if max(frames) > MAX_FRAMES:
        raise ValueError("AASIST back-end: an utterance of %d frames exceeds the %d frames forward(x, lengths) takes under SCL_AASIST_LENGTHS=long: "
                         "the pair-score kernels take at most %d temporal nodes (%d frames each) per utterance"
                         % (max(frames), MAX_FRAMES, GAT_CAP, POOL))
    tb = long_tables(frames, head.pool_cfg)
    dev = feats.device
    cnt = torch.tensor([tb["W"], tb["kT"], tb["kT2"], tb["N1"], tb["N2"]], dtype=torch.int32).to(dev)
    W, kT, kT2, N1, N2 = (cnt[i].contiguous() for i in range(5))
    idx = {k: torch.from_numpy(tb[k]).to(dev) for k in ("cat1", "cat2", "spec1", "spec2")}
    w_max = tb["Wmax"]

    # the stack: Residual_block.run's arithmetic, every convolution input exact zeros at and beyond the utterance's columns
    x = hipnn.max_pool3(feats[:, :POOL * w_max].transpose(1, 2)).unsqueeze(-1)
    x = hipnn.batch_norm_cols(x, head.first_bn, hipnn.ACT_SELU, W)
    dt = torch.float32
    for blk in (b[0] for b in head.encoder):
        h = hipnn.batch_norm_cols(blk.conv1.conv(x, dt, pooled=False), blk.bn2, hipnn.ACT_SELU, W)
        skip = blk.conv_downsample.conv(x, dt, pooled=False) if blk.downsample else x
        x = hipnn.zero_cols_((blk.conv2.conv(h, dt, pooled=False) + skip).contiguous(), W)
    x = hipnn.batch_norm(x, head.first_bn1, hipnn.ACT_SELU)                                       # [B, 42, Wmax, 64]: finite everywhere
    a0, a2, a3 = head.attention[0], head.attention[2], head.attention[3]
    w = hipnn.linear(x, a0.weight.view(a0.weight.shape[0], -1), a0.bias)
    w = hipnn.batch_norm(F.selu(w), a2, hipnn.ACT_NONE)
    w = hipnn.linear(w, a3.weight.view(a3.weight.shape[0], -1), a3.bias)
    cols = _rows(W, w_max)                                                                        # [B, Wmax]
    w_own = torch.where(cols[:, None, :, None], w, w.new_full((), float("-inf")))                 # the soft-max along time: own columns only
    e_S = (x * F.softmax(w_own, dim=2)).sum(2) + head.pos_S
    e_T = (x * F.softmax(w, dim=1)).sum(1)
    e_T = torch.where(cols.unsqueeze(-1), e_T, e_T.new_zeros(()))                                 # [B, Wmax, 64]

    # the graph module: graph_unfused with per-utterance node counts on the temporal side
    out_S = head.pool_S(head.GAT_layer_S(e_S))                                                    # 42 -> kS spectral nodes: the same for every utterance
    out_T = _pool_var(head.pool_T, _gat_var(head.GAT_layer_T, e_T, W), cols, kT, tb["kTmax"])
    res = []
    for l1, l2, pS, pT, m in ((head.HtrgGAT_layer_ST11, head.HtrgGAT_layer_ST12, head.pool_hS1, head.pool_hT1, head.master1),
                              (head.HtrgGAT_layer_ST21, head.HtrgGAT_layer_ST22, head.pool_hS2, head.pool_hT2, head.master2)):
        t, s, mm = _htrg_var(l1, out_T, out_S, m, idx["cat1"], idx["spec1"], N1, kT, tb["kTmax"])
        s, t = pS(s), _pool_var(pT, t, _rows(kT, tb["kTmax"]), kT2, tb["kT2max"])
        t_aug, s_aug, m_aug = _htrg_var(l2, t, s, mm, idx["cat2"], idx["spec2"], N2, kT2, tb["kT2max"])
        res.append((t + t_aug, mm + m_aug, s + s_aug))
    (t1, m1, s1), (t2, m2, s2) = res
    o_T, o_S, master = torch.max(t1, t2), torch.max(s1, s2), torch.max(m1, m2)                    # o_T: zeros at and beyond kT2_b
    last_hidden = torch.cat([o_T.abs().max(dim=1)[0], o_T.sum(dim=1) / kT2.unsqueeze(1).to(o_T.dtype), o_S.abs().max(dim=1)[0], o_S.mean(dim=1),
                             master.squeeze(1)], dim=1)
    return _lin(head.out_layer, last_hidden), last_hidden
