"""AASIST variable-length scoring beyond 242 frames (SCL_AASIST_LENGTHS=long), the parts that need no GPU: the switch's limits, the count
and index tables of aasist_long.long_tables against node_counts, the DEFINITION of the batched masked composition - an fp64 restatement on
the oracle's state-dict names of what aasist_long.forward_frames_long runs (convolution inputs zeroed by selection at and beyond an
utterance's columns, the soft-max along time over the own columns, masked soft-max + aggregation over the own nodes, the ragged
[kT_b temporal | kS spectral] node order through the index tables, GraphPool's per-utterance top-k with padded scores replaced by -1, the
read-out over the own nodes) against oracle/aasist_head.AasistHead on each utterance alone - and the refusals.

The bar is the one tests/test_aasist_varlen_cpu.py states for its definition: both sides are fp64, the test prints the worst difference and
asserts it below 1e-10 (there 1.2e-14 measured; here 1.6e-14)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from scl_amd import aasist_head as AH
from scl_amd import aasist_long as AL
from scl_amd import pack
from test_aasist_varlen_cpu import TEMPS, _bn, _bn_nodes, _lin, _oracle

FRAMES = [243, 282, 283, 387, 390, 773, 776, 100, 3]


# ---- the switch -----------------------------------------------------------------------------------------------------------------------------
def _bare_model():
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_aasist import Model
    m = Model.__new__(Model)      # the limits read the configuration alone: no device, no parameters
    m.__dict__.update(cfg=W2VConfig(), pool_cfg={"pool_ratios": [0.5, 0.5, 0.5, 0.5]})
    return m


def test_long_switch_limits(monkeypatch):
    m = _bare_model()
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
    assert m.head_takes_frames is True
    assert m.head_max_frames() == 3 * 1024 + 2 == 3074 == AL.MAX_FRAMES
    assert m.max_samples() == pack.VARLEN_MAX_SAMPLES == 960000 and m.min_samples() == 1040
    assert m.cfg.conv_lens(960000)[-1] == 2999 and AH.node_counts([2999])["W"] == [999]
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    assert m.head_takes_frames is True and m.head_max_frames() == 242 and m.max_samples() == 77839 and m.min_samples() == 1040
    assert AH.max_frames() == 242
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "yes")      # not a value of the switch
    assert m.head_takes_frames is False
    monkeypatch.delenv("SCL_AASIST_LENGTHS")
    assert m.head_takes_frames is False and AH.max_frames() == 242


def test_main_takes_the_long_value_as_the_switch_being_on(monkeypatch):
    import main as M
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
    assert M._scores_varlen("wav2vec2_aasist")
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "0")
    assert not M._scores_varlen("wav2vec2_aasist")


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
def test_long_tables_equal_node_counts_and_every_index_range_is_disjoint_and_inside_its_block():
    tb, c = AL.long_tables(FRAMES), AH.node_counts(FRAMES)
    for k, v in c.items():
        assert tb[k] == v, k
    assert c["W"] == [81, 94, 94, 129, 130, 257, 258, 33, 1] and c["N1"][5:7] == [149, 150] and c["kT"][5:7] == [128, 129]
    assert (tb["Wmax"], tb["kTmax"], tb["kT2max"], tb["N1max"], tb["N2max"]) == (258, 129, 64, 150, 74)
    for cat, spec, kt, ks, n in ((tb["cat1"], tb["spec1"], c["kT"], c["kS"], c["N1"]), (tb["cat2"], tb["spec2"], c["kT2"], c["kS2"], c["N2"])):
        ktm, B = max(kt), len(FRAMES)
        assert cat.shape == (B, ktm + ks) and spec.shape == (B, ks) and cat.dtype == spec.dtype == np.int64
        for b in range(B):
            temporal, spectral = np.arange(kt[b]), spec[b]
            assert n[b] == kt[b] + ks and spectral.min() == kt[b] and spectral.max() == n[b] - 1 < cat.shape[1]      # inside the block
            assert not set(temporal) & set(spectral) and sorted(set(temporal) | set(spectral)) == list(range(n[b]))  # disjoint, packed at the front
            assert (cat[b, temporal] == temporal).all() and (cat[b, spectral] == ktm + np.arange(ks)).all()          # rows of cat([temporal, spectral], 1)
            assert (cat[b, n[b]:] == -1).all() and (cat[b, :n[b]] >= 0).all()


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def _rows(count, n):
    return torch.arange(n)[None, :] < torch.as_tensor(count)[:, None]


def _agg(s, x, nodes, temp):
    """softmax over the own nodes j < nodes[b] of s [B, R, N] / temp, times x [B, N, D] (padded scores and rows replaced, not multiplied)."""
    own = _rows(nodes, x.shape[1])
    p = F.softmax(torch.where(own[:, None, :], s / temp, torch.full((), float("-inf"), dtype=s.dtype)), dim=-1)
    return p @ torch.where(own[..., None], x, torch.zeros((), dtype=x.dtype))


def _gat_var(t, p, x, nodes, temp):
    s = (torch.tanh(_lin(t, p + "att_proj", x.unsqueeze(2) * x.unsqueeze(1))) @ t[p + "att_weight"]).squeeze(-1)
    return F.selu(_bn_nodes(t, p + "bn", _lin(t, p + "proj_with_att", _agg(s, x, nodes, temp)) + _lin(t, p + "proj_without_att", x)))


def _pool_var(t, p, h, valid, keep, kmax):
    s = torch.sigmoid(_lin(t, p + "proj", h))
    own = torch.where(valid[..., None], s, torch.full((), -1.0, dtype=s.dtype))
    idx = torch.topk(own, kmax, dim=1)[1].expand(-1, -1, h.shape[2])
    return torch.where(_rows(keep, kmax)[..., None], torch.gather(h * s, 1, idx), torch.zeros((), dtype=h.dtype))


def _htrg_var(t, p, x1, x2, master, cat, spec, nodes, n1, k1max, temp):
    cat, spec = torch.from_numpy(cat), torch.from_numpy(spec)
    both = torch.cat([_lin(t, p + "proj_type1", x1), _lin(t, p + "proj_type2", x2)], dim=1)
    x = torch.gather(both, 1, cat.clamp_min(0)[..., None].expand(-1, -1, both.shape[2]))
    x = torch.where((cat >= 0)[..., None], x, torch.zeros((), dtype=x.dtype))
    h = torch.tanh(_lin(t, p + "att_proj", x.unsqueeze(2) * x.unsqueeze(1)))
    first = _rows(n1, x.shape[1])
    same = first[:, :, None] == first[:, None, :]
    a = torch.where(same[..., None], torch.where(first[:, :, None, None], t[p + "att_weight11"][:, 0], t[p + "att_weight22"][:, 0]), t[p + "att_weight12"][:, 0])
    agg = _agg((h * a).sum(-1), x, nodes, temp)
    am = (torch.tanh(_lin(t, p + "att_projM", x * master)) @ t[p + "att_weightM"]).squeeze(-1)      # one score row per utterance
    m_out = _lin(t, p + "proj_with_attM", _agg(am[:, None, :], x, nodes, temp)) + _lin(t, p + "proj_without_attM", master)
    y = F.selu(_bn_nodes(t, p + "bn", _lin(t, p + "proj_with_att", agg) + _lin(t, p + "proj_without_att", x)))
    t_out = torch.where(_rows(n1, k1max)[..., None], y[:, :k1max], torch.zeros((), dtype=y.dtype))
    return t_out, torch.gather(y, 1, spec[..., None].expand(-1, -1, y.shape[2])), m_out


def _long_definition(t, feats, frames):
    tb = AL.long_tables(frames)
    Wmax, zero = tb["Wmax"], torch.zeros((), dtype=feats.dtype)
    cols = _rows(tb["W"], Wmax)
    mask = lambda x: torch.where(cols[:, None, None, :], x, zero)
    conv = lambda x, p, pad: F.conv2d(x, t[p + ".weight"], t[p + ".bias"], padding=pad)
    x = feats[:, :3 * Wmax].transpose(1, 2).unsqueeze(1)
    x = mask(F.selu(_bn(t, "first_bn", F.max_pool2d(x, (3, 3)))))
    for i in range(6):
        p = "encoder.%d.0." % i
        a = mask(F.selu(_bn(t, p + "bn2", conv(x, p + "conv1", (1, 1)))))
        idn = conv(x, p + "conv_downsample", (0, 1)) if (p + "conv_downsample.weight") in t else x
        x = mask(conv(a, p + "conv2", (0, 1)) + idn)
    x = F.selu(_bn(t, "first_bn1", x))
    w = conv(_bn(t, "attention.2", F.selu(conv(x, "attention.0", 0))), "attention.3", 0)
    w_own = torch.where(cols[:, None, None, :], w, torch.full((), float("-inf"), dtype=w.dtype))
    e_S = (x * F.softmax(w_own, dim=-1)).sum(-1).transpose(1, 2) + t["pos_S"]
    e_T = torch.where(cols[..., None], (x * F.softmax(w, dim=-2)).sum(-2).transpose(1, 2), zero)

    from test_aasist_varlen_cpu import _gat, _pool
    out_S = _pool(t, "pool_S.", _gat(t, "GAT_layer_S.", e_S, TEMPS[0]), tb["kS"])
    out_T = _pool_var(t, "pool_T.", _gat_var(t, "GAT_layer_T.", e_T, tb["W"], TEMPS[1]), cols, tb["kT"], tb["kTmax"])
    res = []
    for l1, l2, pS, pT, m in (("HtrgGAT_layer_ST11.", "HtrgGAT_layer_ST12.", "pool_hS1.", "pool_hT1.", "master1"),
                              ("HtrgGAT_layer_ST21.", "HtrgGAT_layer_ST22.", "pool_hS2.", "pool_hT2.", "master2")):
        tt, ss, mm = _htrg_var(t, l1, out_T, out_S, t[m], tb["cat1"], tb["spec1"], tb["N1"], tb["kT"], tb["kTmax"], TEMPS[2])
        ss, tt = _pool(t, pS, ss, tb["kS2"]), _pool_var(t, pT, tt, _rows(tb["kT"], tb["kTmax"]), tb["kT2"], tb["kT2max"])
        ta, sa, ma = _htrg_var(t, l2, tt, ss, mm, tb["cat2"], tb["spec2"], tb["N2"], tb["kT2"], tb["kT2max"], TEMPS[2])
        res.append((tt + ta, ss + sa, mm + ma))
    T_, S_, M_ = (torch.max(res[0][i], res[1][i]) for i in range(3))
    hid = torch.cat([T_.abs().max(dim=1)[0], T_.sum(dim=1) / torch.tensor(tb["kT2"], dtype=T_.dtype)[:, None], S_.abs().max(dim=1)[0], S_.mean(dim=1),
                     M_.squeeze(1)], dim=1)
    return _lin(t, "out_layer", hid), hid


def test_the_batched_masked_composition_equals_the_oracle_on_each_utterance_alone():
    ref = _oracle()
    t = {k: v for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(110)
    T = 800
    feats = torch.zeros(len(FRAMES), T, 128, dtype=torch.float64)
    for b, n in enumerate(FRAMES):
        feats[b, :n] = torch.randn(n, 128, generator=g).double()
        feats[b, n:] = 1e3 * torch.randn(T - n, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(b))      # junk, not zeros
    with torch.no_grad():
        logits, hid = _long_definition(t, feats, FRAMES)
        worst = 0.0
        for b, n in enumerate(FRAMES):
            rl, rh = ref(feats[b:b + 1, :n])
            worst = max(worst, (logits[b] - rl[0]).abs().max().item(), (hid[b] - rh[0]).abs().max().item())
        # the comparison can fail: with every utterance taken at the batch's width the short rows move
        full = _long_definition(t, feats, [max(FRAMES)] * len(FRAMES))[0]
    print("batched masked composition against the oracle alone: %.2e" % worst)
    assert worst < 1e-10
    assert (full[-1] - logits[-1]).abs().max().item() > 1e-3


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_forward_frames_long_refuses_train_mode_autograd_too_many_frames_and_other_widths():
    head = AH.AasistHead()
    feats = torch.zeros(2, 3080, 128)
    head.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
        head.forward_frames_long(feats, [300, 100])
    head.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):      # autograd on
        head.forward_frames_long(feats, [300, 100])
    with torch.no_grad():
        with pytest.raises(ValueError, match="exceeds the 3074 frames"):
            head.forward_frames_long(feats, [3075, 100])
        with pytest.raises(ValueError, match="3..3080"):
            head.forward_frames_long(feats, [300, 2])
        with pytest.raises(ValueError):
            head.forward_frames_long(feats, [300])
        odd = AH.AasistHead(dict(AH.UPSTREAM_AASIST, gat_dims=[48, 32])).eval()
        assert AL.widths_supported(head) and not AL.widths_supported(odd)
        with pytest.raises(NotImplementedError, match="widths"):
            odd.forward_frames_long(feats, [300, 100])
    for dims in ([64, 64], [32, 32]):
        assert AL.widths_supported(AH.AasistHead(dict(AH.UPSTREAM_AASIST, gat_dims=dims)))


def test_the_long_path_does_not_ask_for_the_fused_kernels(monkeypatch):
    """SCL_AASIST_FUSED=0 refuses forward_frames (tests/test_aasist_varlen_cpu.py); forward_frames_long gets past every refusal, to the
    tables that are the first thing behind them."""
    class Reached(Exception):
        pass

    def tables(*a, **k):
        raise Reached()
    head = AH.AasistHead().eval()
    monkeypatch.setattr(AH, "FUSED_STACK", False)      # what SCL_AASIST_FUSED=0 / SCL_AASIST_FUSED_GRAPH=0 set at import
    monkeypatch.setattr(AH, "FUSED_GRAPH", False)
    monkeypatch.setattr(AL, "long_tables", tables)
    with torch.no_grad(), pytest.raises(Reached):
        head.forward_frames_long(torch.zeros(1, 300, 128), [300])
