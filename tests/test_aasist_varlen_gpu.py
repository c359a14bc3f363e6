"""Variable-length scoring batches on the `wav2vec2_aasist` plugin (SCL_AASIST_LENGTHS=1): every masked kernel against its fixed-length
neighbour on each utterance alone, the back-end (AasistHead.forward_frames) against the fixed-length fused forward and the fp64 oracle on
each utterance alone, the whole plugin (both scoring precisions, both row layouts) against itself on each utterance alone, the refusals,
the bound on live plans, and main.py --eval --padding_type none.

Bounds.  Kernel level and back-end: 2e-5 of the reference tensor's largest magnitude (what tests/test_aasist_gpu.py holds the fused path
to).  Plugin: tests/test_resnet_varlen_gpu.py's for the same comparison on its plugin."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import aasist_head as AH  # noqa: E402
from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import graph, ops, resstack  # noqa: E402
from scl_amd import lib as L  # noqa: E402
from scl_amd import model_front as MF  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.model_aasist import Model  # noqa: E402
from oracle import aasist_head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402

NAN = float("nan")
TOL = 2e-5
WIDTHS = [80, 1, 2, 20, 66, 65]                          # map widths / temporal node counts of the kernel-level batches
FRAMES = [3, 5, 6, 61, 199, 200, 201, 242, 100, 8]       # the back-end batch: both T = 3 W + 2 cases, one and two nodes, the limit
SEED = 101      # the fp64 GraphPool gap of this batch: 1.6e-5 (100 gives 6.5e-7, below the precondition)
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)   # 64-wide heads
ARGS = {"contra_mode": "all", "loss_type": 1, "aasist": AH.UPSTREAM_AASIST}


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. the stack's kernels ------------------------------------------------------------------------------------------------------------
class Map:
    """A zero-bordered flat map [B, H + 2, W + 2, C] with the slack resstack.hip reads on either side."""

    def __init__(self, B, H, W, C, dev, fill=0.0):
        self.B, self.H, self.W, self.C = B, H, W, C
        self.G = B * (H + 2) * (W + 2)
        self.slack = W + 2 + 2 + 256 + 6
        self.buf = torch.zeros((self.G + 2 * self.slack) * C, device=dev)
        self.v = self.buf[self.slack * C: (self.slack + self.G) * C].view(B, H + 2, W + 2, C)
        if fill != 0.0:
            self.v.fill_(fill)
        self.ptr = self.buf.data_ptr() + 4 * self.slack * C


def _geom(B, H, W, r_lo, r_hi):
    return L.SclRsGeom(B, H, W, r_lo, r_hi, 0)


H = 42


def test_masked_copy_selects_an_utterances_columns_and_zeros_the_rest(dev):
    B, Ws = len(WIDTHS), max(WIDTHS)
    clean = torch.randn(B, H, Ws, 1, generator=torch.Generator().manual_seed(1))
    src = clean.clone()
    for b, w in enumerate(WIDTHS):
        src[b, :, w:] = NAN
    out, out0 = Map(B, H, Ws, 16, dev, fill=7.0), Map(B, H, Ws, 16, dev, fill=7.0)
    wt = i32(WIDTHS, dev)
    g = _geom(B, H, Ws, 1, H)
    s_d, c_d = src.to(dev), torch.where(torch.isnan(src), torch.zeros(()), src).to(dev)
    ops._call("scl_rs_copy_w", s_d.data_ptr(), out.ptr, 1, 16, Ws, ctypes.byref(g), wt.data_ptr(), S())
    ops._call("scl_rs_copy_w", c_d.data_ptr(), out0.ptr, 1, 16, Ws, ctypes.byref(g), wt.data_ptr(), S())
    torch.cuda.synchronize()
    assert torch.equal(out.v, out0.v) and torch.isfinite(out.v).all()      # NaN in the padding: the same bits
    for b, w in enumerate(WIDTHS):
        alone = Map(1, H, w, 16, dev, fill=7.0)
        one = clean[b:b + 1, :, :w].contiguous().to(dev)
        ga = _geom(1, H, w, 1, H)
        ops._call("scl_rs_copy", one.data_ptr(), alone.ptr, 1, 16, 0, ctypes.byref(ga), S())
        torch.cuda.synchronize()
        assert torch.equal(out.v[b, 1:H + 1, 1:w + 1], alone.v[0, 1:H + 1, 1:w + 1]), (b, w)
        rest = out.v[b].clone()
        rest[1:H + 1, 1:w + 1] = 0
        assert (rest == 0).all(), (b, w)      # borders, other channels and every column beyond the width
    # a narrower source than the map (the widest utterance of a batch below the plan's rounded width)
    out2 = Map(B, H, Ws + 8, 16, dev, fill=7.0)
    g2 = _geom(B, H, Ws + 8, 1, H)
    ops._call("scl_rs_copy_w", s_d.data_ptr(), out2.ptr, 1, 16, Ws, ctypes.byref(g2), wt.data_ptr(), S())
    torch.cuda.synchronize()
    assert torch.equal(out2.v[:, :, :Ws + 1], out.v[:, :, :Ws + 1]) and (out2.v[:, :, Ws + 1:] == 0).all()


def _pack(w, cinp, coutp, dev):
    nt = w.shape[2] * w.shape[3]
    out = torch.empty(coutp * nt * cinp, device=dev)
    arr = (L.SclRsPackJob * 1)()
    arr[0] = L.SclRsPackJob(w.data_ptr(), out.data_ptr(), w.shape[0], w.shape[1], nt, cinp, coutp, 0, 0, 0)
    ops._call("scl_rs_pack_weights", arr, 1, S(), keep=arr)
    return out


def _conv(name, inp, wpk, bias, addend, out, geom, shifts, cin, cout, wt=None):
    d = L.SclRsConv()
    d.inp, d.wpk, d.out, d.bias, d.addend = inp, wpk.data_ptr(), out, bias.data_ptr(), addend
    d.geom = geom
    for i, s in enumerate(shifts):
        d.shift[i] = s
    d.cin, d.cout, d.ntaps = cin, cout, len(shifts)
    if wt is None:
        ops._call("scl_rs_conv", ctypes.byref(d), S(), keep=d)
    else:
        ops._call("scl_rs_conv_w", ctypes.byref(d), wt.data_ptr(), S(), keep=d)


def test_masked_convolution_32_to_64_six_taps(dev):
    """conv1's form: six taps, rows 0..H.  The data input is a masked map by contract (the kernel before wrote zeros at and beyond the
    width: the first column beyond it IS the convolution's padding); NaN goes everywhere no tap of a valid output reaches — the input
    columns from the second one beyond the width — and into the whole padding of the addend."""
    B, Ws, cin, cout = len(WIDTHS), max(WIDTHS), 32, 64
    gen = torch.Generator().manual_seed(2)
    w = (torch.randn(cout, cin, 2, 3, generator=gen) / np.sqrt(6 * cin)).to(dev)
    bias = (0.1 * torch.randn(cout, generator=gen)).to(dev)
    wpk = _pack(w, cin, cout, dev)
    x, ad = Map(B, H, Ws, cin, dev), Map(B, H, Ws, cout, dev)
    xv, av = torch.randn(B, H, Ws, cin, generator=gen), torch.randn(B, H + 1, Ws, cout, generator=gen)
    for b, wd in enumerate(WIDTHS):
        x.v[b, 1:H + 1, 1:wd + 1] = xv[b, :, :wd].to(dev)
        ad.v[b, 0:H + 1, 1:wd + 1] = av[b, :, :wd].to(dev)
    xn, adn = Map(B, H, Ws, cin, dev), Map(B, H, Ws, cout, dev, fill=NAN)
    xn.v.copy_(x.v)
    for b, wd in enumerate(WIDTHS):
        xn.v[b, :, wd + 2:] = NAN
        adn.v[b, 0:H + 1, 1:wd + 1] = ad.v[b, 0:H + 1, 1:wd + 1]
    wt = i32(WIDTHS, dev)
    shifts = lambda Wp: [kh * Wp + kw - 1 for kh in (0, 1) for kw in (0, 1, 2)]
    g = _geom(B, H, Ws, 0, H)
    out, outn = Map(B, H, Ws, cout, dev, fill=7.0), Map(B, H, Ws, cout, dev, fill=7.0)
    _conv("w", x.ptr, wpk, bias, ad.ptr, out.ptr, g, shifts(Ws + 2), cin, cout, wt)
    _conv("w", xn.ptr, wpk, bias, adn.ptr, outn.ptr, g, shifts(Ws + 2), cin, cout, wt)
    torch.cuda.synchronize()
    assert torch.isfinite(outn.v).all() and torch.equal(out.v, outn.v)
    worst = 0.0
    for b, wd in enumerate(WIDTHS):
        xa, aa, oa = Map(1, H, wd, cin, dev), Map(1, H, wd, cout, dev), Map(1, H, wd, cout, dev, fill=7.0)
        xa.v[0, 1:H + 1, 1:wd + 1] = xv[b, :, :wd].to(dev)
        aa.v[0, 0:H + 1, 1:wd + 1] = av[b, :, :wd].to(dev)
        _conv("fixed", xa.ptr, wpk, bias, aa.ptr, oa.ptr, _geom(1, H, wd, 0, H), shifts(wd + 2), cin, cout)
        torch.cuda.synchronize()
        err = maxrel(out.v[b, 0:H + 1, 1:wd + 1], oa.v[0, 0:H + 1, 1:wd + 1])
        worst = max(worst, err)
        assert err <= TOL, (b, wd, err)
        rest = out.v[b].clone()
        rest[0:H + 1, 1:wd + 1] = 0
        assert (rest == 0).all(), (b, wd)
    print("masked convolution against the fixed-length one alone: worst %.2e" % worst)


def test_masked_bn_act(dev):
    B, Ws, C = len(WIDTHS), max(WIDTHS), 64
    gen = torch.Generator().manual_seed(3)
    stats = torch.cat([0.2 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen), 0.5 + torch.rand(C, generator=gen),
                       0.3 * torch.randn(C, generator=gen)]).to(dev)
    yv = torch.randn(B, H, Ws, C, generator=gen)
    y, yn = Map(B, H, Ws, C, dev, fill=5.0), Map(B, H, Ws, C, dev, fill=NAN)
    for b, wd in enumerate(WIDTHS):
        y.v[b, 1:H + 1, 1:wd + 1] = yv[b, :, :wd].to(dev)
        yn.v[b, 1:H + 1, 1:wd + 1] = yv[b, :, :wd].to(dev)
    wt = i32(WIDTHS, dev)
    g = _geom(B, H, Ws, 1, H)
    for act in (1, 0):
        a, an = Map(B, H, Ws, C, dev, fill=7.0), Map(B, H, Ws, C, dev, fill=7.0)
        ops._call("scl_rs_bn_act_w", y.ptr, stats.data_ptr(), a.ptr, C, act, ctypes.byref(g), wt.data_ptr(), S())
        ops._call("scl_rs_bn_act_w", yn.ptr, stats.data_ptr(), an.ptr, C, act, ctypes.byref(g), wt.data_ptr(), S())
        torch.cuda.synchronize()
        assert torch.isfinite(an.v).all() and torch.equal(a.v, an.v)
        for b, wd in enumerate(WIDTHS):
            ya, aa = Map(1, H, wd, C, dev), Map(1, H, wd, C, dev, fill=7.0)
            ya.v[0, 1:H + 1, 1:wd + 1] = yv[b, :, :wd].to(dev)
            ga = _geom(1, H, wd, 1, H)
            ops._call("scl_rs_bn_act", ya.ptr, stats.data_ptr(), aa.ptr, C, act, ctypes.byref(ga), S())
            torch.cuda.synchronize()
            assert maxrel(a.v[b, 1:H + 1, 1:wd + 1], aa.v[0, 1:H + 1, 1:wd + 1]) <= TOL, (act, b, wd)
            rest = a.v[b].clone()
            rest[1:H + 1, 1:wd + 1] = 0
            assert (rest == 0).all(), (act, b, wd)      # selu(bn(0)) is not 0: the zeros are selected


def test_masked_attention_pooling(dev):
    B, Ws, C = len(WIDTHS), max(WIDTHS), 64
    gen = torch.Generator().manual_seed(4)
    xv, lv = torch.randn(B, H, Ws, C, generator=gen), 2.0 * torch.randn(B, H, Ws, C, generator=gen)
    pos = torch.randn(H, C, generator=gen).to(dev)
    maps = {}
    for tag, fill in (("zero", 0.0), ("nan", NAN)):
        x, l = Map(B, H, Ws, C, dev, fill=fill), Map(B, H, Ws, C, dev, fill=fill)
        for b, wd in enumerate(WIDTHS):
            x.v[b, 1:H + 1, 1:wd + 1] = xv[b, :, :wd].to(dev)
            l.v[b, 1:H + 1, 1:wd + 1] = lv[b, :, :wd].to(dev)
        eS, eT = torch.full((B, H, C), 7.0, device=dev), torch.full((B, Ws, C), 7.0, device=dev)
        g = _geom(B, H, Ws, 1, H)
        ops._call("scl_rs_attn_pool_fwd_w", x.ptr, l.ptr, pos.data_ptr(), eS.data_ptr(), eT.data_ptr(), C, ctypes.byref(g), i32(WIDTHS, dev).data_ptr(), S())
        torch.cuda.synchronize()
        maps[tag] = (eS, eT)
    (eS, eT), (eSn, eTn) = maps["zero"], maps["nan"]
    assert torch.isfinite(eSn).all() and torch.isfinite(eTn).all() and torch.equal(eS, eSn) and torch.equal(eT, eTn)
    for b, wd in enumerate(WIDTHS):
        xa, la = Map(1, H, wd, C, dev), Map(1, H, wd, C, dev)
        xa.v[0, 1:H + 1, 1:wd + 1] = xv[b, :, :wd].to(dev)
        la.v[0, 1:H + 1, 1:wd + 1] = lv[b, :, :wd].to(dev)
        aS, aT = torch.empty(1, H, C, device=dev), torch.empty(1, wd, C, device=dev)
        ga = _geom(1, H, wd, 1, H)
        ops._call("scl_rs_attn_pool_fwd", xa.ptr, la.ptr, pos.data_ptr(), aS.data_ptr(), aT.data_ptr(), C, ctypes.byref(ga), S())
        torch.cuda.synchronize()
        assert maxrel(eS[b], aS[0]) <= TOL and maxrel(eT[b, :wd], aT[0]) <= TOL, (b, wd)
        assert (eT[b, wd:] == 0).all(), (b, wd)      # the graph module's input copy reads these rows


# ---- 2. the pair scores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["homogeneous", "heterogeneous"])
def test_pair_scores_of_graphs_of_different_sizes(dev, kind):
    cnt = AH.node_counts([3 * w for w in WIDTHS])
    if kind == "homogeneous":
        D, Do, nodes, n1 = 64, 64, cnt["W"], None
    else:
        D, Do, nodes, n1 = 64, 32, cnt["N1"], cnt["kT"]      # HtrgGAT_layer_ST11: kT_b temporal nodes in front of the 21 spectral ones
    B, Nmax = len(nodes), max(nodes)
    gen = torch.Generator().manual_seed(5)
    Wm, bias, a = (torch.randn(Do, D, generator=gen) / 8).to(dev), (0.1 * torch.randn(Do, generator=gen)).to(dev), torch.randn(3, Do, generator=gen).to(dev)
    xv = torch.randn(B, Nmax, D, generator=gen)
    res = []
    for fill in (0.0, NAN):
        x = xv.clone()
        for b, n in enumerate(nodes):
            x[b, n:] = fill
        s = torch.full((B, Nmax, Nmax), 7.0, device=dev)
        ops.gat_score_fwd_var(x.to(dev), Wm, bias, a, s, i32(nodes, dev), None if n1 is None else i32(n1, dev), B, Nmax, D, Do)
        torch.cuda.synchronize()
        res.append(s)
    assert torch.isfinite(res[1]).all() and torch.equal(res[0], res[1])
    for b, n in enumerate(nodes):
        alone = torch.empty(1, n, n, device=dev)
        ops.gat_score_fwd(xv[b:b + 1, :n].contiguous().to(dev), Wm, bias, a, alone, 1, n, D, Do, n if n1 is None else n1[b])
        torch.cuda.synchronize()
        got = res[0][b].flatten()
        assert maxrel(got[:n * n].view(n, n), alone[0]) <= TOL, (kind, b, n)
        assert (got[n * n:] == 7.0).all(), (kind, b, n)      # nothing is written beyond the utterance's own matrix


# ---- 3. the graph module's kernels -----------------------------------------------------------------------------------------------------
def _filled_head(dev, seed=3):
    head = AH.AasistHead()
    sd = fill_state({k: tuple(v.shape) for k, v in head.state_dict().items()}, seed=seed)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return head.to(dev).eval(), sd


@pytest.fixture(scope="module")
def graph_case(dev):
    """One plan of the padded batch (temporal node counts WIDTHS) and one fixed-length plan per utterance alone, both run once: the fixed
    plans then hold every launch's inputs and outputs for their utterance."""
    head, _ = _filled_head(dev)
    cnt = AH.node_counts([3 * w for w in WIDTHS])
    B, nT = len(WIDTHS), max(WIDTHS)
    gen = torch.Generator().manual_seed(6)
    e_S, e_T = torch.randn(B, 42, 64, generator=gen).to(dev), torch.randn(B, nT, 64, generator=gen).to(dev)
    with torch.no_grad():
        pl = graph._Plan(head, B, 42, nT, dev, counts=True)
        pl.cnt.copy_(torch.tensor([cnt["W"], cnt["kT"], cnt["kT2"], cnt["N1"], cnt["N2"]], dtype=torch.int32))
        graph._forward(pl, head, e_S, e_T, False)
        alone = []
        for b, w in enumerate(WIDTHS):
            pb = graph._Plan(head, 1, 42, w, dev)
            out = graph._forward(pb, head, e_S[b:b + 1].contiguous(), e_T[b:b + 1, :w].contiguous(), False)
            alone.append((pb, out))
        torch.cuda.synchronize()
    return head, cnt, pl, alone


def _rows(cnt, name, b):
    return {"S": cnt["nS"], "T": cnt["W"][b], "11": cnt["N1"][b], "21": cnt["N1"][b], "12": cnt["N2"][b], "22": cnt["N2"][b]}[name]


@pytest.mark.parametrize("names", [("S", "T"), ("11", "21"), ("12", "22")], ids=["homogeneous", "first-htrg", "second-htrg"])
def test_one_post_launch(dev, graph_case, names):
    head, cnt, pl, alone = graph_case
    B = len(WIDTHS)
    mods = pl.st["mods"]
    outs = []
    with torch.no_grad():
        for fill in (NAN, 0.0):
            for nm in names:
                lay = pl.layers[nm]
                for k in ("xd", "S", "y", "g"):
                    lay[k].fill_(fill)
                for b, (pb, _) in enumerate(alone):
                    n = _rows(cnt, nm, b)
                    fx = pb.layers[nm]
                    lay["xd"][b, :n] = fx["xd"][0]
                    raw = torch.empty(1, n, n, device=dev)      # the fixed plan's S holds the soft-max already: the raw scores again
                    ops.gat_score_fwd(fx["xd"], mods[nm].att_proj.weight, mods[nm].att_proj.bias, fx["a3_used"], raw, 1, n, fx["D"], fx["Do"], fx["n1"])
                    lay["S"][b].view(-1)[:n * n] = raw.view(-1)
                if lay["master"] and nm in ("12", "22"):      # the master node these layers start from: the first layer's output
                    src = pl.layers["11" if nm == "12" else "21"]["mout"]
                    for b, (pb, _) in enumerate(alone):
                        src[b] = pb.layers["11" if nm == "12" else "21"]["mout"][0]
            graph._post(pl.st, names, B, True, pl)
            torch.cuda.synchronize()
            outs.append({nm: {k: pl.layers[nm][k].clone() for k in ("y", "g", "S") + (("mout", "am") if pl.layers[nm]["master"] else ())} for nm in names})
    worst = 0.0
    for nm in names:
        for b, (pb, _) in enumerate(alone):
            n = _rows(cnt, nm, b)
            fx = pb.layers[nm]
            got = outs[0][nm]
            pairs = [(got["y"][b, :n], fx["y"][0]), (got["g"][b, :n], fx["g"][0]), (got["S"][b].view(-1)[:n * n], fx["S"][0].view(-1))]
            if pl.layers[nm]["master"]:
                pairs += [(got["mout"][b], fx["mout"][0]), (got["am"][b, :n], fx["am"][0])]
            for g_, f_ in pairs:
                assert torch.isfinite(g_).all(), (nm, b)
                worst = max(worst, maxrel(g_, f_))
            for k in ("y", "g"):      # NaN against zeros in everything beyond the utterance's rows: the same bits in the rows
                assert torch.equal(outs[0][nm][k][b, :n], outs[1][nm][k][b, :n]), (nm, b, k)
            assert torch.equal(outs[0][nm]["S"][b].view(-1)[:n * n], outs[1][nm]["S"][b].view(-1)[:n * n])
    print("post launch %s: worst %.2e" % (names, worst))
    assert worst <= TOL


@pytest.mark.parametrize("tag", ["1", "2"])
def test_one_pre_launch(dev, graph_case, tag):
    head, cnt, pl, alone = graph_case
    B = len(WIDTHS)
    srcs, outs_l = (("T", "S"), ("11", "21")) if tag == "1" else (("11", "21"), ("12", "22"))
    units = ("T", "S") if tag == "1" else ("T1", "S1", "T2", "S2")
    res = []
    with torch.no_grad():
        for fill in (NAN, 0.0):
            for nm in srcs:
                pl.layers[nm]["y"].fill_(fill)
                for b, (pb, _) in enumerate(alone):
                    pl.layers[nm]["y"][b, :_rows(cnt, nm, b)] = pb.layers[nm]["y"][0]
            for nm in outs_l:
                pl.layers[nm]["xd"].fill_(fill)
            for u in units:
                pl.units[u]["pooled"].fill_(fill)
            graph._pre_fwd(pl, pl.st, tag, 1 if tag == "1" else 0, B)
            torch.cuda.synchronize()
            res.append(({nm: pl.layers[nm]["xd"].clone() for nm in outs_l}, {u: (pl.units[u]["pooled"].clone(), pl.units[u]["idx"].clone()) for u in units}))
    worst = 0.0
    for b, (pb, _) in enumerate(alone):
        for nm in outs_l:
            n = _rows(cnt, nm, b)
            got = res[0][0][nm][b, :n]
            assert torch.isfinite(got).all() and torch.equal(got, res[1][0][nm][b, :n]), (nm, b)
            worst = max(worst, maxrel(got, pb.layers[nm]["xd"][0]))
        for u in units:
            k = pb.units[u]["pooled"].shape[1]
            worst = max(worst, maxrel(res[0][1][u][0][b, :k], pb.units[u]["pooled"][0]))
            assert torch.equal(res[0][1][u][1][b, :k], pb.units[u]["idx"][0]), (u, b)      # the same nodes kept, in the same order
    print("pre launch %s: worst %.2e" % (tag, worst))
    assert worst <= TOL


def test_one_final_launch(dev, graph_case):
    head, cnt, pl, alone = graph_case
    B = len(WIDTHS)
    fin = pl.st["fin"]
    res = []
    with torch.no_grad():
        for fill in (NAN, 0.0):
            for nm in ("12", "22"):
                pl.layers[nm]["y"].fill_(fill)
            for u in ("T1", "T2"):
                pl.units[u]["pooled"].fill_(fill)
            for b, (pb, _) in enumerate(alone):
                for nm in ("11", "21", "12", "22"):
                    pl.layers[nm]["mout"][b] = pb.layers[nm]["mout"][0]
                for nm in ("12", "22"):
                    pl.layers[nm]["y"][b, :cnt["N2"][b]] = pb.layers[nm]["y"][0]
                for u in ("T1", "S1", "T2", "S2"):
                    k = pb.units[u]["pooled"].shape[1]
                    pl.units[u]["pooled"][b, :k] = pb.units[u]["pooled"][0]
            logits, hidden = torch.empty(B, 2, device=dev), torch.empty(B, 160, device=dev)
            fin.logits, fin.hidden = logits.data_ptr(), hidden.data_ptr()
            ops._call("scl_graph_final_fwd_var", ctypes.byref(fin), pl.cnt[2].data_ptr(), B, S(), keep=fin)
            torch.cuda.synchronize()
            res.append((logits, hidden))
    assert torch.isfinite(res[0][0]).all() and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for b, (pb, (lo, hid)) in enumerate(alone):
        assert maxrel(res[0][0][b], lo[0]) <= TOL and maxrel(res[0][1][b], hid[0]) <= TOL, b


# ---- 4. the back-end -------------------------------------------------------------------------------------------------------------------
def _pool_gaps(ref, feats):
    """Every GraphPool of the fp64 oracle on one utterance: the gap between the last kept and the first dropped score."""
    gaps, hooks = [], []

    def hook(mod, inp, out):
        s = torch.sigmoid(mod.proj(inp[0]))[0, :, 0].sort(descending=True)[0]
        keep = max(int(s.shape[0] * mod.k), 1)
        if keep < s.shape[0]:
            gaps.append((s[keep - 1] - s[keep]).item())
    for m in ref.modules():
        if isinstance(m, OH.GraphPool):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        out = ref(feats)
    for h in hooks:
        h.remove()
    return out, min(gaps)


@pytest.fixture(scope="module")
def backend_case(dev):
    head, sd = _filled_head(dev)
    ref = OH.AasistHead().double().eval()
    ref.load_state_dict({k: torch.from_numpy(v).to(ref.state_dict()[k].dtype) for k, v in sd.items()})
    gen = torch.Generator().manual_seed(SEED)
    T = 320      # a batch padded well beyond its longest utterance, as main.py pads to multiples of 16,000 samples
    feats = torch.zeros(len(FRAMES), T, 128)
    for b, n in enumerate(FRAMES):
        feats[b, :n] = torch.randn(n, 128, generator=gen)
    refs, gap = [], 1.0
    for b, n in enumerate(FRAMES):
        out, g = _pool_gaps(ref, feats[b:b + 1, :n].double())
        refs.append(out)
        gap = min(gap, g)
    return head, feats, refs, gap


def test_forward_frames_against_the_fixed_length_forward_and_the_fp64_oracle(dev, backend_case):
    head, feats, refs, gap = backend_case
    print("smallest gap between a kept and a dropped GraphPool score (fp64): %.2e" % gap)
    assert gap >= 2e-6      # precondition: top-k is discontinuous, a closer gap cannot be compared across precisions (change SEED, not the batch)
    resstack._POOL_W.plans.clear(); graph._POOL_C.plans.clear()
    fd = feats.to(dev)
    with torch.no_grad():
        lo, hid = (t.clone() for t in head.forward_frames(fd, FRAMES))
        torch.cuda.synchronize()
        assert lo.shape == (len(FRAMES), 2) and hid.shape == (len(FRAMES), 160) and torch.isfinite(lo).all() and torch.isfinite(hid).all()
        worst_f, worst_o = 0.0, 0.0
        for b, n in enumerate(FRAMES):
            fl, fh = head(fd[b:b + 1, :n].contiguous())      # the product's fixed-length fused forward on the utterance alone
            ef = max(maxrel(lo[b], fl[0]), maxrel(hid[b], fh[0]))
            eo = max(maxrel(lo[b], refs[b][0][0]), maxrel(hid[b], refs[b][1][0]))
            print("%3d frames: against the fixed-length forward %.2e, against the fp64 oracle %.2e" % (n, ef, eo))
            worst_f, worst_o = max(worst_f, ef), max(worst_o, eo)
        assert worst_f <= TOL and worst_o <= TOL, (worst_f, worst_o)
        # NaN in the padded rows of feats: not a bit changes
        fn = fd.clone()
        for b, n in enumerate(FRAMES):
            fn[b, n:] = NAN
        lo2, hid2 = head.forward_frames(fn, FRAMES)
        assert torch.equal(lo2, lo) and torch.equal(hid2, hid)
        # a second batch of another shape and other counts, then the first again (a replay of its recorded plan)
        second = [200, 199, 198, 197]
        g2 = torch.Generator().manual_seed(SEED + 1)
        f2 = torch.zeros(4, 200, 128)
        for b, n in enumerate(second):
            f2[b, :n] = torch.randn(n, 128, generator=g2)
        f2 = f2.to(dev)
        lo_s, hid_s = (t.clone() for t in head.forward_frames(f2, second))
        for b, n in enumerate(second):
            fl, fh = head(f2[b:b + 1, :n].contiguous())
            assert maxrel(lo_s[b], fl[0]) <= TOL and maxrel(hid_s[b], fh[0]) <= TOL, n
        lo3, hid3 = head.forward_frames(fd, FRAMES)
        assert torch.equal(lo3, lo) and torch.equal(hid3, hid)
        # the same shape with other counts: the recorded plan follows the count tables
        perm = FRAMES[::-1]
        fp = torch.stack([fd[len(FRAMES) - 1 - b] for b in range(len(FRAMES))])
        lo4, hid4 = head.forward_frames(fp.contiguous(), perm)
        assert torch.equal(lo4, lo.flip(0)) and torch.equal(hid4, hid.flip(0))
        torch.cuda.synchronize()
    # the plan bound: map widths are rounded up to a multiple of 8 — the batches' widest utterances have 80 and 66 columns: 80 and 72
    keys = sorted(p.key for p in resstack._POOL_W.plans)
    assert [k[:3] for k in keys] == [(4, 42, 72), (10, 42, 80)] and all(k[2] % resstack.WIDTH_STEP == 0 for k in keys)
    assert sorted(p.key[:3] for p in graph._POOL_C.plans) == [(4, 42, 72), (10, 42, 80)]


def test_plans_stay_bounded_over_many_batch_shapes(dev, backend_case):
    """The choice: the map width is the widest utterance rounded up to a multiple of 8 (<= 10 geometries per batch size), and the pools of
    these forward-only plans keep at most PlanPool.MAX_POOL plans, the oldest going first."""
    head = backend_case[0]
    resstack._POOL_W.plans.clear(); graph._POOL_C.plans.clear()
    assert [resstack.plan_width(w) for w in (1, 8, 9, 66, 73, 80)] == [8, 8, 16, 72, 80, 80]
    with torch.no_grad():
        for B in (1, 2, 3):
            for n in range(3, 243, 12):      # 20 lengths -> at most 10 widths per batch size
                head.forward_frames(torch.zeros(B, n, 128, device=dev), [n] * B)
        torch.cuda.synchronize()
    cap = resstack.PlanPool.MAX_POOL
    assert len(resstack._POOL_W.plans) <= cap and len(graph._POOL_C.plans) <= cap
    assert len({p.key for p in resstack._POOL_W.plans}) == len(resstack._POOL_W.plans)
    assert all(p.key[2] % 8 == 0 and getattr(p, "dx", None) is None for p in resstack._POOL_W.plans)      # forward buffers only
    assert all(p.layers["T"]["dP"] is None and p.de is None for p in graph._POOL_C.plans)


# ---- 5. the plugin ---------------------------------------------------------------------------------------------------------------------
class CpuRef(torch.nn.Module):
    """oracle encoder + LL + the oracle head on the CPU, one utterance at its own length."""

    def __init__(self, ssl_sd, cfg, head_sd):
        super().__init__()
        self.cfg = cfg
        self.ssl = {k: v.clone() for k, v in ssl_sd.items()}
        self.LL = torch.nn.Linear(cfg.embed, 128)
        head = OH.AasistHead(AH.UPSTREAM_AASIST)
        for n, c in head.named_children():
            self.add_module(n, c)
        for n in ("pos_S", "master1", "master2"):
            self.register_parameter(n, getattr(head, n))
        self.load_state_dict(head_sd)
        self.eval()

    def alone(self, x):
        with torch.no_grad():
            rf = self.LL(W.forward(self.ssl, self.cfg, x))
            ro, rh = OH.AasistHead.forward(self, rf)
        return ro, rf, rh


COUNTS = [1040, 1700, 20000, 64000, 77839]      # 3, 5, 62, 199 and 242 frames in a [5, 80000] batch: every row has padding
_CACHE = {}


def _setup(dev, small, seed):
    if small not in _CACHE:
        ocfg = W.W2VConfig(**SMALL) if small else W.W2VConfig.tiny()
        ssl = W.init_state(ocfg, seed=seed)
        m = Model(ARGS, dev, w2v_cfg=W2VConfig(**SMALL) if small else W2VConfig.tiny())
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("ssl_model.")}
        head_sd = {k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=seed + 1).items()}
        sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
        sd.update(head_sd)
        m.load_state_dict(sd)
        m.eval()
        gen = torch.Generator().manual_seed(seed)
        x = torch.zeros(len(COUNTS), 80000)
        for b, n in enumerate(COUNTS):
            x[b, :n] = 0.1 * torch.randn(n, generator=gen)
        _CACHE[small] = (m, x, CpuRef(ssl, ocfg, head_sd))
    return _CACHE[small]


def _alone_on_gpu(m, x, dev):
    with torch.no_grad():
        return [tuple(t.clone() for t in m(x[b:b + 1, :n].to(dev))) for b, n in enumerate(COUNTS)]


def test_fp32_scoring_of_a_padded_batch(dev, monkeypatch):
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    m, x, _ = _setup(dev, False, 91)
    assert m.head_takes_frames and m.min_samples() == 1040 and m.max_samples() == 77839 and m.head_max_frames() == 242
    cfg = m.cfg
    with torch.no_grad():
        out, feats, hid = m(x.to(dev), lengths=COUNTS)
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, dev)
    assert hid.shape == (5, 160) and feats.shape == (5, cfg.conv_lens(80000)[-1], 128)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        assert (feats[b, Tb:] == 0).all() and (feats[b, Tb - 1] != 0).any()
        go, gf, gh = alone[b]
        g = (maxrel(out[b], go[0]), maxrel(hid[b], gh[0]), maxrel(feats[b, :Tb], gf[0]))
        print("fp32 n=%d (%d frames): max-rel against the GPU alone logits %.2e hidden %.2e feats %.2e" % ((n, Tb) + g))
        assert max(g) < 1e-3, (n, g)


def test_fp32_scoring_on_packed_rows_agrees_with_the_padded_layout(dev, monkeypatch):
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    m, x, _ = _setup(dev, True, 93)
    cfg = m.cfg
    res = {}
    for pack in (False, True):
        monkeypatch.setattr(ENC, "SCORE_PACK", pack)
        with torch.no_grad():
            res[pack] = tuple(t.clone() for t in m(x.to(dev), lengths=COUNTS))
            torch.cuda.synchronize()
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    alone = _alone_on_gpu(m, x, dev)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        for pack in (False, True):
            out, feats, hid = res[pack]
            assert (feats[b, Tb:] == 0).all()
            go, gf, gh = alone[b]
            g = (maxrel(out[b], go[0]), maxrel(hid[b], gh[0]), maxrel(feats[b, :Tb], gf[0]))
            print("fp32 %s n=%d (%d frames): max-rel against the GPU alone logits %.2e hidden %.2e feats %.2e" % ("packed" if pack else "padded", n, Tb, g[0], g[1], g[2]))
            assert max(g) < 1e-3, (pack, n, g)
        p = tuple(maxrel(res[True][i][b], res[False][i][b]) for i in range(3))
        assert max(p) < 1e-3, (n, p)


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_bf16_scoring_of_a_padded_batch(dev, monkeypatch, pack):
    """SCL_SCORE_FP32=0: the bf16 encoder kernels with the padding mask (and SCL_VARLEN_PACK).  Per tensor the bar is the larger of the bf16
    floor (rel-L2 1e-2 feats, 3e-2 hidden and logits) and twice the error the fixed-length bf16 path makes on the same utterance alone,
    both against the CPU chain on that utterance alone — tests/test_resnet_varlen_gpu.py's bar for its plugin."""
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    monkeypatch.setattr(MF, "SCORE_FP32", False); monkeypatch.setattr(ML, "SCORE_FP32", False)
    monkeypatch.setattr(ENC, "VARLEN_PACK", pack)
    m, x, ref = _setup(dev, True, 93)
    cfg = m.cfg
    with torch.no_grad():
        out, feats, hid = (t.clone() for t in m(x.to(dev), lengths=COUNTS))
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, dev)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, rh = ref.alone(x[b:b + 1, :n].clone())
        assert (feats[b, Tb:] == 0).all()
        go, gf, gh = alone[b]
        for name, got, fixed, want, floor in (("feats", feats[b, :Tb], gf[0], rf[0], 1e-2), ("hidden", hid[b], gh[0], rh[0], 3e-2),
                                              ("logits", out[b], go[0], ro[0], 3e-2)):
            err, base = rl2(got, want), rl2(fixed, want)
            print("bf16 %s n=%d (%d frames) %s: rel-L2 %.2e, the fixed-length path alone %.2e, bar %.2e"
                  % ("packed" if pack else "padded", n, Tb, name, err, base, max(floor, 2 * base)))
            assert err < max(floor, 2 * base), (name, n, err, base)


def test_plugin_refusals(dev, monkeypatch):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    m, x, _ = _setup(dev, False, 91)
    xs = x[2:4].to(dev)
    ok = [20000, 64000]
    monkeypatch.delenv("SCL_AASIST_LENGTHS", raising=False)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="wav2vec2_linear_nll"):
        m(xs, lengths=ok)      # the switch is off: the refusal as it was
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(xs, lengths=ok)      # autograd on
    m.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
            m(xs, lengths=ok)
    finally:
        m.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="1040"):
            m(xs, lengths=[20000, 1039])      # 2 frames
        with pytest.raises(ValueError, match="77839"):
            m(xs, lengths=[20000, 77840])     # 243 frames
        monkeypatch.setattr(AH, "FUSED_STACK", False)
        with pytest.raises(NotImplementedError, match="SCL_AASIST_FUSED=0"):
            m(xs, lengths=ok)
        monkeypatch.setattr(AH, "FUSED_STACK", True)
        assert torch.isfinite(m(xs, lengths=ok)[0]).all()


# ---- 6. main.py --eval --padding_type none ----------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_eval_padding_type_none_with_the_aasist_plugin(dev, tmp_path, monkeypatch, capsys):
    import yaml
    import main as M
    from scl_amd import pack
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    sizes = [700, 3000, 20000, 33333, 64600, 90000]      # one below min_samples() = 1040, one beyond max_samples() = 77839
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(root / u), 0.1 * rs.randn(n))
    (root / "protocol.txt").write_text("".join("%s eval bonafide\n" % u for u in ids))
    cfg = {"model": {"name": "wav2vec2_aasist", "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"}, "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ref_model = M.MODEL_REGISTRY["wav2vec2_aasist"](cfg["model"], dev, seed=5)
    shapes = {k: tuple(v.shape) for k, v in ref_model.state_dict().items() if not k.startswith("ssl_model.")}
    ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=6).items()}, strict=False)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    lo, hi = ref_model.min_samples(), ref_model.max_samples()
    assert (lo, hi) == (1040, 77839)
    want_lp, want_emb = [], []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            x = torch.cat([x, torch.zeros(lo - n)]) if n < lo else x[:hi]      # the data path pads to the minimum and cuts at the maximum
            o, _, e = ref_model(x[None].to(dev))      # each file alone at its own length
            want_lp.append(o[0].cpu().numpy()); want_emb.append(e[0].cpu().numpy())
    common = ["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "3", "--eval", "--model_path", str(ck), "--padding_type", "none"]
    relerr = lambda got, ref: np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()
    out = tmp_path / "scores.txt"
    monkeypatch.delenv("SCL_AASIST_LENGTHS", raising=False)
    with pytest.raises(SystemExit) as e:      # the switch unset: main.py exits as before
        M.main(common + ["--eval_output", str(out)])
    assert "wav2vec2_linear_nll only" in str(e.value) and not out.exists()
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    capsys.readouterr()
    assert M.main(common + ["--eval_output", str(out)]) == 0
    assert "6 utterances, 1 cut to 77839 samples" in capsys.readouterr().out
    lines = out.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for l, ref in zip(lines, want_lp):
        assert relerr([float(v) for v in l.split()[1:]], ref) < 1e-3, (l, ref)
    pred = tmp_path / "pred.txt"
    assert M.main(common + ["--predict", "--eval_output", str(pred)]) == 0
    lines = pred.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for l, ref in zip(lines, want_lp):
        assert abs(float(l.split()[1]) - ref[1]) <= 1e-3 * np.abs(ref).max() and int(l.split()[2]) == int(ref.argmax())
    embd = tmp_path / "emb"
    assert M.main(common + ["--emb", "--eval_output", str(embd)]) == 0
    lines = (embd / "scores.txt").read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for u, ref in zip(ids, want_emb):
        got = np.load(str(embd / (u.split(".")[0] + ".npy")))
        assert got.shape[-1] == 160 and relerr(got, ref) < 1e-3, u
