"""The stretch between the conv stack and the transformer layers as the encoder composes it, stage by stage against fp64
(tests/posconv_cases.py): the feature LayerNorm, post_extract_proj, zero_tail_rows, the weight-normed grouped positional convolution with
GELU and residual, and the backward of all of these.

a. Stages of a real step.  Two training steps of the linear model (seeded Gaussian cotangents on its three outputs; the second step on
another input and, with lengths, on the lengths permuted, so it replays the recorded plans over other valid rows).  After each, stage P
and stage F are compared with the fp64 stages fed their own STORED inputs (x0, d(xin[0]), z[-1], d(x0), h0, d_h; the master weights):
the tap order of the weight pack, the flipped / transposed data-gradient operand, pad_before = K // 2 forward and K // 2 - 1 backward, the
dropped last output frame, gelu' on the stored bf16 pre-activation, the weight-norm backward, and the masks of a padded / packed batch.
Before each step h0, x0, the slabs of xpad and dcpad, pc_pre, xin[0] / xin_pad, dwf and d_h are NaN, so a row the step does not write
shows.  Cases (posconv_cases.CASES): pos_k = 128 over 64-channel groups at T = 18, 199, 208 (csrc/posconv.hip), 209 (forward and data
gradient on the grouped GEMM, weight gradient still posconv.hip) and 225 (everything on the GEMM and the split-K queue); pos_k = 16 on
posconv.hip; 32-channel groups on the GEMM; padded and packed batches of (199, 66, 18, 1) and (37, 12, 24, 1) frames.

d(xin[0]) and d(x0) are read through d["dxin0"] / d["dx0"], the names Encoder.backward leaves for the two f32 buffers it ended in (two of
the rotating dx_rot pairs; dxin_pad and dx0_pad[0] when packed).  Behind the positional-conv stage the backward writes d_h, dz, dyp, dwk,
the conv-stack gradients and reads the bf16 half of d(x0)'s pair: nothing writes those two f32 buffers again, so after the step they
still hold what the stage read and wrote.

b. Row-tile and tap edges of the kernels alone: ops.pad_rows -> ops.posconv_mfma (forward, data gradient) and ops.posconv_wgrad on
Gaussian stages at the 16-row tile edges of PC_TILES = 13, a single frame and the shortest tap rings, against the same fp64 stage and bars.

Bars: tests/posconv_cases.py::BARS.  bf16-limited tensors: twice what the fp64 stage with the encoder's permitted roundings gives on the
CPU (EMU; tests/test_posconv_cases_cpu.py asserts it).  Nothing is excluded from any comparison.

Worst values measured on the MI355X over the eleven cases of (a) and both steps, as "measured / emulated / bar":
    pc_pre       rel-L2 2.929e-3 / 2.95e-3 / 5.90e-3   max 4.282e-3 / 4.05e-3 / 8.10e-3   boundary rows 3.426e-3 / 3.55e-3 / 7.10e-3
    xin0 - x0    rel-L2 2.417e-3 / 2.40e-3 / 4.80e-3   max 2.643e-3 / 2.30e-3 / 4.60e-3   boundary rows 3.103e-3 / 3.15e-3 / 6.30e-3
    dc           rel-L2 1.818e-3 / 1.78e-3 / 3.56e-3   max 4.138e-3 / 3.45e-3 / 6.90e-3   boundary rows 2.188e-3 / 2.05e-3 / 4.10e-3
    dx0 - dxin0  rel-L2 2.478e-3 / 2.45e-3 / 4.90e-3   max 2.850e-3 / 2.75e-3 / 5.50e-3   boundary rows 3.122e-3 / 3.20e-3 / 6.40e-3
    dwf          rel-L2 2.711e-3 / 2.45e-3 / 4.90e-3   max 3.622e-3 / 2.95e-3 / 5.90e-3
    d weight_v   rel-L2 2.712e-3 / 2.45e-3 / 4.90e-3   max 3.573e-3 / 3.25e-3 / 6.50e-3
    d weight_g   rel-L2 3.526e-3 / 3.20e-3 / 6.40e-3   max 3.774e-3 / 4.25e-3 / 8.50e-3
    d conv bias  rel-L2 2.207e-3 / 2.15e-3 / 4.30e-3   max 2.378e-3 / 2.25e-3 / 4.50e-3
    h0           rel-L2 1.676e-3 / 1.72e-3 / 3.44e-3   max 3.453e-3 / 3.15e-3 / 6.30e-3   boundary rows 2.871e-3 / 2.80e-3 / 5.60e-3
    d_h          rel-L2 2.933e-3 / 2.92e-3 / 5.84e-3   max 4.202e-3 / 4.20e-3 / 8.40e-3   boundary rows 4.302e-3 / 4.50e-3 / 9.00e-3
    dz[-1]       rel-L2 1.720e-3 / 1.70e-3 / 3.40e-3   max 3.449e-3 / 2.95e-3 / 5.90e-3   boundary rows 2.406e-3 / 2.35e-3 / 4.70e-3
    d proj W     rel-L2 1.945e-3 / 1.70e-3 / 3.40e-3   max 2.643e-3 / 1.90e-3 / 3.80e-3
    x0 2.8e-2 of its per-element bound; pos_wf / pos_wd 0.996 of one bf16 rounding (the rounding itself); mean 5.5e-8 (bar 1e-5), rstd
    1.1e-7 (2e-5), dgamma 3.2e-7 (5e-5), dbeta 7.5e-8 (5e-5), projection bias gradient 2.1e-7 (2e-4), conv bias gradient given dcpad
    5.1e-8 (2e-4), d weight_v / d weight_g given dwf 1.8e-7 / 3.1e-7 (1e-4).
The kernels of (b) alone, worst over the 18 shapes: pc_pre 2.873e-3 / 4.577e-3 / 3.635e-3, xin0 - x0 2.361e-3 / 2.747e-3 / 3.172e-3,
dc 1.888e-3 / 3.774e-3 / 2.519e-3, dx0 - dxin0 2.787e-3 / 3.624e-3 / 3.831e-3 (rel-L2 / max / boundary rows), dwf 2.500e-3 / 3.725e-3.
Every measured value is 0.44 - 0.70 of its bar, i.e. at the emulation, nowhere near twice it.
Every must-be-zero region was exactly 0 after both steps in every case: the padding rows of xpad and dcpad, the rows of x0, d(x0) and
d(xin[0]) at and beyond frames[b], rows [row0[B], Mq) of the packed xin[0]; xpad's frame rows were bf16(x0) and the packed xin[0] the
valid rows of xin_pad bit for bit.  All 30 tests passed on first contact with the kernels; the emulation was not changed after it.
(Three deliberate in-bounds mistakes — dcpad one row late, the first frame trimmed, zero_tail_rows left out — each failed its case.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.lib import ACT_GELU  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests import posconv_cases as PC  # noqa: E402
from tests.test_conv_stack_gpu import ARGS, PRE, Report, step  # noqa: E402

NAN = float("nan")


def build(dev, name, train):
    kw = PC.config_kwargs(name)
    ocfg = W.W2VConfig(**kw)
    ssl, head = W.init_state(ocfg, seed=41), OH.init_head(ocfg.embed, seed=42)
    m = Model(ARGS, dev, w2v_cfg=W2VConfig(**kw))      # every encoder dropout is 0 in W2VConfig's defaults
    sd = {PRE + k: v for k, v in ssl.items()}
    sd.update(head)
    _, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected
    m.train(train)      # a batch with lengths trains on model.train() (the head's dropout is patched to 0); a fixed one as test_conv_stack_gpu
    return m


def poison(d, Bn, T, cfg, packed):
    C, E, K = cfg.conv_dim, cfg.embed, cfg.pos_k
    M = Bn * T
    for buf, n in ((d["h0"], M * C), (d["x0"], M * E), (d["xpad"], Bn * (T + K) * E), (d["dcpad"], Bn * (T + K) * E), (d["pc_pre"], M * E),
                   (d["xin"][0], d["xin"][0].numel()), (d["dwf"], d["dwf"].numel()), (d["d_h"], M * C)):
        buf[:n].fill_(NAN)
    if packed:
        d["xin_pad"].fill_(NAN)


def exactly_zero(t):
    return bool((t == 0).all())


def check_stages(rep, m, d, Bn, frames, layout):
    """frames: the valid frame counts of this step (None: fixed layout); layout: the RowLayout of the step or None."""
    cfg, P, enc = m.cfg, m.P, m.encoder
    C, E, K, G, T = cfg.conv_dim, cfg.embed, cfg.pos_k, cfg.pos_groups, d["T"]
    Cg, M, pb = E // G, Bn * d["T"], K // 2 - 1
    packed = layout is not None and layout.packed
    vec = lambda name: P.f32(PRE + name).float().cpu()
    grad = lambda name: P.g(PRE + name).float().cpu()
    rows = lambda buf, width: buf[: M * width].view(Bn, T, width).cpu()
    nv = PC.valid(frames, Bn, T)
    tag = "T %d%s" % (T, "" if frames is None else " frames %s" % (tuple(nv),))

    x0, xin0 = rows(d["x0"], E), rows(d["xin_pad"] if packed else d["xin"][0], E)
    dxin0, dx0 = rows(d["dxin0"], E), rows(d["dx0"], E)
    for name, t in (("d(xin[0])", dxin0), ("d(x0)", dx0)):      # precondition: a real gradient reached the stage
        rep.require(bool(torch.isfinite(t).all()) and bool(t.any()), "%s is not finite and non-zero" % name)
    if packed:
        rep.require(d["dxin0"] is d["dxin_pad"] and d["dx0"] is d["dx0_pad"][0], "the packed layout's names for d(xin[0]) / d(x0)")
    else:
        f32s = [pair[0] for pair in d["dx_rot"]]
        rep.require(any(d["dxin0"] is t for t in f32s) and any(d["dx0"] is t for t in f32s) and d["dxin0"] is not d["dx0"],
                    "d(xin[0]) / d(x0) are two of the rotating pairs")

    # ---- the two zero-padded images: exact
    xpad = d["xpad"][: Bn * (T + K) * E].view(Bn, T + K, E).cpu()
    dcpad = d["dcpad"][: Bn * (T + K) * E].view(Bn, T + K, E).cpu()
    rep.require(torch.equal(xpad[:, K // 2: K // 2 + T], x0.to(torch.bfloat16)), "%s: xpad's frame rows are not bf16(x0)" % tag)
    rep.require(exactly_zero(xpad[:, : K // 2]) and exactly_zero(xpad[:, K // 2 + T:]), "%s: a padding row of xpad is not 0" % tag)
    rep.require(exactly_zero(dcpad[:, :pb]) and exactly_zero(dcpad[:, pb + T:]), "%s: a padding row of dcpad is not 0" % tag)

    # ---- stage P
    v, g, b = vec("encoder.pos_conv.0.weight_v"), vec("encoder.pos_conv.0.weight_g"), vec("encoder.pos_conv.0.bias")
    ref = PC.stage_reference_p(x0, v, g, b, dxin0, G, frames)
    dwf = d["dwf"].view(G, Cg, K * Cg).cpu()
    got = dict(pre=rows(d["pc_pre"], E), branch=xin0.double() - x0.double(), dc=dcpad[:, pb: pb + T], dbranch=dx0.double() - dxin0.double(),
               dwf=dwf, dv=grad("encoder.pos_conv.0.weight_v"), dg=grad("encoder.pos_conv.0.weight_g"), db=grad("encoder.pos_conv.0.bias"))
    for kind, val in PC.stage_metrics_p(got, ref, frames).items():
        rep.check(kind, tag, val)
    rep.check("wpack", tag + " pos_wf", PC.wpack_ratio(enc.pos_wf, PC.wf_layout(ref["w"], G)))
    rep.check("wpack", tag + " pos_wd", PC.wpack_ratio(enc.pos_wd, PC.wd_layout(ref["w"], G)))
    dv, dg = PC.weight_norm_backward(dwf, v, g, G)      # the fp32-limited kernels against fp64 on the matrices they read
    rep.check("dv_wn", tag, PC.rel_max(got["dv"], dv))
    rep.check("dg_wn", tag, PC.rel_max(got["dg"], dg))
    rep.check("dbp_sum", tag, PC.rel_max(got["db"], dcpad.double().sum((0, 1))))

    # ---- stage F
    z = rows(d["z"][-1], C)
    h0, d_h = rows(d["h0"], C), rows(d["d_h"], C)
    ref = PC.stage_reference_f(z, vec("layer_norm.weight"), vec("layer_norm.bias"), vec("post_extract_proj.weight"), vec("post_extract_proj.bias"),
                               dx0, h0_stored=h0, dh_stored=d_h)
    got = dict(h0=h0, mean=d["fmean"].view(Bn, T).cpu(), rstd=d["frstd"].view(Bn, T).cpu(), x0=x0, d_h=d_h, dz=rows(d["dz"][-1], C),
               dW=grad("post_extract_proj.weight"), db=grad("post_extract_proj.bias"), dgamma=grad("layer_norm.weight"),
               dbeta=grad("layer_norm.bias"))
    for kind, val in PC.stage_metrics_f(got, ref, frames).items():
        rep.check(kind, tag, val)

    # ---- the masks of a batch with lengths: exact
    if frames is not None:
        for bi, n in enumerate(nv):
            rep.require(exactly_zero(x0[bi, n:]) and exactly_zero(dx0[bi, n:]), "%s: x0 / d(x0) of utterance %d is not 0 beyond its frames" % (tag, bi))
            rep.require(exactly_zero(dxin0[bi, n:]), "%s: d(xin[0]) of utterance %d is not 0 beyond its frames" % (tag, bi))
    if packed:
        Mq, Mv = layout.Mq, sum(nv)
        pk = d["xin"][0][: Mq * E].view(Mq, E).cpu()
        rep.require(torch.equal(pk[:Mv], torch.cat([xin0[bi, :n] for bi, n in enumerate(nv)])), "%s: xin[0] is not the valid rows of xin_pad" % tag)
        rep.require(Mq % 64 == 0 and Mq >= Mv and exactly_zero(pk[Mv:]), "%s: rows [row0[B], Mq) of xin[0] are not 0" % tag)


@pytest.mark.parametrize("case", PC.CASES, ids=[PC.case_id(c) for c in PC.CASES])
def test_posconv_and_projection_stages_against_fp64(dev, monkeypatch, case):
    name, layout_name, lengths = case
    varlen = layout_name != "fixed"
    monkeypatch.setattr(ML, "DROP_P", 0.0)
    monkeypatch.setattr(ENC, "VARLEN_PACK", layout_name == "packed")
    m = build(dev, name, train=varlen)
    cfg = m.cfg
    Bn, L = len(lengths), max(lengths)
    Cg = cfg.embed // cfg.pos_groups
    assert Cg == (32 if name == "cg32" else 64)

    def layout_of(lens):
        return ENC.row_layout(cfg, lens, Bn, L, min_samples=m.min_samples(), refuse_short=False, score_f32=False, device=dev)

    if varlen:
        _, lay = layout_of(lengths)
        assert lay.packed == (layout_name == "packed")
        d = m.encoder.bufs(Bn, L, lay, train=True)
    else:
        lay = None
        d = m.encoder.bufs(Bn, L, train=True)
    T = d["T"]
    assert T == cfg.conv_lens(L)[-1]
    gen = torch.Generator().manual_seed(7)
    cot = [torch.randn(Bn, 2, generator=gen).to(dev), torch.randn(Bn, T, 128, generator=gen).to(dev), torch.randn(Bn, 128, generator=gen).to(dev)]
    rep = Report("posconv %s" % PC.case_id(case), PC.BARS)
    for n in range(2):      # the second step replays the recorded plans on another input (and other lengths): stale state, stale tails
        rep.step = n + 1
        lens = (lengths, PC.VARLEN_SECOND[name])[n] if varlen else None
        x = (0.1 * torch.randn(Bn, L, generator=torch.Generator().manual_seed(1000 * n + L))).to(dev)
        poison(d, Bn, T, cfg, varlen and lay.packed)
        if varlen:
            frames, lay_n = layout_of(lens)
            out, feats, emb = m(x, lengths=list(lens))
            for p in m.parameters():
                p.grad = None
            ((out * cot[0]).sum() + (feats * cot[1]).sum() + (emb * cot[2]).sum()).backward()
            torch.cuda.synchronize()
            sets = list(m.encoder._vbufs_train.values())
            assert len(sets) == 1 and sets[0] is d and not m.encoder._bufs
            st, = m._vstates_train.values()
            assert len(st["plans"]) == 2      # one plan per direction: the second step replayed them
        else:
            frames, lay_n = None, None
            step(m, x, cot)
            assert m.encoder.bufs(Bn, L, train=True) is d
        check_stages(rep, m, d, Bn, frames, lay_n)
    rep.done()


# ---- b. the kernels alone at the row-tile and tap edges ----------------------------------------------------------------------------------
TK = [(1, 128), (16, 128), (17, 128), (192, 128), (193, 128), (208, 128), (1, 2), (17, 2), (65, 8)]


def nan_tail(t, dev, extra=65536):
    buf = torch.full((t.numel() + extra,), NAN, dtype=t.dtype, device=dev)
    buf[: t.numel()] = t.reshape(-1).to(dev)
    return buf


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("T,K", TK, ids=["T%d-K%d" % tk for tk in TK])
def test_posconv_kernels_at_tile_and_tap_edges_against_fp64(dev, T, K, G):
    Bn, Cg = 2, 64
    E, M, pb = G * Cg, Bn * T, K // 2 - 1
    assert ops.posconv_supported(T, K, G, Cg)
    s = PC.gaussian_stage(E, G, K, T, seed=300 + 7 * T + K + G, Bn=Bn)
    ref = PC.stage_reference_p(*PC.p_args(s))
    w = PC.weight_norm(s["v"], s["g"]).to(torch.bfloat16)      # fp32 normalisation, one rounding; the layouts by index
    wf, wd = nan_tail(PC.wf_layout(w, G).contiguous(), dev), nan_tail(PC.wd_layout(w, G).contiguous(), dev)
    n_img = Bn * (T + K) * E
    x0, dxin0, bias = nan_tail(s["x0"], dev), nan_tail(s["dxin0"], dev), s["b"].to(dev)
    new = lambda n, dtype: torch.full((n + 65536,), NAN, dtype=dtype, device=dev)
    xpad, dcpad, pre = new(n_img, torch.bfloat16), new(n_img, torch.bfloat16), new(M * E, torch.bfloat16)
    xin0, dx0 = new(M * E, torch.float32), new(M * E, torch.float32)
    ops.pad_rows(x0, xpad, Bn, T, E, T + K, K // 2)
    ops.posconv_mfma(xpad, wf, xin0, x0, Bn, T, K, G, Cg, bias=bias, c2=pre)
    ops.pad_rows(dxin0, dcpad, Bn, T, E, T + K, pb, pre=pre, ract=ACT_GELU)
    ops.posconv_mfma(dcpad, wd, dx0, dxin0, Bn, T, K, G, Cg)
    dwf = None
    if ops.posconv_wgrad_supported(T, K, G, Cg):
        dwf = new(G * Cg * K * Cg, torch.float32)
        ops.posconv_wgrad(dcpad, pb, xpad, dwf, Bn, T, K, G, Cg)
    assert (dwf is not None) == (K % 8 == 0)
    torch.cuda.synchronize()
    rep = Report("posconv kernels T=%d K=%d G=%d" % (T, K, G), PC.BARS)
    rep.step = 1
    for what, buf, n in (("xpad", xpad, n_img), ("dcpad", dcpad, n_img), ("pc_pre", pre, M * E), ("xin0", xin0, M * E), ("dx0", dx0, M * E)) + \
            ((("dwf", dwf, G * Cg * K * Cg),) if dwf is not None else ()):
        rep.require(bool(torch.isnan(buf[n:].float()).all()), "%s: written past its end" % what)
        rep.require(bool(torch.isfinite(buf[:n].float()).all()), "%s: not finite" % what)
    img = lambda buf: buf[:n_img].view(Bn, T + K, E).cpu()
    rows = lambda buf: buf[: M * E].view(Bn, T, E).cpu()
    rep.require(torch.equal(img(xpad)[:, K // 2: K // 2 + T], s["x0"].to(torch.bfloat16)), "xpad's frame rows are not bf16(x0)")
    rep.require(exactly_zero(img(xpad)[:, : K // 2]) and exactly_zero(img(xpad)[:, K // 2 + T:]), "a padding row of xpad is not 0")
    rep.require(exactly_zero(img(dcpad)[:, :pb]) and exactly_zero(img(dcpad)[:, pb + T:]), "a padding row of dcpad is not 0")
    got = dict(pre=rows(pre), branch=rows(xin0).double() - s["x0"].double(), dc=img(dcpad)[:, pb: pb + T],
               dbranch=rows(dx0).double() - s["dxin0"].double())
    if dwf is not None:
        got["dwf"] = dwf[: G * Cg * K * Cg].view(G, Cg, K * Cg).cpu()
    for kind, val in PC.stage_metrics_p(got, ref).items():
        rep.check(kind, "kernels", val)
    rep.done()


def test_posconv_kernels_still_refuse_what_they_cannot_run(dev):
    assert not ops.posconv_supported(209, 128, 2, 64) and not ops.posconv_supported(225, 128, 2, 64)
    assert ops.posconv_supported(208, 128, 2, 64) and ops.posconv_wgrad_supported(209, 128, 2, 64) and ops.posconv_wgrad_supported(224, 128, 2, 64)
    assert not ops.posconv_wgrad_supported(225, 128, 2, 64)
    assert not ops.posconv_supported(18, 15, 2, 64) and not ops.posconv_wgrad_supported(18, 15, 2, 64)      # odd K
    assert ops.posconv_supported(18, 6, 2, 64) and not ops.posconv_wgrad_supported(18, 6, 2, 64)             # K = 6: no 8-tap block
    assert not ops.posconv_supported(18, 16, 4, 32) and not ops.posconv_wgrad_supported(18, 16, 4, 32)       # 32-channel groups
