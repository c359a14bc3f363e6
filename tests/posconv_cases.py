"""Feature LayerNorm, post_extract_proj and the weight-normed grouped positional convolution, one stage at a time (CPU only; shared by
tests/test_posconv_cases_cpu.py and tests/test_posconv_stage_gpu.py).  Activations are channels-last [B, T, E]; `frames` is None or the
valid frame count of every utterance (rows at and beyond frames[b] are padding).

  Stage P   h = x0 * mask(frames);  w = g * v / ||v|| over dims (0, 1);  pre = conv1d(h, w, b, padding = K // 2, groups = G)[..., :-1];
            xin0 = h + gelu(pre).  Backward from dxin0: dc = dxin0 * gelu'(pre), dx0 = (dxin0 + conv^T(dc)) * mask, dv, dg, db.
            (oracle/wav2vec2.py forward(): the "positional conv" block, plus fairseq's features[padding_mask] = 0.)
  Stage F   h0 = layer_norm(z_last);  x0 = h0 W^T + b.  Backward from dx0: db, dW, d_h, then dz_last, dgamma, dbeta.

  stage_reference_p / _f   plain torch float64 autograd on the stage's STORED inputs (x0 or z[-1], the master weights, the stored upstream
            gradient): the anchor.
  stage_emulation_p / _f   the same stage with exactly the roundings the encoder is written to make and nothing else: xpad = bf16(x0),
            w rounded to bf16 after the fp32 normalisation, fp32 accumulation, pc_pre stored bf16 (of acc + bias, before the GELU), the
            GELU and the residual add in fp32 (gelu by the erf polynomial of csrc/common.h), dc = bf16(dxin0 * gelu'(bf16 pre)), the
            flipped / transposed bf16 weights for the data gradient, dwf from the two bf16 images; h0, d_h and dz in bf16, dx0 rounded to
            bf16 before the projection's two gradient GEMMs, its bias gradient from the fp32 dx0.  EMU holds the emulation's worst
            values over the cases of the CPU test; the bars of the bf16-limited tensors are twice those (BARS).

The convolution BRANCH is compared, not the residual sum (the sum dilutes a branch error by the size of x0): pc_pre, xin0 - x0, dc,
dx0 - dxin0.  Rows metrics run over the first and last four VALID frames of every utterance."""
import math

import torch
import torch.nn.functional as F

from tests.conv_stack_cases import U23, boundary_rows, rel_l2, rel_max, u24

EPS = 1e-5
BASE = dict(conv_dim=32, embed=128, layers=1, heads=2, ffn=256, final_dim=16, latent_vars=8, latent_groups=2)
CONFIGS = {"k128": dict(pos_k=128, pos_groups=2), "k16": dict(pos_k=16, pos_groups=2), "cg32": dict(pos_k=16, pos_groups=4)}
B_FIXED = 3
# fixed-layout clips as (frames, samples): the shortest clip of that many frames, and the 4 s production clip for 199
FIXED_CLIPS = {"k128": ((18, 5840), (199, 64000), (208, 66640), (209, 66960), (225, 72080)), "k16": ((18, 5840),), "cg32": ((18, 5840),)}
VARLEN_LENGTHS = {"k128": (64000, 21200, 5840, 400),      # 199, 66, 18 and 1 frames
                  "cg32": (12000, 4000, 7777, 400)}       # tests/test_varlen_train_gpu.py's LENGTHS: 37, 12, 24 and 1 frames
VARLEN_SECOND = {"k128": (5840, 64000, 400, 21200), "cg32": (4000, 12000, 400, 9000)}      # the second step: other rows, same slab


def samples_for(T):
    """The shortest clip of T frames."""
    return 320 * (T - 1) + 400


# (config, layout, sample counts): layout "fixed" (every row L samples), "padded" or "packed"
CASES = [(name, "fixed", (L,) * B_FIXED) for name in ("k128", "k16", "cg32") for _, L in FIXED_CLIPS[name]]
CASES += [(name, layout, VARLEN_LENGTHS[name]) for name in ("k128", "cg32") for layout in ("padded", "packed")]


def case_id(case):
    name, layout, lengths = case
    return "%s-%s-%d" % (name, layout, max(lengths))


def config_kwargs(name):
    return dict(BASE, **CONFIGS[name])


def _bf(t):
    return t.to(torch.bfloat16)


def mask_of(frames, Bn, T, dtype):
    """[B, T, 1]: 1 on rows below frames[b], 0 at and beyond it; None without frames."""
    if frames is None:
        return None
    return (torch.arange(T)[None, :] < torch.tensor([int(n) for n in frames])[:, None]).to(dtype).view(Bn, T, 1)


def valid(frames, Bn, T):
    return [T] * Bn if frames is None else [int(n) for n in frames]


def weight_norm(v, g):
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


# ---- packed weight layouts (index-built, no arithmetic) --------------------------------------------------------------------------------
def wf_layout(w, G):
    """Conv1d weight [E, Cg, K] -> the forward operand [g][co][j][ci] as [G, Cg, K * Cg]."""
    E, Cg, K = w.shape
    return w.view(G, Cg, Cg, K).permute(0, 1, 3, 2).reshape(G, Cg, K * Cg)


def wd_layout(w, G, flip=True):
    """The data-gradient operand [g][ci][j'][co], j' = K - 1 - j (flipped taps, transposed channels)."""
    E, Cg, K = w.shape
    w4 = w.view(G, Cg, Cg, K)
    return (w4.flip(-1) if flip else w4).permute(0, 2, 3, 1).reshape(G, Cg, K * Cg)


def dwf_to_conv(dwf, E, Cg, K):
    """[G, Cg, K * Cg] ([g][co][j][ci]) -> the gradient in Conv1d's layout [E, Cg, K]."""
    return dwf.reshape(E // Cg, Cg, K, Cg).permute(0, 1, 3, 2).reshape(E, Cg, K)


def slab_product(pad, wpk, T, G):
    """What both launches of the positional convolution compute: out[b][t][g, o] = sum_{j, c} pad[b][t + j][g, c] wpk[g][o][j * Cg + c]
    over a zero-padded image pad [B, T + K, E] and a packed operand [G, Cg, K * Cg] (accumulation in pad's dtype)."""
    Bn, Tp, E = pad.shape
    Cg = E // G
    K = wpk.shape[2] // Cg
    conv_w = wpk.reshape(G, Cg, K, Cg).permute(0, 1, 3, 2).reshape(E, Cg, K)
    return F.conv1d(pad.transpose(1, 2), conv_w, None, groups=G).transpose(1, 2)[:, :T]


def pad_image(x, K, before):
    """[B, T, E] -> [B, T + K, E] with `before` zero rows in front (ops.pad_rows)."""
    Bn, T, E = x.shape
    out = torch.zeros(Bn, T + K, E, dtype=x.dtype)
    out[:, before: before + T] = x
    return out


def wgrad_product(dypad, row0, xpad, T, G):
    """ops.posconv_wgrad / the transposed GEMM: dw[g][o][j * Cg + c] = sum_{b, t} dypad[b][row0 + t][g, o] xpad[b][t + j][g, c]."""
    Bn, Tp, E = xpad.shape
    K, Cg = Tp - T, E // G
    dy = dypad[:, row0: row0 + T].reshape(Bn, T, G, Cg)
    x4 = xpad.view(Bn, Tp, G, Cg)
    return torch.stack([torch.einsum("btgo,btgc->goc", dy, x4[:, j: j + T]) for j in range(K)], dim=2).reshape(G, Cg, K * Cg)


# ---- GELU as csrc/common.h evaluates it (erf by Abramowitz-Stegun 7.1.26, fp32) -----------------------------------------------------------
def _gelu_parts(x):
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    e = torch.exp(-(z * z))
    p = t * 1.061405429 - 1.453152027
    p = t * p + 1.421413741
    p = t * p - 0.284496736
    p = t * p + 0.254829592
    half_tail = (0.5 * (t * p)) * e
    return torch.where(x >= 0, 1.0 - half_tail, half_tail), e


def gelu_poly(x):
    return x * _gelu_parts(x)[0]


def gelu_grad_poly(x):
    cdf, e = _gelu_parts(x)
    return x * 0.39894228040143268 * e + cdf


# ---- Stage P -----------------------------------------------------------------------------------------------------------------------------
def stage_reference_p(x0, v, g, b, dxin0, G, frames=None):
    """float64 autograd.  x0 [B, T, E] as stored (fp32), v [E, Cg, K], g [1, 1, K], b [E] the master weights, dxin0 [B, T, E] as stored or
    None (forward only).  Returns fp64: h, w, pre, branch (= xin0 - h), xin0 and, with dxin0, dc, dx0, dbranch (= dx0 - dxin0), dw (Conv1d
    layout), dv, dg, db."""
    bwd = dxin0 is not None
    x = x0.detach().double().clone().requires_grad_(bwd)
    vd, gd, bd = (t.detach().double().clone().requires_grad_(bwd) for t in (v, g, b))
    Bn, T, E = x.shape
    K = v.shape[2]
    m = mask_of(frames, Bn, T, torch.float64)
    h = x if m is None else x * m
    w = weight_norm(vd, gd)
    pre = F.conv1d(h.transpose(1, 2), w, bd, padding=K // 2, groups=G)[..., :-1].transpose(1, 2)
    if bwd:
        w.retain_grad()
        pre.retain_grad()
    xin0 = h + F.gelu(pre)
    out = dict(h=h.detach(), w=w.detach(), pre=pre.detach(), branch=(xin0 - h).detach(), xin0=xin0.detach())
    if bwd:
        dx = dxin0.detach().double()
        xin0.backward(dx)
        out.update(dc=pre.grad, dx0=x.grad, dbranch=x.grad - dx, dw=w.grad, dv=vd.grad, dg=gd.grad, db=bd.grad)
    return out


MUTATIONS_P = ("drop_last_tap", "trim_first", "pb_off", "no_flip", "tail_leak", "tail_grad", "wgrad_last_frame")


def stage_emulation_p(x0, v, g, b, dxin0, G, frames=None, mutate=None):
    """Stage P as Encoder.forward / backward compose it (the "positional conv" blocks of scl_amd/encoder.py), in fp32 with the encoder's
    roundings: zero_tail_rows(x0); xpad = bf16(x0) behind K // 2 zero rows; pos_wf / pos_wd = the index-built layouts of bf16(w), w
    normalised in fp32; pc_pre = bf16(acc + bias); xin0 = gelu(acc + bias) + x0 in fp32; dcpad = bf16(dxin0 * gelu'(pc_pre)) behind
    K // 2 - 1 zero rows; db its column sum; dwf from dcpad x xpad; dx0 = dcpad * pos_wd + dxin0, its padded rows zeroed.  Same keys as
    stage_reference_p plus xpad, dcpad, wf, wd, dwf (pre and dc come back in bf16).
    mutate (the sensitivity test): "drop_last_tap" leaves tap K - 1 out of all three products; "trim_first" trims the first output frame
    instead of the last (K // 2 - 1 zero rows in front of x0); "pb_off" writes dcpad behind K // 2 rows while the products read it from
    K // 2 - 1; "no_flip" runs the data gradient with the forward tap order; "tail_leak" does not zero the padded rows of x0; "tail_grad"
    does not zero those of dx0; "wgrad_last_frame" leaves the last valid frame of every utterance out of the weight gradient."""
    assert mutate is None or mutate in MUTATIONS_P
    Bn, T, E = x0.shape
    Cg, K = v.shape[1], v.shape[2]
    pb = K // 2 - 1
    m = mask_of(frames, Bn, T, torch.float32)
    h = x0.float() if (m is None or mutate == "tail_leak") else x0.float() * m
    v32, g32, b32 = v.float(), g.float(), b.float()
    w = _bf(weight_norm(v32, g32))
    wq = w.clone()
    if mutate == "drop_last_tap":
        wq[:, :, K - 1] = 0
    wf, wd = wf_layout(wq, G), wd_layout(wq, G, flip=mutate != "no_flip")
    xpad = pad_image(_bf(h), K, K // 2 - 1 if mutate == "trim_first" else K // 2)
    acc = slab_product(xpad.float(), wf.float(), T, G) + b32
    pre = _bf(acc)
    xin0 = gelu_poly(acc) + h
    out = dict(h=h, w=w, wf=wf_layout(w, G), wd=wd_layout(w, G), xpad=xpad, pre=pre, xin0=xin0, branch=xin0.double() - h.double())
    if dxin0 is None:
        return out
    dx = dxin0.float()
    dc = _bf(dx * gelu_grad_poly(pre.float()))
    dcpad = pad_image(dc, K, K // 2 if mutate == "pb_off" else pb)
    db = dcpad.float().sum((0, 1))
    dyw = dcpad.float().clone()
    if mutate == "wgrad_last_frame":
        for bi, n in enumerate(valid(frames, Bn, T)):
            dyw[bi, pb + n - 1] = 0
    dwf = wgrad_product(dyw, pb, xpad.float(), T, G)
    if mutate == "drop_last_tap":
        dwf.view(G, Cg, K, Cg)[:, :, K - 1] = 0
    dx0 = slab_product(dcpad.float(), wd.float(), T, G) + dx
    if m is not None and mutate != "tail_grad":
        dx0 = dx0 * m
    vr, gr = v32.clone().requires_grad_(True), g32.clone().requires_grad_(True)
    dw = dwf_to_conv(dwf, E, Cg, K)
    weight_norm(vr, gr).backward(dw)
    out.update(dc=dc, dcpad=dcpad, dx0=dx0, dbranch=dx0.double() - dx.double(), dwf=dwf, dw=dw, dv=vr.grad, dg=gr.grad, db=db)
    return out


def weight_norm_backward(dwf, v, g, G):
    """fp64 (dv, dg) of w = g v / ||v|| from a given gradient image dwf [G, Cg, K * Cg]: what ops.posconv_weight_bwd computes."""
    E, Cg, K = v.shape
    vr, gr = v.detach().double().clone().requires_grad_(True), g.detach().double().clone().requires_grad_(True)
    weight_norm(vr, gr).backward(dwf_to_conv(dwf.detach().double().cpu(), E, Cg, K))
    return vr.grad, gr.grad


# ---- Stage F -----------------------------------------------------------------------------------------------------------------------------
def stage_reference_f(z, gamma, beta, W, b, dx0, h0_stored=None, dh_stored=None):
    """float64.  z [B, T, C] as stored (bf16), gamma / beta [C], W [E, C], b [E] the master weights, dx0 [B, T, E] as stored (fp32) or None.
    Every sub-stage is fed its own stored input where one is given: the projection h0_stored (else the reference's h0), the LayerNorm
    backward dh_stored (else the reference's d_h).  Returns h0, mean, rstd, x0 and x0_bound (the fp32 GEMM output from the operands the
    launch reads — h0 as stored, bf16(W) — with the per-element bound of tests/gemm_ref.py), proj (the reference's h0 through the master
    weight: the oracle's projection) and, with dx0, db, dW, d_h, dz, dgamma, dbeta."""
    zd = z.detach().double()
    C = zd.shape[-1]
    mean = zd.mean(-1)
    rstd = (zd.var(-1, unbiased=False) + EPS).rsqrt()
    h0 = F.layer_norm(zd, (C,), gamma.double(), beta.double(), EPS)
    hin = (h0 if h0_stored is None else h0_stored.detach().double())
    Wb = _bf(W.float()).double()
    x0 = hin @ Wb.t() + b.double()
    e = C * U23 * (hin.abs() @ Wb.abs().t())
    e = e + u24 * (x0.abs() + e)
    Wd = W.detach().double()
    out = dict(h0=h0, mean=mean, rstd=rstd, x0=x0, x0_bound=e, proj=h0 @ Wd.t() + b.double())
    if dx0 is None:
        return out
    d = dx0.detach().double()
    out.update(db=d.sum((0, 1)), dW=d.reshape(-1, d.shape[-1]).t() @ hin.reshape(-1, C), d_h=d @ Wd)
    dh = out["d_h"] if dh_stored is None else dh_stored.detach().double()
    zr = zd.clone().requires_grad_(True)
    gr, br = gamma.detach().double().clone().requires_grad_(True), beta.detach().double().clone().requires_grad_(True)
    F.layer_norm(zr, (C,), gr, br, EPS).backward(dh)
    out.update(dz=zr.grad, dgamma=gr.grad, dbeta=br.grad)
    return out


def stage_emulation_f(z, gamma, beta, W, b, dx0):
    """Stage F with the encoder's roundings: LayerNorm in fp32 with h0 stored bf16; x0 = h0 bf16(W)^T + b accumulated and stored in fp32;
    the bias gradient from the fp32 dx0; dx0 rounded to bf16 before the weight-gradient and the data-gradient GEMM (fp32 accumulation);
    d_h stored bf16; the LayerNorm backward in fp32 from it, dz stored bf16."""
    zf = _bf(z).float()
    C = zf.shape[-1]
    zr = zf.clone().requires_grad_(True)
    gr, br = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    mean = zf.mean(-1)
    rstd = (zf.var(-1, unbiased=False) + EPS).rsqrt()
    h32 = F.layer_norm(zr, (C,), gr, br, EPS)
    h0 = _bf(h32.detach())
    Wb = _bf(W.float()).float()
    x0 = h0.float() @ Wb.t() + b.float()
    out = dict(h0=h0, mean=mean, rstd=rstd, x0=x0)
    if dx0 is None:
        return out
    d = dx0.float()
    db = d.sum((0, 1))
    dxb = _bf(d).float()
    dW = dxb.reshape(-1, dxb.shape[-1]).t() @ h0.float().reshape(-1, C)
    d_h = _bf(dxb @ Wb)
    h32.backward(d_h.float())
    out.update(db=db, dW=dW, d_h=d_h, dz=_bf(zr.grad), dgamma=gr.grad, dbeta=br.grad)
    return out


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------
def valid_boundary_rows(got, ref, frames=None, n=4):
    """boundary_rows over the first n and the last n VALID frames of every utterance."""
    Bn, T = ref.shape[0], ref.shape[1]
    return max(boundary_rows(got[bi: bi + 1, :nv], ref[bi: bi + 1, :nv], n) for bi, nv in enumerate(valid(frames, Bn, T)))


P_FRAME_KINDS = (("pre", "pre"), ("br", "branch"), ("dc", "dc"), ("dxb", "dbranch"))      # (kind, key): [B, T, E] tensors of stage P
F_FRAME_KINDS = (("h0", "h0"), ("dh", "d_h"), ("dzl", "dz"))


def _frame_metrics(kinds, got, ref, frames, only=None):
    m = {}
    for kind, key in kinds:
        if key in got and key in ref and (only is None or kind in only):
            m[kind + "_l2"], m[kind + "_max"] = rel_l2(got[key], ref[key]), rel_max(got[key], ref[key])
            m[kind + "_rows"] = valid_boundary_rows(got[key], ref[key], frames)
    return m


def stage_metrics_p(got, ref, frames=None):
    """{kind: value}: the four branch tensors (rel-L2, max, boundary rows) and, where got holds them, dwf (got's packed layout against the
    reference's Conv1d-layout dw), dv, dg and the bias gradient against the fp64 stage."""
    m = _frame_metrics(P_FRAME_KINDS, got, ref, frames)
    if "dwf" in got:
        E, Cg, K = ref["dw"].shape
        dw = dwf_to_conv(got["dwf"].double().cpu(), E, Cg, K)
        m["dwf_l2"], m["dwf_max"] = rel_l2(dw, ref["dw"]), rel_max(dw, ref["dw"])
    for kind, key in (("dv", "dv"), ("dg", "dg"), ("dbp", "db")):
        if key in got:
            m[kind + "_l2"], m[kind + "_max"] = rel_l2(got[key].reshape(-1), ref[key].reshape(-1)), rel_max(got[key].reshape(-1), ref[key].reshape(-1))
    return m


def x0_ratio(got, ref, frames=None):
    """Worst |got - x0| / bound over the valid rows of the fp32 projection output."""
    r = (got.double().cpu() - ref["x0"]).abs() / ref["x0_bound"].clamp_min(1e-300)
    Bn, T = r.shape[0], r.shape[1]
    return max(r[bi, :nv].max().item() for bi, nv in enumerate(valid(frames, Bn, T)))


def stage_metrics_f(got, ref, frames=None):
    m = _frame_metrics(F_FRAME_KINDS, got, ref, frames)
    m["x0_ratio"] = x0_ratio(got["x0"], ref, frames)
    m["mean"], m["rstd"] = rel_max(got["mean"], ref["mean"]), rel_max(got["rstd"], ref["rstd"])
    if "dW" in got:
        m["pw_l2"], m["pw_max"] = rel_l2(got["dW"], ref["dW"]), rel_max(got["dW"], ref["dW"])
        for kind in ("dgamma", "dbeta", "db"):
            m[kind] = rel_max(got[kind], ref[kind])
    return m


# ---- bars --------------------------------------------------------------------------------------------------------------------------------
# Worst value of the emulations against the fp64 stages per tensor kind over the cases of tests/test_posconv_cases_cpu.py (which asserts
# them as upper bounds, and that each constant is within 15 % of the measured worst).  l2: rel-L2; max: max |err| / max |ref|; rows:
# valid_boundary_rows.  pre: pc_pre; br: xin0 - x0; dc; dxb: dx0 - dxin0; dwf, dv, dg, dbp: the gradients of the packed weight, weight_v,
# weight_g and the convolution's bias; h0, dh, dzl, pw: stage F's h0, d_h, dz[-1] and the gradient of post_extract_proj.weight.
EMU = {
    "pre_l2": 2.95e-3, "pre_max": 4.05e-3, "pre_rows": 3.55e-3,      # measured 2.902e-3, 4.007e-3, 3.488e-3
    "br_l2": 2.4e-3, "br_max": 2.3e-3, "br_rows": 3.15e-3,           # measured 2.373e-3, 2.285e-3, 3.097e-3
    "dc_l2": 1.78e-3, "dc_max": 3.45e-3, "dc_rows": 2.05e-3,         # measured 1.758e-3, 3.433e-3, 2.020e-3
    "dxb_l2": 2.45e-3, "dxb_max": 2.75e-3, "dxb_rows": 3.2e-3,       # measured 2.423e-3, 2.723e-3, 3.158e-3
    "dwf_l2": 2.45e-3, "dwf_max": 2.95e-3,                           # measured 2.422e-3, 2.905e-3
    "dv_l2": 2.45e-3, "dv_max": 3.25e-3,                             # measured 2.422e-3, 3.205e-3
    "dg_l2": 3.2e-3, "dg_max": 4.25e-3,                              # measured 3.177e-3, 4.226e-3
    "dbp_l2": 2.15e-3, "dbp_max": 2.25e-3,                           # measured 2.133e-3, 2.241e-3
    "h0_l2": 1.72e-3, "h0_max": 3.15e-3, "h0_rows": 2.8e-3,          # measured 1.705e-3, 3.100e-3, 2.749e-3
    "dh_l2": 2.92e-3, "dh_max": 4.2e-3, "dh_rows": 4.5e-3,           # measured 2.896e-3, 4.142e-3, 4.443e-3
    "dzl_l2": 1.7e-3, "dzl_max": 2.95e-3, "dzl_rows": 2.35e-3,       # measured 1.680e-3, 2.928e-3, 2.305e-3
    "pw_l2": 1.7e-3, "pw_max": 1.9e-3,                               # measured 1.688e-3, 1.895e-3
}
# bf16-limited tensors: twice the emulation (a different fp32 summation order on the GPU is second order next to the bf16 roundings the
# emulation contains; tests/conv_stack_cases.py reasons the same way).  fp32-limited quantities: the bars tests/test_kernels_gpu.py
# applies to the same kernels (max |err| / max |ref|): mean 1e-5, rstd 2e-5, dgamma / dbeta 5e-5, a column-sum bias gradient given the
# matrix it sums 2e-4 (db: post_extract_proj.bias from the stored dx0; dbp_sum: the convolution's from the stored dcpad), dv / dg given
# the stored dwf 1e-4 (dv_wn, dg_wn); wpack: a packed weight within one bf16 rounding of the index-built layout of w, as a ratio of
# 2^-8 |ref|; x0: the per-element bound of tests/gemm_ref.py for an fp32 C from bf16 operands, as a ratio.
# What the MI355X measures against these bars is recorded in the docstring of tests/test_posconv_stage_gpu.py: 0.44 - 0.70 of the bar on
# every bf16-limited kind (0.9 - 1.4 of EMU), at most 3 % of the bar on the fp32-limited ones.
BARS = {k: 2 * v for k, v in EMU.items()}
BARS.update({"x0_ratio": 1.0, "mean": 1e-5, "rstd": 2e-5, "dgamma": 5e-5, "dbeta": 5e-5, "db": 2e-4, "dbp_sum": 2e-4, "dv_wn": 1e-4,
             "dg_wn": 1e-4, "wpack": 1.0})


def wpack_ratio(got, ref):
    """Worst |got - ref| / (2^-8 |ref|) over a packed weight (0 where both are 0)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    err, lim = (got - ref).abs(), 2.0 ** -8 * ref.abs()
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return r.max().item()


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
def gaussian_stage(E, G, K, T, seed, Bn=B_FIXED, frames=None, C=32):
    """Seeded Gaussian inputs of both stages at the oracle's weight scales: dict with x0, v, g, b, dxin0 (stage P; dxin0 is 0 on padded
    rows, as the encoder's backward hands it over, x0 is not; x0 at the projection's output scale, 0.02 weights over 32 channels) and z (a
    GELU output, as z[-1] is), gamma, beta, W, pb, dx0 (stage F)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    Cg = E // G
    v = rn(E, Cg, K) * math.sqrt(4.0 / (K * E))
    g = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1.0 + 0.1 * rn(1, 1, K))
    dxin0 = rn(Bn, T, E)
    m = mask_of(frames, Bn, T, torch.float32)
    if m is not None:
        dxin0 = dxin0 * m
    return dict(x0=0.1 * rn(Bn, T, E), v=v, g=g, b=0.02 * rn(E), dxin0=dxin0, G=G, frames=frames,
                z=_bf(F.gelu(rn(Bn, T, C))), gamma=1.0 + 0.1 * rn(C), beta=0.05 * rn(C), W=0.02 * rn(E, C), pb=0.02 * rn(E), dx0=rn(Bn, T, E))


def p_args(s):
    return (s["x0"], s["v"], s["g"], s["b"], s["dxin0"], s["G"], s["frames"])


def f_args(s):
    return (s["z"], s["gamma"], s["beta"], s["W"], s["pb"], s["dx0"])
