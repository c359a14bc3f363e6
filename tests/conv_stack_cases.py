"""Conv feature extractor, layers 1..6, one stage at a time (CPU only; shared by tests/test_conv_stack_cases_cpu.py and
tests/test_conv_stack_gpu.py).

A stage is  z = gelu(layer_norm(conv1d(z_prev, W, stride s) + b))  on channels-last [B, T, C] activations.  The encoder keeps every
stage's inputs and outputs (Encoder.bufs: z, y, cmean, crstd, dz, dyp), so a stage of a real step is checked against a reference fed
that stage's own stored inputs: no error accumulates across stages and the bars sit at one bf16 rounding.

  stage_reference   plain torch float64 autograd: the anchor.
  stage_emulation   the same stage in fp32 with exactly the roundings the encoder is written to make (bf16 operands, fp32 accumulation,
                    y fp32, z bf16, dy rounded to bf16 before both gradient GEMMs, dz_prev bf16): what the reference alone, with the
                    permitted roundings, gives under the metrics below.  EMU holds its worst values over the cases of the CPU test; the
                    bars of the bf16-limited tensors are twice those (BARS).
  wd_reference / phase_dgrad   the backward-data operand of ops.conv_weight_pack built by index, and the phase-split transposed convolution
                    over it in fp64 (dz[s u + p] = sum_q dy[u - q] W[p + s q]).
"""
import math

import torch
import torch.nn.functional as F

B = 3
CLIPS = (4000, 6075)
WIDTHS = ("tiny", "c512")
CASES = [(w, L) for w in WIDTHS for L in CLIPS]
EPS = 1e-5
U23, u24 = 2.0 ** -23, 2.0 ** -24


def config_kwargs(width):
    """Keyword arguments of W2VConfig (the encoder's and the oracle's alike).  tiny: the config of every golden.  c512: the production
    conv width (tile selection and split-K of the weight gradient depend on N = 512, K = k * 512) over a shallow transformer."""
    if width == "tiny":
        return dict(conv_dim=32, embed=64, layers=2, heads=4, ffn=128, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)
    return dict(conv_dim=512, embed=128, layers=1, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)


def leftover(Tin, k, s):
    """Input frames behind the last tap of the last output frame: no gradient reaches them."""
    return (Tin - k) % s


def unreached_rows(Tin, k, s):
    Tout = (Tin - k) // s + 1
    return range(s * (Tout - 1) + k, Tin)


# ---- the stage ---------------------------------------------------------------------------------------------------------------------
def _cols(x, k, s, Tout):
    """[B, Tin, C] -> [B, Tout, k * C], column j * C + c = x[:, s t + j, c]  (the GEMM rows of the convolution)."""
    return torch.cat([x[:, j: j + s * (Tout - 1) + 1: s] for j in range(k)], dim=2)


def _wk(w):
    """Conv1d weight [Co, Ci, k] -> GEMM operand [Co, k * Ci], k index = j * Ci + ci."""
    Co, Ci, k = w.shape
    return w.permute(0, 2, 1).reshape(Co, k * Ci)


def stage_reference(z_prev, w, b, gamma, beta, dz, s):
    """float64 autograd.  z_prev: bf16 (or any) [B, Tin, C] as stored; w: the master weight rounded to bf16 [Co, Ci, k]; b, gamma, beta:
    fp32 [C]; dz: bf16 [B, Tout, C] as stored, or None (forward only).  Returns a dict of fp64 tensors: y, y_bound (the per-element bound
    of tests/gemm_ref.py for an fp32 C from bf16 operands + bias), mean, rstd, z and, with dz, dy, dz_prev, dw [Co, Ci, k], db, dgamma,
    dbeta."""
    x = z_prev.detach().double().clone().requires_grad_(dz is not None)
    wd_, bd, gd, btd = (t.detach().double().clone().requires_grad_(dz is not None) for t in (w, b, gamma, beta))
    k = w.shape[2]
    Tout = (x.shape[1] - k) // s + 1
    cols = _cols(x, k, s, Tout)
    acc = cols @ _wk(wd_).t()
    y = acc + bd
    if dz is not None:
        y.retain_grad()
    mean = y.mean(-1)
    var = y.var(-1, unbiased=False)
    rstd = (var + EPS).rsqrt()
    z = F.gelu(F.layer_norm(y, (y.shape[-1],), gd, btd, EPS))
    with torch.no_grad():
        Kd = cols.shape[-1]
        e = Kd * U23 * (cols.abs() @ _wk(wd_).abs().t())
        e = e + u24 * (y.abs() + e)
    out = dict(y=y.detach(), y_bound=e, mean=mean.detach(), rstd=rstd.detach(), z=z.detach())
    if dz is not None:
        z.backward(dz.detach().double())
        out.update(dy=y.grad, dz_prev=x.grad, dw=wd_.grad, db=bd.grad, dgamma=gd.grad, dbeta=btd.grad)
    return out


def _bf(t):
    return t.to(torch.bfloat16)


def stage_emulation(z_prev, w, b, gamma, beta, dz, s, mutate=None):
    """The stage with the roundings the encoder makes and nothing else: fp32 products of bf16 operands with fp32 accumulation, y fp32,
    z stored bf16, dy rounded to bf16 before both gradient GEMMs, dz_prev stored bf16; the LayerNorm / GELU arithmetic and the vector
    gradients in fp32.  Same arguments and keys as stage_reference (z, dy, dz_prev come back in bf16).
    mutate (the sensitivity test): "dgrad_last_frame" / "wgrad_last_frame" leave the last output frame of every utterance out of that
    gradient, "wd_swap" swaps the two tap blocks of phase 0 of the backward-data operand, "stale_leftover" leaves the left-over input
    rows of dz_prev at a previous step's values."""
    x = _bf(z_prev).float()
    wf = _bf(w).float()
    b, gamma, beta = b.float(), gamma.float(), beta.float()
    Co, Ci, k = w.shape
    Bn, Tin, C = x.shape
    Tout = (Tin - k) // s + 1
    cols = _cols(x, k, s, Tout)
    y = (cols @ _wk(wf).t() + b).requires_grad_(True)
    mean = y.mean(-1)
    rstd = (y.var(-1, unbiased=False) + EPS).rsqrt()
    g_, bt_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = F.gelu(F.layer_norm(y, (C,), g_, bt_, EPS))
    z.backward(_bf(dz).float())
    dy = y.grad
    dyb = _bf(dy)
    dyf = dyb.float()
    dyw = dyf.clone()
    if mutate == "wgrad_last_frame":
        dyw[:, -1] = 0
    dw = (dyw.reshape(-1, Co).t() @ cols.reshape(-1, k * Ci)).view(Co, k, Ci).permute(0, 2, 1).contiguous()
    dyd = dyf.clone()
    if mutate == "dgrad_last_frame":
        dyd[:, -1] = 0
    blocks = wd_reference(_bf(w), s)
    if mutate == "wd_swap":
        assert len(range(0, k, s)) == 2, "phase 0 needs two taps"
        blocks = [blocks[1], blocks[0]] + blocks[2:]
    dzp = phase_dgrad(dyd, [t.float() for t in blocks], k, s, Tin)
    if mutate == "stale_leftover":
        rows = list(unreached_rows(Tin, k, s))
        assert rows, "no left-over input frame at this shape"
        stale = torch.randn(Bn, len(rows), C, generator=torch.Generator().manual_seed(99)) * dzp.std()
        dzp[:, rows] = stale
    return dict(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), z=_bf(z.detach()), dy=dyb, dz_prev=_bf(dzp), dw=dw, db=dy.sum((0, 1)),
                dgamma=g_.grad, dbeta=bt_.grad)


# ---- backward-data operand ----------------------------------------------------------------------------------------------------------
def wd_order(k, s):
    """The tap of every block of wd: phases ascending, descending tap inside a phase."""
    return [j for p in range(min(s, k)) for j in reversed(range(p, k, s))]


def wd_reference(w, s):
    """w [Co, Ci, k] -> list of k blocks [Co, Ci] in wd's order (built by index; the values are w's own, no arithmetic)."""
    return [w[:, :, j].contiguous() for j in wd_order(w.shape[2], s)]


def phase_dgrad(dy, blocks, k, s, Tin):
    """dz_prev [B, Tin, Ci] from dy [B, Tout, Co] and wd's blocks, one product per output phase as the encoder launches them:
    dz[s u + p] = sum_q dy[u - q] W[p + s q], u = 0 .. (Tin - 1 - p) // s, dy = 0 outside its frames.  Every row of dz is written."""
    Bn, Tout, Co = dy.shape
    Ci = blocks[0].shape[1]
    dz = torch.full((Bn, Tin, Ci), float("nan"), dtype=dy.dtype)
    blk = 0
    for p in range(s):
        nq = len(range(p, k, s))
        Up = (Tin - 1 - p) // s
        if Up < 0:
            continue
        acc = torch.zeros(Bn, Up + 1, Ci, dtype=dy.dtype)
        for i in range(nq):      # block blk + i holds tap p + s * q with q = nq - 1 - i
            q = nq - 1 - i
            lo, hi = q, min(Up, Tout - 1 + q)      # u with 0 <= u - q <= Tout - 1
            if hi >= lo:
                acc[:, lo: hi + 1] += dy[:, lo - q: hi - q + 1] @ blocks[blk + i]
        dz[:, p::s][:, : Up + 1] = acc
        blk += nq
    return dz


# ---- dyp geometry -------------------------------------------------------------------------------------------------------------------
def dyp_view(dyp, Bn, C, Rp):
    return dyp[: Bn * Rp * C].view(Bn, Rp, C)


def dyp_frames(dyp, Bn, C, Q, Rp, Tout):
    """The frame rows of the zero-padded LayerNorm-backward output: [B, Tout, C]."""
    return dyp_view(dyp, Bn, C, Rp)[:, Q: Q + Tout]


def dyp_padding(dyp, Bn, C, Q, Rp, Tout):
    """The complement: the Q rows in front of and the Rp - Q - Tout rows behind every utterance's frames, [B, Rp - Tout, C]."""
    v = dyp_view(dyp, Bn, C, Rp)
    return torch.cat([v[:, :Q], v[:, Q + Tout:]], dim=1)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------
def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def rel_max(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def boundary_rows(got, ref, n=4):
    """Worst per-row rel-L2 over the first n and the last n frames of every utterance ([B, T, C]).  A row whose reference is exactly 0
    (a left-over input frame's gradient) counts 0 when it is exactly 0 and inf otherwise."""
    got, ref = got.double().cpu(), ref.double().cpu()
    T = ref.shape[1]
    rows = sorted(set(range(min(n, T))) | set(range(max(0, T - n), T)))
    err = (got[:, rows] - ref[:, rows]).norm(dim=-1)
    nrm = ref[:, rows].norm(dim=-1)
    r = torch.where(nrm > 0, err / nrm.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(err), torch.full_like(err, math.inf), r)
    return r.max().item()


def y_ratio(got, ref):
    """Worst |got - y| / bound over the elements of the fp32 conv output."""
    return ((got.double().cpu() - ref["y"]).abs() / ref["y_bound"].clamp_min(1e-300)).max().item()


# ---- bars ---------------------------------------------------------------------------------------------------------------------------
# Worst value of stage_emulation against stage_reference per tensor kind over the cases of tests/test_conv_stack_cases_cpu.py (which
# asserts them as upper bounds).  l2: rel-L2; max: max |err| / max |ref|; rows: boundary_rows.
EMU = {
    "z_l2": 1.72e-3, "z_max": 3.2e-3, "z_rows": 2.9e-3,          # measured 1.709e-3, 3.198e-3, 2.862e-3
    "dyp_l2": 1.68e-3, "dyp_max": 2.65e-3, "dyp_rows": 2.75e-3,   # measured 1.673e-3, 2.625e-3, 2.734e-3
    "dz_l2": 2.37e-3, "dz_max": 4.2e-3, "dz_rows": 3.4e-3,        # measured 2.363e-3, 4.185e-3, 3.374e-3
    "dw_l2": 1.68e-3, "dw_max": 2.35e-3,                          # measured 1.677e-3, 2.332e-3
}
# bf16-limited tensors: twice the emulation (a different fp32 summation order and split-K slab order on the GPU are second-order next to
# the bf16 roundings the emulation contains).  fp32-limited quantities: the bars tests/test_kernels_gpu.py::test_layernorm_fwd_bwd
# applies to the same kernels (max |err| / max |ref|: 2e-5 an fp32 output, so rstd too; 1e-5 the mean; 5e-5 dgamma / dbeta; 2e-4 the
# sum-mode-2 column sum = the conv bias gradient); y: the per-element bound tests/gemm_ref.py derives for an fp32 C from bf16 operands
# (K * 2^-23 * sum |a b|, then one f32 rounding for the bias), as a ratio.
#
# Worst values measured on the MI355X by tests/test_conv_stack_gpu.py (four cases, two steps, layers 1..6), next to bar = 2 x EMU:
#   z    l2 1.690e-3 (3.44e-3)   max 3.548e-3 (6.4e-3)   rows 2.784e-3 (5.8e-3)
#   dyp  l2 1.755e-3 (3.36e-3)   max 3.387e-3 (5.3e-3)   rows 2.841e-3 (5.5e-3)
#   dz   l2 2.473e-3 (4.74e-3)   max 4.680e-3 (8.4e-3)   rows 3.795e-3 (6.8e-3)
#   dw   l2 2.048e-3 (3.36e-3)   max 2.399e-3 (4.7e-3)
#   y_ratio 1.52e-2 (1)   mean 4.5e-7 (1e-5)   rstd 1.3e-7 (2e-5)   dgamma 3.8e-7 (5e-5)   dbeta 2.5e-7 (5e-5)   db 4.0e-7 (2e-4)
# i.e. the kernels sit at the emulation (ratio 0.98 - 1.28 of EMU), nowhere near twice it.
BARS = {k: 2 * v for k, v in EMU.items()}
BARS.update({"y_ratio": 1.0, "mean": 1e-5, "rstd": 2e-5, "dgamma": 5e-5, "dbeta": 5e-5, "db": 2e-4})


def stage_metrics(got, ref, vectors=True):
    """{kind: value} of one stage: got / ref are dicts with the keys of stage_reference (got may lack y)."""
    m = {}
    for kind, key in (("z", "z"), ("dyp", "dy"), ("dz", "dz_prev")):
        m[kind + "_l2"], m[kind + "_max"] = rel_l2(got[key], ref[key]), rel_max(got[key], ref[key])
        m[kind + "_rows"] = boundary_rows(got[key], ref[key])
    m["dw_l2"], m["dw_max"] = rel_l2(got["dw"], ref["dw"]), rel_max(got["dw"], ref["dw"])
    if vectors:
        m["y_ratio"] = y_ratio(got["y"], ref)
        for kind in ("mean", "rstd", "dgamma", "dbeta", "db"):
            m[kind] = rel_max(got[kind], ref[kind])
    return m


def gaussian_stage(C, k, s, Tin, seed, Bn=B):
    """Seeded Gaussian inputs of one stage (weights at the oracle's scales)."""
    g = torch.Generator().manual_seed(seed)
    Tout = (Tin - k) // s + 1
    z_prev = _bf(torch.randn(Bn, Tin, C, generator=g))
    w = _bf(torch.randn(C, C, k, generator=g) * math.sqrt(2.0 / (C * k))).float()
    b = 0.02 * torch.randn(C, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g)
    beta = 0.05 * torch.randn(C, generator=g)
    dz = _bf(torch.randn(Bn, Tout, C, generator=g))
    return z_prev, w, b, gamma, beta, dz
