"""The materialised-score attention path (225-512 frames with 64-wide heads, every length with other head widths, and the fp32 scoring
path up to 512 frames): scl_softmax_fwd / scl_softmax_fwd_f32 / scl_softmax_bwd / scl_dropout_rows and the batched GEMMs around them,
against fp64 (tests/attention_cases.py).

  1. the soft-max rows on their own, element by element, at every 64-column chunk boundary up to T = Tp = 512;
  2. the bf16 training chain of encoder.py, forward and backward, against fp64 at 2 x the rounding model's own distance to fp64, and
     against the streaming / fused kernels on the same inputs;
  3. the same chain at training batch sizes (64 and 128 utterances x 16 heads x 512 frames) with twinned utterances;
  4. the fp32 scoring chain (pair form and exact kernel) at the shipped --eval shape;
  5. the model through this path at 225 / 257 / 511 / 512 frames against the fp32 CPU oracle.

Measured on an MI355X (profiles/attention_mat_tests.log; the table is in DESIGN.md's test section).  Part 2 and 3, rel-L2 to fp64, all
46 chain runs: ctx 2.28 - 3.05e-3, dq 2.86 - 3.20e-3, dk 2.79 - 3.07e-3, dv 2.27 - 2.97e-3 — the rounding model gives the same figures to
three digits (largest GPU / model ratio 1.002, bar 2), max-rel at most 5.3e-3 (bar 3e-2); second launches and all twins bit-equal.
Streaming and fused kernels against the chain: ctx 3.1 - 3.8e-3, dq / dk 3.5 - 3.6e-3, dv 1e-4 (p = 0) and 3.5 - 3.6e-3 (p = 0.1),
every utterance of the (64, 16, 512) dropout launch within 3.7e-3.  Part 4, max-rel: S 5.3 - 6.6e-6 (pair form) and 2.2 - 4.3e-7
(exact), P 6 - 11e-8, ctx 5.5 - 6.5e-6 (pair) and 5.4e-7 - 1.0e-6 (exact; a plain fp32 CPU attention: 4.0 - 4.8e-7).  Part 5: outputs
7e-5, feats 7.1 - 7.3e-3, emb 7e-4 - 1.0e-3 rel-L2 to the oracle; fp32 scoring 1.7e-7 / 3.8e-6 / 3.0e-5 max-rel."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from scl_amd.model_linear import DROP_P, Model  # noqa: E402
from scl_amd.ops import Op  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests import attention_cases as AC  # noqa: E402
from tests.attention_cases import cosine, keep_scale, keep_scale_range, maxrel, rl2  # noqa: E402

NAN = float("nan")
SEED = 0x2468ACE
U = 2.0 ** -23            # one f32 ulp (relative)
TINY = 2.0 ** -126        # smallest normal f32 / bf16: anything below may be flushed to zero
# The bars of other tests that this file re-uses, by name
CLOSE_BF16_MAXREL = 3e-2                      # test_model_gpu.py / test_long_clip_gpu.py::close_bf16
LONG_RL2_CTX, LONG_RL2_DQKV = 1.2e-2, 2.5e-2  # test_long_clip_gpu.py::test_long_attention_kernels_against_fp64 (rl2 of ctx; of dq / dk / dv)
F32_SOFTMAX_MAXREL = 1e-5                     # test_long_clip_gpu.py::test_long_f32_softmax_rows
F32_GEMM_BAR = {True: 2e-5, False: 2e-6}      # test_gemm_gpu.py::test_f32_operand_kernel_matches_fp64 (pair form / exact kernel); None = pair form


def close_bf16(got, ref):      # test_model_gpu.py's bar for outputs
    return rl2(got, ref) < 1e-2 and maxrel(got, ref) < 3e-2


def g(seed):
    return torch.Generator().manual_seed(seed)


def up(n, m):
    return (n + m - 1) // m * m


# =====================================================================================================================================
# 1. soft-max rows on their own
# =====================================================================================================================================
ROW_LENGTHS = [1, 63, 64, 65, 199, 201, 224, 225, 249, 256, 257, 320, 384, 448, 449, 505, 511, 512]
KINDS = ["normal3", "pm80", "const", "dominant"]


def score_rows(kind, R, T, seed):
    if kind == "normal3":
        return 3.0 * torch.randn(R, T, generator=g(seed))
    if kind == "pm80":            # rows scaled to +-80: every term but the largest few underflows
        s = torch.randn(R, T, generator=g(seed))
        return s * (80.0 / s.abs().amax(1, keepdim=True).clamp_min(1e-30))
    if kind == "const":
        return torch.full((R, T), 1.0) * torch.linspace(-50.0, 50.0, R)[:, None]
    s = torch.randn(R, T, generator=g(seed))            # one dominant entry, at a different column in every row (the last one included)
    for r in range(R):
        s[r, (T - 1 - r * 97) % T] += 30.0
    return s


def fwd_eps(S):
    """Relative f32 round-off of one soft-max output before its final rounding, per row, from the operation count of softmax_fwd_kernel:
    a = s - max is exact up to 2^-24 |a|, `__expf(a)` = exp2(a log2 e) carries the rounding of that product (another 2^-24 |a| in the
    result) plus one ulp of the hardware exp2: U (|a| + 1) with |a| <= the row's range; the row sum adds 8 terms per lane and 6 butterfly
    steps (14 roundings of 2^-24 = 7 U) to terms that carry the same exp error (their weighted mean <= U (range + 1)); the reciprocal
    and the final product are one ulp each (2 U).  Total U (2 range + 11)."""
    rng = (S.double().amax(1, keepdim=True) - S.double().amin(1, keepdim=True))
    return U * (2.0 * rng + 11.0)


def check_bf16_fwd(P, S, T, what):
    """Every element within one bf16 rounding (2^-8 |ref|) of fp64, widened by the f32 round-off in front of the rounding; pads exactly 0."""
    ref = torch.softmax(S.double(), -1)
    got = P[:, :T].double().cpu()
    bound = (2.0 ** -8 * (1.0 + fwd_eps(S)) + fwd_eps(S)) * ref + TINY
    bad = (got - ref).abs() > bound
    assert not bad.any() and torch.isfinite(got).all(), (what, int(bad.sum()), ((got - ref).abs() / bound).max().item())
    assert (P[:, T:] == 0).all(), (what, "pad columns")


def check_bwd(dS, Pb, dP, T, what):
    """softmax_bwd_kernel: dot = sum P dP (per lane 8 multiply-adds, 6 butterfly steps: <= 16 roundings of 2^-24 of sum |P dP|), then
    dP - dot and the product with P (one rounding each: U |ref| together, and U more for the bf16 rounding acting on the perturbed
    value), then the bf16 rounding.  The dv - dot cancellation is why
    the dot's error enters as an absolute term |P| 8 U sum |P dP| and not relative to the result."""
    P64, dP64 = Pb.double(), dP.double()
    ref = P64 * (dP64 - (P64 * dP64).sum(1, keepdim=True))
    floor = P64.abs() * 8.0 * U * (P64 * dP64).abs().sum(1, keepdim=True)
    bound = (2.0 ** -8 + 2.0 * U) * ref.abs() + (1.0 + 2.0 ** -8) * floor + TINY
    got = dS[:, :T].double().cpu()
    bad = (got - ref).abs() > bound
    assert not bad.any() and torch.isfinite(got).all(), (what, int(bad.sum()), ((got - ref).abs() / bound).max().item())
    assert (dS[:, T:] == 0).all(), (what, "pad columns")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", ROW_LENGTHS)
def test_softmax_rows_against_fp64(dev, T, kind):
    R, Tp = 7, up(T, 8)                      # R % 4 != 0: the last block of four waves is partly filled
    S = score_rows(kind, R, T, 1000 + T)
    Sd = torch.full((R, Tp), NAN); Sd[:, :T] = S
    Sd = Sd.to(dev)
    # bf16 forward
    P = torch.full((R, Tp), NAN, dtype=torch.bfloat16, device=dev)
    ops.softmax_fwd(Sd, P, R, T, Tp, Tp)
    torch.cuda.synchronize()
    check_bf16_fwd(P, S, T, "softmax_fwd")
    # f32 forward, at Tp = T rounded up to 8 and to 4
    for Tp4 in sorted({Tp, up(T, 4)}):
        S4 = torch.full((R, Tp4), NAN); S4[:, :T] = S
        P4 = torch.full((R, Tp4), NAN, device=dev)
        ops.softmax_fwd_f32(S4.to(dev), P4, R, T, Tp4, Tp4)
        torch.cuda.synchronize()
        e = maxrel(P4[:, :T], torch.softmax(S.double(), -1))
        assert e < F32_SOFTMAX_MAXREL, ("softmax_fwd_f32", Tp4, e)
        assert (P4[:, T:] == 0).all(), ("softmax_fwd_f32 pad columns", Tp4)
    # backward: P = the bf16 rounding of the fp64 soft-max, the reference formed in fp64 from those same bf16 values
    Pb = torch.zeros(R, Tp, dtype=torch.bfloat16); Pb[:, :T] = torch.softmax(S.double(), -1).float().to(torch.bfloat16)
    dP = torch.full((R, Tp), NAN); dP[:, :T] = torch.randn(R, T, generator=g(2000 + T))
    dS = torch.full((R, Tp), NAN, dtype=torch.bfloat16, device=dev)
    ops.softmax_bwd(Pb.to(dev), dP.to(dev), dS, R, T, Tp, Tp)
    torch.cuda.synchronize()
    check_bwd(dS, Pb[:, :T], dP[:, :T], T, "softmax_bwd")


def test_softmax_rows_with_a_score_pitch_beyond_Tp(dev):
    R, T, Tp, ld = 7, 257, 264, 288
    S = score_rows("normal3", R, T, 5)
    Sd = torch.full((R, ld), NAN); Sd[:, :T] = S
    P = torch.full((R, Tp), NAN, dtype=torch.bfloat16, device=dev)
    ops.softmax_fwd(Sd.to(dev), P, R, T, ld, Tp)
    Pf = torch.full((R, Tp), NAN, device=dev)
    ops.softmax_fwd_f32(Sd.to(dev), Pf, R, T, ld, Tp)
    torch.cuda.synchronize()
    check_bf16_fwd(P, S, T, "softmax_fwd ldS > Tp")
    assert maxrel(Pf[:, :T], torch.softmax(S.double(), -1)) < F32_SOFTMAX_MAXREL and (Pf[:, T:] == 0).all()
    Pb = torch.zeros(R, Tp, dtype=torch.bfloat16); Pb[:, :T] = torch.softmax(S.double(), -1).float().to(torch.bfloat16)
    dP = torch.full((R, ld), NAN); dP[:, :T] = torch.randn(R, T, generator=g(6))
    dS = torch.full((R, Tp), NAN, dtype=torch.bfloat16, device=dev)
    ops.softmax_bwd(Pb.to(dev), dP.to(dev), dS, R, T, ld, Tp)
    torch.cuda.synchronize()
    check_bwd(dS, Pb[:, :T], dP[:, :T], T, "softmax_bwd lddP > Tp")


def test_softmax_rows_at_the_evaluation_launch_size(dev):
    """One launch of R = 64 x 16 x 201 rows (the shipped evaluation's batch): every 997th row and the first and last eight against fp64,
    the pad columns of ALL rows (an unwritten row keeps its NaN there)."""
    T, Tp = 201, 208
    R = 64 * 16 * T
    S = 3.0 * torch.randn(R, Tp, generator=g(9))
    Sd = S.to(dev)
    rows = torch.unique(torch.cat([torch.arange(0, R, 997), torch.arange(8), torch.arange(R - 8, R)]))
    P = torch.full((R, Tp), NAN, dtype=torch.bfloat16, device=dev)
    ops.softmax_fwd(Sd, P, R, T, Tp, Tp)
    Pf = torch.full((R, Tp), NAN, device=dev)
    ops.softmax_fwd_f32(Sd, Pf, R, T, Tp, Tp)
    dP = torch.randn(R, Tp, generator=g(10)).to(dev)
    dS = torch.full((R, Tp), NAN, dtype=torch.bfloat16, device=dev)
    ops.softmax_bwd(P, dP, dS, R, T, Tp, Tp)
    torch.cuda.synchronize()
    assert (P[:, T:] == 0).all() and (Pf[:, T:] == 0).all() and (dS[:, T:] == 0).all()
    assert torch.isfinite(P.float()).all() and torch.isfinite(Pf).all() and torch.isfinite(dS.float()).all()
    rd = rows.to(dev)
    Ssub = S[rows, :T]
    check_bf16_fwd(P[rd].cpu(), Ssub, T, "softmax_fwd sampled rows")
    assert maxrel(Pf[rd][:, :T], torch.softmax(Ssub.double(), -1)) < F32_SOFTMAX_MAXREL
    check_bwd(dS[rd].cpu(), P[rd][:, :T].cpu(), dP[rd][:, :T].cpu(), T, "softmax_bwd sampled rows")


@pytest.mark.parametrize("T,Tp,which", [(513, 520, "all"), (512, 520, "all"), (201, 204, "bf16"), (201, 202, "f32"), (201, 200, "all")])
def test_softmax_refusals(dev, T, Tp, which):
    """The SCL_REQUIRE checks of csrc/attention.hip's entry points, made on the host before any launch: T = 513, Tp = 520, Tp % 8 != 0
    for the bf16 kernels, Tp % 4 != 0 for the f32 kernel, Tp < T."""
    R, ld = 4, 520
    S = torch.zeros(R, ld, device=dev)
    Pb = torch.zeros(R, ld, dtype=torch.bfloat16, device=dev); Pf = torch.zeros(R, ld, device=dev)
    if which in ("all", "bf16"):
        with pytest.raises(SclError):
            ops.softmax_fwd(S, Pb, R, T, ld, Tp)
        with pytest.raises(SclError):
            ops.softmax_bwd(Pb, S, torch.zeros_like(Pb), R, T, ld, Tp)
    if which in ("all", "f32"):
        with pytest.raises(SclError):
            ops.softmax_fwd_f32(S, Pf, R, T, ld, Tp)


# =====================================================================================================================================
# 2. the bf16 training chain, forward and backward
# =====================================================================================================================================
class MatChain:
    """The materialised-score attention of one encoder layer on buffers laid out as Encoder.bufs() lays them out (same slack), the
    logical regions filled with NaN before every run."""

    def __init__(self, dev, B, H, T, D):
        self.dev, self.B, self.H, self.T, self.D = dev, B, H, T, D
        E = H * D
        self.E, self.Tp, self.M = E, up(T, 8), B * T
        self.Mp = up(self.M, 64)
        self.slack = 128 * E
        n = B * H * T * self.Tp
        bfz = lambda k: torch.zeros(k, dtype=torch.bfloat16, device=dev)
        self.S = torch.zeros(n, device=dev)
        self.P, self.dS = bfz(n + 1024), bfz(n + 1024)
        self.qkv = bfz(self.M * 3 * E + self.slack)
        self.ctx = bfz(self.Mp * E)
        self.d_ctx = bfz(self.M * E + self.slack)
        self.dqkv = bfz(self.Mp * 3 * E + self.slack)
        self.n = n

    def load(self, qkv, dctx):
        self.qkv[: self.M * 3 * self.E].copy_(qkv.reshape(-1))
        self.d_ctx[: self.M * self.E].copy_(dctx.reshape(-1))

    def forward(self, p, seed):
        """encoder.py:512-521."""
        B, H, T, D, E, Tp, qkv = self.B, self.H, self.T, self.D, self.E, self.Tp, self.qkv
        self.S.fill_(NAN); self.P[: self.n].fill_(NAN); self.dS[: self.n].fill_(NAN); self.ctx[: self.M * E].fill_(NAN)
        ops.gemm(Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), self.S, T, T, D,
                 nb1=B, nb2=H, alpha=D ** -0.5, ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp)
        ops.softmax_fwd(self.S, self.P, B * H * T, T, Tp, Tp)
        Pv = self.P
        if p > 0:
            Pv = self.dS
            ops.dropout_rows(self.P, Pv, B * H * T, T, Tp, seed, p)
        ops.gemm(Op(Pv, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E),
                 self.ctx, T, D, T, b_t=True, nb1=B, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D)
        return self.ctx[: self.M * E].view(B, T, E)

    def backward(self, p, seed):
        """encoder.py:773-794 (after forward(): P holds the layer's probabilities)."""
        B, H, T, D, E, Tp, qkv, dqkv, d_ctx = self.B, self.H, self.T, self.D, self.E, self.Tp, self.qkv, self.dqkv, self.d_ctx
        dqkv[: self.M * 3 * E].fill_(NAN)
        Pn = self.P
        bq = dict(nb1=B, nb2=H)
        Pv = Pn
        if p > 0:
            Pv = self.dS
            ops.dropout_rows(Pn, Pv, B * H * T, T, Tp, seed, p)
        ops.gemm(Op(Pv, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(d_ctx, E, bs1=T * E, bs2=D), dqkv, T, D, T, a_t=True, b_t=True,
                 ldc=3 * E, c_bs1=T * 3 * E, c_bs2=D, c_offset=2 * E, **bq)
        ops.gemm(Op(d_ctx, E, bs1=T * E, bs2=D), Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E), self.S, T, T, D,
                 ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp, **bq)
        if p > 0:
            ops.dropout_rows(self.S, self.S, B * H * T, T, Tp, seed, p)      # in place on the f32 buffer
        ops.softmax_bwd(Pn, self.S, self.dS, B * H * T, T, Tp, Tp)
        sc = D ** -0.5
        dS = Op(self.dS, Tp, bs1=H * T * Tp, bs2=T * Tp)
        ops.gemm(dS, Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), dqkv, T, D, T, b_t=True, alpha=sc, ldc=3 * E,
                 c_bs1=T * 3 * E, c_bs2=D, c_offset=0, **bq)
        ops.gemm(dS, Op(qkv, 3 * E, bs1=T * 3 * E, bs2=D, offset=0), dqkv, T, D, T, a_t=True, b_t=True, alpha=sc, ldc=3 * E,
                 c_bs1=T * 3 * E, c_bs2=D, c_offset=E, **bq)
        return dqkv[: self.M * 3 * E].view(B, T, 3, H, D)

    def run(self, p, seed):
        ctx = self.forward(p, seed).clone()
        dqkv = self.backward(p, seed).clone()
        torch.cuda.synchronize()
        return ctx, dqkv


def make_inputs(B, H, T, D, seed, amp=0.7):
    gen = g(seed)
    qkv = (amp * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16)
    dctx = torch.randn(B, T, H * D, generator=gen).to(torch.bfloat16)
    return qkv, dctx


def check_against_fp64(tag, ctx, dqkv, qkv, dctx, keep):
    """ctx and the q / k / v thirds of dqkv: rl2(gpu, fp64) <= 2 x rl2(rounding model, fp64) — the factor 2 covers the f32 accumulation
    order and `__expf`, which the model does not reproduce — and max-rel below close_bf16's 3e-2.  Returns the measured figures."""
    ref_ctx, ref_g = AC.attention_fp64(qkv, dctx, keep)
    mod_ctx, mod_g = AC.attention_rounding_model(qkv, dctx, keep)
    rows = [("ctx", ctx, ref_ctx, mod_ctx)] + [("d" + "qkv"[i], dqkv[:, :, i], ref_g[i], mod_g[i]) for i in range(3)]
    out, bad = {}, []
    for name, got, ref, mod in rows:
        e, floor, mr = rl2(got, ref), rl2(mod, ref), maxrel(got, ref)
        out[name] = (e, floor)
        print("%s %-3s rl2 gpu %.3e  model %.3e  ratio %.2f  maxrel %.3e" % (tag, name, e, floor, e / max(floor, 1e-30), mr))
        if ref.abs().max().item() == 0.0:          # one key: dq = dk = 0 exactly in fp64; the chain leaves at most bf16 round-off of dP - dot
            if got.double().abs().max().item() > 1e-2 * ref_g[2].abs().max().item():
                bad.append((name, "not zero"))
            continue
        if not (e <= 2.0 * floor and mr < CLOSE_BF16_MAXREL):
            bad.append((name, e, floor, mr))
    assert not bad, (tag, bad)
    return out


def keep_for(B, H, T, p, seed=SEED):
    return None if p == 0 else keep_scale(seed, B * H * T * T, p).view(B, H, T, T)


CHAIN_CASES = [(64, 2, 3, 225), (64, 2, 16, 249), (64, 1, 4, 256), (64, 1, 4, 257), (64, 2, 2, 320), (64, 1, 16, 505), (64, 2, 4, 511),
               (64, 2, 16, 512), (32, 3, 4, 18), (32, 2, 4, 201), (32, 2, 4, 300)]


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("D,B,H,T", CHAIN_CASES)
def test_mat_chain_against_fp64(dev, D, B, H, T, drop_p):
    qkv, dctx = make_inputs(B, H, T, D, T * 7 + H)
    ch = MatChain(dev, B, H, T, D)
    ch.load(qkv.to(dev), dctx.to(dev))
    ctx, dqkv = ch.run(drop_p, SEED)
    check_against_fp64("D=%d B=%d H=%d T=%d p=%.1f" % (D, B, H, T, drop_p), ctx, dqkv, qkv, dctx, keep_for(B, H, T, drop_p))
    ctx2, dqkv2 = ch.run(drop_p, SEED)      # a second launch writes the same bits
    assert torch.equal(ctx, ctx2) and torch.equal(dqkv, dqkv2)


def test_mat_chain_on_wide_scores(dev):
    """2.0 N(0,1) operands: |S| up to ~22, soft-max rows close to one-hot."""
    D, B, H, T = 64, 1, 4, 257
    qkv, dctx = make_inputs(B, H, T, D, 77, amp=2.0)
    ch = MatChain(dev, B, H, T, D)
    ch.load(qkv.to(dev), dctx.to(dev))
    for p in (0.0, 0.1):
        ctx, dqkv = ch.run(p, SEED)
        check_against_fp64("wide scores T=257 p=%.1f" % p, ctx, dqkv, qkv, dctx, keep_for(B, H, T, p))


def long_path(dev, qkv, dctx, B, H, T, p, seed):
    D, E = 64, H * 64
    ctx = torch.full((B, T, E), NAN, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    ops.attn_fwd_long(qkv, ctx, lse, B, T, H, D, D ** -0.5, drop_p=p, drop_seed=seed)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    dqkv = torch.full((B, T, 3, H, D), NAN, dtype=torch.bfloat16, device=dev)
    ops.attn_bwd_long(qkv, ctx, dctx, lse, dqkv, ws, B, T, H, D, D ** -0.5, drop_p=p, drop_seed=seed)
    torch.cuda.synchronize()
    return ctx, dqkv


def fused_path(dev, qkv, dctx, B, H, T, p, seed):
    D, E = 64, H * 64
    ctx = torch.full((B, T, E), NAN, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    ops.attn_fwd(qkv, ctx, lse, B, T, H, D, D ** -0.5, drop_p=p, drop_seed=seed)
    dqkv = torch.full((B, T, 3, H, D), NAN, dtype=torch.bfloat16, device=dev)
    ops.attn_bwd(qkv, ctx, dctx, lse, dqkv, B, T, H, D, D ** -0.5, drop_p=p, drop_seed=seed)
    torch.cuda.synchronize()
    return ctx, dqkv


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,T", [(2, 4, 201), (1, 4, 224)] + [c[1:] for c in CHAIN_CASES if c[0] == 64])
def test_mat_chain_agrees_with_the_streaming_and_fused_kernels(dev, B, H, T, drop_p):
    """The three attention implementations on the same inputs and the same seed.  Each pair must agree within the SUM of the two paths'
    bars against fp64: 2 x the rounding model's distance for the materialised chain, and test_long_attention_kernels_against_fp64's
    rel-L2 bars (1.2e-2 for ctx, 2.5e-2 for dq / dk / dv) for the streaming kernels and for the fused kernels (which that test holds
    within 5e-3 / 1e-2 of the streaming ones).  A keep-mask indexed differently shows up as an error of order sqrt(p) = 0.3."""
    D = 64
    qkv, dctx = make_inputs(B, H, T, D, T * 7 + H)
    keep = keep_for(B, H, T, drop_p)
    ref_ctx, ref_g = AC.attention_fp64(qkv, dctx, keep)
    mod_ctx, mod_g = AC.attention_rounding_model(qkv, dctx, keep)
    ch = MatChain(dev, B, H, T, D)
    qd, dd = qkv.to(dev), dctx.to(dev)
    ch.load(qd, dd)
    ctx, dqkv = ch.run(drop_p, SEED)
    others = [("streaming", long_path(dev, qd, dd, B, H, T, drop_p, SEED))]
    if T <= 224:
        others.append(("fused", fused_path(dev, qd, dd, B, H, T, drop_p, SEED)))
    bad = []
    for name, (octx, odqkv) in others:
        e = rl2(ctx, octx)
        bar = 2.0 * rl2(mod_ctx, ref_ctx) + LONG_RL2_CTX
        print("T=%d p=%.1f %s vs materialised: ctx rl2 %.3e (bar %.3e)" % (T, drop_p, name, e, bar))
        if not e <= bar:
            bad.append((name, "ctx", e, bar))
        for i in range(3):
            e = rl2(dqkv[:, :, i], odqkv[:, :, i])
            bar = 2.0 * rl2(mod_g[i], ref_g[i]) + LONG_RL2_DQKV
            print("T=%d p=%.1f %s vs materialised: d%s rl2 %.3e (bar %.3e)" % (T, drop_p, name, "qkv"[i], e, bar))
            if not e <= bar:
                bad.append((name, "d" + "qkv"[i], e, bar))
    assert not bad, bad


# =====================================================================================================================================
# 3. training and scoring batch sizes
# =====================================================================================================================================
# GPU memory at (B, H, T) = (128, 16, 512), the largest case: S f32 128 x 16 x 512 x 512 x 4 = 2 GiB (its last utterance starts
# 2^31 - 2^24 bytes in and ends at 2^31: batch offsets beyond 2^31 bytes from (64, 16, 512)'s 1 GiB on for element-indexed kernels), P and
# dS bf16 1 GiB each, qkv and dqkv 384 MiB each, ctx and d_ctx 128 MiB each, the clones of ctx / dqkv 0.5 GiB, the streaming kernels' outputs
# at (64, 16, 512) 0.3 GiB: about 6 GiB.  The host holds qkv / dctx of FOUR utterances and their fp64 attention (16 x 512 x 512 x 8 B
# = 32 MiB per utterance and tensor).
def twin_inputs(dev, B, H, T, D, seed):
    qkv4, dctx4 = make_inputs(4, H, T, D, seed)
    rep = B // 4
    qkv = qkv4.to(dev).repeat(rep, 1, 1, 1, 1)         # qkv[b] = qkv[b % 4]
    dctx = dctx4.to(dev).repeat(rep, 1, 1)
    return qkv4, dctx4, qkv, dctx


@pytest.mark.parametrize("B,H,T", [(64, 16, 512), (128, 16, 512), (64, 16, 249)])
def test_mat_chain_at_training_batch_sizes_twins(dev, B, H, T):
    """qkv[b] = qkv[b % 4], dctx likewise, no dropout: every (b, h) is an independent problem of the same shape, so every utterance's
    ctx and dqkv must be BIT-EQUAL to its twin among the first four, and the first four (all heads) are held to fp64 as in part 2.
    No utterance goes unchecked."""
    D = 64
    qkv4, dctx4, qkv, dctx = twin_inputs(dev, B, H, T, D, 31 + T)
    ch = MatChain(dev, B, H, T, D)
    ch.load(qkv, dctx)
    del qkv, dctx
    ctx, dqkv = ch.run(0.0, SEED)
    check_against_fp64("twins B=%d T=%d" % (B, T), ctx[:4].cpu(), dqkv[:4].cpu(), qkv4, dctx4, None)
    c = ctx.view(B // 4, 4, -1); dq = dqkv.view(B // 4, 4, -1)
    same_c = (c == c[:1]).all(2); same_d = (dq == dq[:1]).all(2)
    assert same_c.all() and same_d.all(), ("utterances that differ from their twin (ctx, dqkv)",
                                           (~same_c).nonzero().tolist()[:8], (~same_d).nonzero().tolist()[:8])


def test_mat_chain_at_training_batch_size_with_dropout(dev):
    """(64, 16, 512), attention dropout 0.1, twinned operands: the masks differ per utterance.  Utterances {0, 1, 2, 3, 31, 32, 63}
    against fp64 (the base utterance's operands under the utterance's OWN mask), and EVERY utterance against the streaming kernels'
    output of the same launch shape at the cross-path bar of part 2."""
    B, H, T, D, p = 64, 16, 512, 64, 0.1
    qkv4, dctx4, qkv, dctx = twin_inputs(dev, B, H, T, D, 31 + T)
    ch = MatChain(dev, B, H, T, D)
    ch.load(qkv, dctx)
    ctx, dqkv = ch.run(p, SEED)
    floors = None
    for b in (0, 1, 2, 3, 31, 32, B - 1):
        keep = keep_scale_range(SEED, b * H * T * T, H * T * T, p).view(1, H, T, T)
        out = check_against_fp64("dropout B=64 T=512 utterance %d" % b, ctx[b: b + 1].cpu(), dqkv[b: b + 1].cpu(), qkv4[b % 4: b % 4 + 1],
                                 dctx4[b % 4: b % 4 + 1], keep)
        floors = {k: max(v[1], floors[k] if floors else 0.0) for k, v in out.items()}
    lctx, ldqkv = long_path(dev, qkv, dctx, B, H, T, p, SEED)
    per = lambda a, b_: ((a.float() - b_.float()).flatten(1).norm(dim=1) / b_.float().flatten(1).norm(dim=1)).cpu()
    e = per(ctx, lctx)
    bar = 2.0 * floors["ctx"] + LONG_RL2_CTX
    print("every utterance vs streaming: ctx rl2 max %.3e (bar %.3e)" % (e.max().item(), bar))
    assert (e <= bar).all(), ("ctx", (e > bar).nonzero().flatten().tolist(), e.max().item())
    for i in range(3):
        e = per(dqkv[:, :, i], ldqkv[:, :, i])
        bar = 2.0 * floors["d" + "qkv"[i]] + LONG_RL2_DQKV
        print("every utterance vs streaming: d%s rl2 max %.3e (bar %.3e)" % ("qkv"[i], e.max().item(), bar))
        assert (e <= bar).all(), ("d" + "qkv"[i], (e > bar).nonzero().flatten().tolist(), e.max().item())


# =====================================================================================================================================
# 4. the fp32 scoring chain
# =====================================================================================================================================
def f32_chain(dev, qkv, B, H, T, D, x3):
    """encoder.py:643-647 on f32 operands; buffers as Encoder.forward_f32 sizes them, Pm filled with NaN: the kernel writes the pads."""
    E, Tp, M = H * D, up(T, 8), B * T
    slack = 128 * E
    n = B * H * T * Tp
    qb = torch.zeros(M * 3 * E + slack, device=dev)
    qb[: M * 3 * E].copy_(qkv.reshape(-1))
    S = torch.full((n,), NAN, device=dev)
    Pm = torch.zeros(n + 1024, device=dev); Pm[:n].fill_(NAN)
    ctx = torch.zeros(M * E + slack, device=dev); ctx[: M * E].fill_(NAN)
    ops.gemm(Op(qb, 3 * E, bs1=T * 3 * E, bs2=D), Op(qb, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), S, T, T, D, nb1=B, nb2=H, alpha=D ** -0.5,
             ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp, x3=x3)
    ops.softmax_fwd_f32(S, Pm, B * H * T, T, Tp, Tp)
    ops.gemm(Op(Pm, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(qb, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E), ctx, T, D, T, b_t=True,
             nb1=B, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D, x3=x3)
    torch.cuda.synchronize()
    return S.view(B, H, T, Tp), Pm[:n].view(B, H, T, Tp), ctx[: M * E].view(B, T, E)


@pytest.mark.parametrize("x3", [None, False])
@pytest.mark.parametrize("D,B,H,T", [(64, 64, 16, 201), (64, 64, 16, 199), (64, 2, 16, 249), (64, 3, 2, 505), (64, 2, 4, 512), (32, 2, 4, 300)])
def test_f32_scoring_chain_against_fp64(dev, D, B, H, T, x3):
    """x3 = None: the default pair form; False: the exact kernel.  S at test_f32_operand_kernel_matches_fp64's bar for the kernel form
    (max-abs error over the tensor's max-abs); P at test_long_f32_softmax_rows' 1e-5 against the fp64 soft-max of the scores the kernel
    was given (the same arithmetic as there: the GEMM's own error in S is held by the first check); ctx at 4 x the error of a plain fp32
    torch attention on the CPU, never below the GEMM bar.  Batch 64: utterances twinned as in part 3, the first four against fp64."""
    pair = ops.F32X3 if x3 is None else bool(x3)
    nb = min(B, 4)
    qkv4 = 0.7 * torch.randn(nb, T, 3, H, D, generator=g(T + H))
    qkv = qkv4.to(dev).repeat(B // nb, 1, 1, 1, 1) if B > nb else qkv4.to(dev)
    S, Pm, ctx = f32_chain(dev, qkv, B, H, T, D, x3)
    if B > nb:
        for t in (S, Pm, ctx):
            v = t.reshape(B // nb, nb, -1)
            same = torch.isclose(v, v[:1], rtol=0, atol=0, equal_nan=True).all(2)      # S's pad columns are never written (NaN)
            assert same.all(), (~same).nonzero().tolist()[:8]
    assert (Pm[..., T:] == 0).all()
    q, k, v = AC._heads(qkv4)
    S64 = (q * D ** -0.5) @ k.transpose(-1, -2)
    Sg = S[:nb, :, :, :T].cpu()
    eS = maxrel(Sg, S64)
    eP = maxrel(Pm[:nb, :, :, :T], torch.softmax(Sg.double(), -1))
    ref = AC._merge(torch.softmax(S64, -1) @ v)
    qf, kf, vf = (t.float() for t in (q, k, v))
    cpu32 = AC._merge(torch.softmax((qf * D ** -0.5) @ kf.transpose(-1, -2), -1) @ vf)
    eC, eCpu = maxrel(ctx[:nb], ref), maxrel(cpu32, ref)
    bar = max(4.0 * eCpu, F32_GEMM_BAR[pair])
    print("f32 chain D=%d B=%d H=%d T=%d %s: S %.2e  P %.2e  ctx %.2e (fp32 CPU %.2e, bar %.2e)" %
          (D, B, H, T, "pair" if pair else "exact", eS, eP, eC, eCpu, bar))
    assert eS < F32_GEMM_BAR[pair], eS
    assert eP < F32_SOFTMAX_MAXREL, eP
    assert eC <= bar, (eC, bar)


# =====================================================================================================================================
# 5. the shipped call chain, through the model
# =====================================================================================================================================
ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
CONF = {"model": {"contra_mode": "all", "loss_type": 1}}
SMALL = dict(conv_dim=32, embed=128, layers=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)
FRAMES = {72100: 225, 82400: 257, 163840: 511, 164000: 512}
GRADS = ("ssl_model.model.encoder.layers.0.self_attn.q_proj.weight", "ssl_model.model.encoder.layers.0.self_attn.v_proj.weight",
         "ssl_model.model.encoder.layers.1.self_attn.k_proj.weight", "ssl_model.model.encoder.layers.1.self_attn.out_proj.weight",
         "ssl_model.model.feature_extractor.conv_layers.2.0.weight", "LL.weight")
DROP_GRADS = ("ssl_model.model.encoder.layers.0.self_attn.q_proj.weight", "ssl_model.model.encoder.layers.0.self_attn.v_proj.weight",
              "ssl_model.model.encoder.layers.0.self_attn.q_proj.bias", "ssl_model.model.encoder.layers.0.self_attn.out_proj.bias",
              "ssl_model.model.encoder.layers.1.self_attn.k_proj.weight", "ssl_model.model.encoder.layers.1.self_attn.out_proj.weight",
              "ssl_model.model.encoder.layers.0.fc1.weight", "ssl_model.model.encoder.layers.0.fc1.bias", "ssl_model.model.encoder.layers.1.fc2.weight",
              "ssl_model.model.encoder.layers.1.fc2.bias", "ssl_model.model.encoder.layers.1.final_layer_norm.weight",
              "ssl_model.model.post_extract_proj.weight", "ssl_model.model.post_extract_proj.bias", "ssl_model.model.encoder.pos_conv.0.weight_v",
              "ssl_model.model.feature_extractor.conv_layers.2.0.weight")


def small_model(dev, heads, **cfg_kw):
    ocfg = W.W2VConfig(heads=heads, **SMALL)
    cfg = W2VConfig(heads=heads, **SMALL, **cfg_kw)
    ssl, head = W.init_state(ocfg, seed=41), OH.init_head(ocfg.embed, seed=42)
    m = Model(ARGS, dev, w2v_cfg=cfg)
    sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
    sd.update(head)
    m.load_state_dict(sd, strict=False)
    return m, ssl, head, ocfg, cfg


def test_clip_lengths_give_the_frame_counts():
    cfg = W2VConfig(heads=2, **SMALL)
    assert {L: cfg.conv_lens(L)[-1] for L in FRAMES} == FRAMES


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("L", sorted(FRAMES))
def test_model_takes_the_materialised_path_and_matches_oracle(dev, L, heads):
    """test_model_gpu.py::test_head_dim_64_config_uses_fused_attention_and_matches_oracle's config, oracle call and bars, eval mode, four
    clips of 225 / 257 / 511 / 512 frames, 64-wide (heads = 2) and 32-wide (heads = 4) heads."""
    m, ssl, head, ocfg, cfg = small_model(dev, heads)
    m.eval()
    x = 0.1 * torch.randn(4, L, generator=g(3))
    y = torch.tensor([1, 1, 0, 0])
    out, feats, emb = m(x.to(dev))
    bufs = m.encoder.bufs(4, L)
    assert bufs["T"] == FRAMES[L] and not bufs["fused_attn"] and not bufs["long_attn"]
    losses = m.loss(out, feats, emb, y.to(dev), CONF)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    ref_losses, ref_grads, (ro, rf, re), _ = OH.train_step(ssl, head, ocfg, x, y)
    print("T=%d heads=%d rl2 out %.2e feats %.2e emb %.2e" % (FRAMES[L], heads, rl2(out, ro), rl2(feats, rf), rl2(emb, re)))
    assert close_bf16(out, ro) and close_bf16(feats, rf) and close_bf16(emb, re), (rl2(feats, rf), maxrel(feats, rf))
    for k, v in ref_losses.items():
        assert abs(losses[k].item() - v) <= 2e-2 * max(abs(v), 1e-3), (k, losses[k].item(), v)
    for name in GRADS:
        c = cosine(m.P.g(name), ref_grads[name])
        assert c > (0.99 if name == "LL.weight" else 0.995), (name, c)


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("L", [82400, 164000])
@pytest.mark.parametrize("probs", [(0.1, 0.1, 0.1, 0.1), (0.0, 0.15, 0.05, 0.0)])
def test_model_dropout_on_the_materialised_path_matches_oracle_given_the_same_masks(dev, probs, L, heads):
    """test_dropout_gpu.py::test_encoder_dropout_matches_the_oracle_given_the_same_masks at 257 and 512 frames: train mode, three steps,
    the last two replayed from launch plans; the masks rebuilt on the host and handed to the oracle; that test's bars."""
    m, ssl, head, ocfg, cfg = small_model(dev, heads, dropout=probs[0], attention_dropout=probs[1], activation_dropout=probs[2],
                                          dropout_input=probs[3])
    m.train()
    B, T = 4, FRAMES[L]
    x = 0.1 * torch.randn(B, L, generator=g(3))
    y = torch.tensor([1, 1, 0, 0])
    for step in range(3):
        out, feats, emb = m(x.to(dev))
        losses = m.loss(out, feats, emb, y.to(dev), CONF)
        for p_ in m.parameters():
            p_.grad = None
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        if step == 1:
            continue
        bufs = m.encoder.bufs(B, L)
        assert bufs["T"] == T and not bufs["fused_attn"] and not bufs["long_attn"]
        step_seed = m._step_seed
        enc_masks = AC.enc_masks_for(step_seed, cfg, B, T, probs)
        head_masks = [keep_scale((step_seed + 7919 * j) & 0x7FFFFFFF, B * T * 128, DROP_P).view(B, T, 128) for j in range(3)]
        ref_losses, ref_grads, (ro, rf, re), _ = OH.train_step(copy.deepcopy(ssl), copy.deepcopy(head), ocfg, x, y, lr=0.0, wd=0.0,
                                                               dropout_masks=head_masks, enc_masks=enc_masks)
        print("T=%d heads=%d step %d rl2 feats %.2e emb %.2e out %.2e" % (T, heads, step, rl2(feats, rf), rl2(emb, re), rl2(out, ro)))
        assert rl2(feats, rf) < 1.5e-2 and rl2(emb, re) < 2e-2 and rl2(out, ro) < 2e-2, (step, rl2(feats, rf), rl2(emb, re), rl2(out, ro))
        for k, v in ref_losses.items():
            assert abs(losses[k].item() - v) <= 3e-2 * max(abs(v), 1e-3), (step, k, losses[k].item(), v)
        for name in DROP_GRADS:
            c = cosine(m.P.g(name), ref_grads[name])
            assert c > 0.99, (step, name, c)


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("L", [82400, 164000])
def test_model_fp32_scoring_forward_matches_oracle(dev, L, heads):
    """The fp32 scoring forward (Encoder.forward_f32: scl_softmax_fwd_f32) at 257 and 512 frames against OH.full_forward at
    test_fp32_scoring_path_matches_oracle_to_1e3_at_xlsr_shape's 1e-3 max-rel bar."""
    m, ssl, head, ocfg, cfg = small_model(dev, heads)
    m.eval()
    x = 0.1 * torch.randn(4, L, generator=g(3))
    with torch.no_grad():
        ro, rf, re = OH.full_forward(ssl, head, ocfg, x)
        out, feats, emb = m(x.to(dev))
    assert ("f32", 4, L) in m.encoder._bufs
    print("fp32 scoring T=%d heads=%d: max-rel logp %.2e emb %.2e feats %.2e" % (FRAMES[L], heads, maxrel(out, ro), maxrel(emb, re), maxrel(feats, rf)))
    assert maxrel(out, ro) < 1e-3 and maxrel(emb, re) < 1e-3 and maxrel(feats, rf) < 1e-3


def test_other_head_widths_are_refused_beyond_512_frames(dev):
    """heads = 4 (32-wide) at 513 frames: the SclError of Encoder.bufs, raised on the host before any launch."""
    m, _, _, _, cfg = small_model(dev, 4)
    L = 164000
    while cfg.conv_lens(L)[-1] < 513:
        L += 80
    assert cfg.conv_lens(L)[-1] == 513
    with pytest.raises(SclError, match="streaming attention"):
        m.encoder.bufs(4, L)

