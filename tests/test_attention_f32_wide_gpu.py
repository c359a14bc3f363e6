"""The fp32 streaming attention over packed rows for head dims 72..128 (csrc/attention_f32_wide.hip behind ops.attn_fwd_packed_f32):
tests/test_attention_f32_gpu.py with the head dim as a parameter.  Against fp64 attention on each utterance's own frames, with the
materialised chain of Encoder.forward_f32 (score GEMM, scl_softmax_fwd_f32_varlen, P V GEMM — it takes any head dim) on the same inputs
as the yardstick; bit for bit against a launch of each utterance alone; what is stored where; one row count with other offsets; the
neighbouring head's columns (D..DP-1 of the padded head dim) are never read, with a qkv buffer of exactly Mq x 3 x H x D floats; the
refusals.  D = 80 and 120 (XLS-R 1B / 2B) run every shape of the 64-wide file; 72, 96, 104 and 128 — the last 16-column tile part-valid,
full, skipped and full again — run the 130-frame shape.  Inputs are fp32 0.7 * randn, so the lo planes carry weight."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from scl_amd.ops import Op  # noqa: E402
from tests.test_varlen_train_gpu import SHAPES, i32  # noqa: E402

GUARD = 3      # rows behind the launch's Mq: never touched
NAN = float("nan")
PEAKED = (3, 4, 577, [577, 65, 512])      # with Q x 6: the running maximum moves in later blocks, most exponentials underflow
EDGE = (4, 2, 130, [1, 63, 64, 130])
assert SHAPES[0] == EDGE
CASES = ([(D,) + s + (1.0,) for D in (80, 120) for s in SHAPES] + [(D,) + PEAKED + (6.0,) for D in (80, 120)] +
         [(D,) + EDGE + (1.0,) for D in (72, 96, 104, 128)])
_CASE = {}


def layout(klen, T):
    row0 = [0]
    for n in klen:
        row0.append(row0[-1] + n)
    Mq = (row0[-1] + 63) // 64 * 64
    ops.check_packed_rows(row0, T, Mq)
    return row0, row0[-1], Mq


def padded_inputs(D, B, H, T, qmul):
    """fp32 qkv [B, T, 3, H, D] on the host (finite everywhere: the materialised chain multiplies masked P = 0 by the padded V rows).
    Once per case, never modified."""
    key = (D, B, H, T, qmul)
    if key not in _CASE:
        gen = torch.Generator().manual_seed(T * 13 + H + 1000 * D)
        qkv = 0.7 * torch.randn(B, T, 3, H, D, generator=gen)
        qkv[:, :, 0] *= qmul
        _CASE[key] = qkv
    return _CASE[key]


def fp64_reference(qkv, klen):
    """fp64 attention of every utterance on its own frames, [n, H * D] each."""
    D = qkv.shape[-1]
    refs = []
    for b, n in enumerate(klen):
        q, k, v = (qkv[b, :n, i].double().permute(1, 0, 2) for i in range(3))      # [H, n, D]
        pr = torch.softmax((q @ k.transpose(-1, -2)) * D ** -0.5, -1)
        refs.append((pr @ v).permute(1, 0, 2).reshape(n, -1))
    return refs


def packed_from(qkv, klen, row0, rows, dev):
    """[rows, 3, H, D] on the device: the utterances' valid rows back to back, NaN everywhere else."""
    out = torch.full((rows,) + tuple(qkv.shape[2:]), NAN)
    for b, n in enumerate(klen):
        out[row0[b]:row0[b] + n] = qkv[b, :n]
    return out.to(dev)


def run_packed(qkv, klen, T, dev, Mq=None, r0buf=None):
    B, H, D = qkv.shape[0], qkv.shape[3], qkv.shape[4]
    row0, Mv, Mq0 = layout(klen, T)
    Mq = Mq0 if Mq is None else Mq
    qp = packed_from(qkv, klen, row0, Mq + GUARD, dev)      # NaN in rows [Mv, Mq + GUARD)
    ctx = torch.full((Mq + GUARD, H * D), NAN, device=dev)
    r0 = i32(row0, dev) if r0buf is None else r0buf
    if r0buf is not None:
        r0buf.copy_(i32(row0, dev))
    ops.attn_fwd_packed_f32(qp, ctx, r0, B, T, H, D, Mq, D ** -0.5)
    torch.cuda.synchronize()
    return ctx, row0, Mv, Mq


def alone(qkv, b, n, dev):
    """Utterance b in a launch of its own: B = 1, row0 = [0, n], Mq = roundup(n, 64)."""
    H, D = qkv.shape[3], qkv.shape[4]
    Mq = (n + 63) // 64 * 64
    qp = packed_from(qkv[b:b + 1], [n], [0, n], Mq, dev)
    ctx = torch.full((Mq, H * D), NAN, device=dev)
    ops.attn_fwd_packed_f32(qp, ctx, i32([0, n], dev), 1, n, H, D, Mq, D ** -0.5)
    torch.cuda.synchronize()
    return ctx[:n]


def materialised(qkv, klen, dev):
    """The chain on the padded rectangle: the three launches of Encoder.forward_f32 (ops.F32X3 at its default), at any head dim."""
    B, T, _, H, D = qkv.shape
    E, Tp = H * D, (T + 7) // 8 * 8
    slack = 128 * E
    f32 = lambda n: torch.zeros(n, device=dev)
    q = f32(B * T * 3 * E + slack)
    q[:B * T * 3 * E] = qkv.reshape(-1).to(dev)
    S, Pm, ctx = f32(B * H * T * Tp), f32(B * H * T * Tp + 1024), f32(B * T * E + slack)
    ops.gemm(Op(q, 3 * E, bs1=T * 3 * E, bs2=D), Op(q, 3 * E, bs1=T * 3 * E, bs2=D, offset=E), S, T, T, D, nb1=B, nb2=H,
             alpha=D ** -0.5, ldc=Tp, c_bs1=H * T * Tp, c_bs2=T * Tp)
    ops.softmax_fwd_f32_varlen(S, Pm, i32(klen, dev), B * H * T, H * T, T, Tp, Tp)
    ops.gemm(Op(Pm, Tp, bs1=H * T * Tp, bs2=T * Tp), Op(q, 3 * E, bs1=T * 3 * E, bs2=D, offset=2 * E), ctx, T, D, T, b_t=True,
             nb1=B, nb2=H, ldc=E, c_bs1=T * E, c_bs2=D)
    torch.cuda.synchronize()
    return ctx[:B * T * E].view(B, T, E)


def pooled_rl2(parts, refs):
    num = sum(((g.double().cpu() - r) ** 2).sum().item() for g, r in zip(parts, refs))
    den = sum((r ** 2).sum().item() for r in refs)
    return (num / den) ** 0.5


# ---- 1. against fp64, with the materialised chain as the yardstick --------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,H,T,klen,qmul", CASES)
def test_error_against_fp64_is_within_twice_the_materialised_chains(dev, D, B, H, T, klen, qmul):
    """err_new <= 2 x err_materialised, both rel-L2 against fp64 pooled over the case's valid rows: the 64-wide test's bar."""
    qkv = padded_inputs(D, B, H, T, qmul)
    refs = fp64_reference(qkv, klen)
    ctx, row0, Mv, Mq = run_packed(qkv, klen, T, dev)
    err_new = pooled_rl2([ctx[row0[b]:row0[b] + n] for b, n in enumerate(klen)], refs)
    mat = materialised(qkv, klen, dev)
    err_mat = pooled_rl2([mat[b, :n] for b, n in enumerate(klen)], refs)
    print("D=%d B=%d H=%d T=%d klen=%s q x %g: rel-L2 against fp64, streaming pair-form kernel %.3e, materialised chain %.3e"
          % (D, B, H, T, klen, qmul, err_new, err_mat))
    assert err_mat < 1e-4      # the yardstick itself is an fp32-grade result
    assert err_new <= 2 * err_mat, (err_new, err_mat)


# ---- 2. each utterance gets the bits it gets alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,H,T,klen,qmul", CASES)
def test_each_utterance_gets_the_bits_it_gets_alone(dev, D, B, H, T, klen, qmul):
    qkv = padded_inputs(D, B, H, T, qmul)
    ctx, row0, Mv, Mq = run_packed(qkv, klen, T, dev)      # NaN in qkv rows [Mv, Mq + GUARD) and in all of ctx before the launch
    again, _, _, _ = run_packed(qkv, klen, T, dev)
    assert torch.equal(again[:Mq], ctx[:Mq])      # deterministic
    for b, n in enumerate(klen):
        got = ctx[row0[b]:row0[b] + n]
        assert torch.isfinite(got).all(), (b, n)
        assert torch.equal(got, alone(qkv, b, n, dev)), (b, n)
    assert (ctx[Mv:Mq] == 0).all()                 # rows of the launch that belong to no utterance
    assert torch.isnan(ctx[Mq:]).all()             # rows behind the launch


# ---- 3. one Mq, other offsets in the same device buffer -------------------------------------------------------------------------------------
def test_a_recorded_row_count_serves_other_lengths(dev):
    """Mv is read from row0[B] on the device: the same launch arguments (Mq) with other offsets in the same buffer."""
    D, B, H, T = 80, 4, 2, 130
    qkv = padded_inputs(D, B, H, T, 1.0)
    r0 = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    for klen in ([1, 63, 64, 130], [130, 2, 70, 100], [60, 60, 60, 60]):
        ctx, row0, Mv, Mq = run_packed(qkv, klen, T, dev, Mq=320, r0buf=r0)
        assert r0.tolist() == row0 and Mv < Mq == 320
        for b, n in enumerate(klen):
            assert torch.equal(ctx[row0[b]:row0[b] + n], alone(qkv, b, n, dev)), (klen, b)
        assert (ctx[Mv:Mq] == 0).all() and torch.isnan(ctx[Mq:]).all()


# ---- 4. columns D..DP-1 of the padded head dim are the neighbour's: never read --------------------------------------------------------------
@pytest.mark.parametrize("D", [80, 120])
def test_the_neighbours_columns_are_never_read(dev, D):
    """H = 2: with head 1 of the q, k and v sections NaN, head 0 keeps its bits (its padded columns D..DP-1 are head 1's first
    columns in memory), and the other way round (head 1's padded columns are the next section's head 0, or the next row's q).  Then
    the clean batch from a qkv buffer of exactly Mq x 3 x H x D floats: every index the kernel forms lies inside it by construction."""
    B, H, T, klen = EDGE
    qkv = padded_inputs(D, B, H, T, 1.0)
    row0, Mv, Mq = layout(klen, T)
    clean, _, _, _ = run_packed(qkv, klen, T, dev)
    assert torch.isfinite(clean[:Mv]).all()
    for dead in (1, 0):
        live = 1 - dead
        poisoned = qkv.clone()
        poisoned[:, :, :, dead] = NAN
        got, _, _, _ = run_packed(poisoned, klen, T, dev)
        cols = slice(live * D, (live + 1) * D)
        assert torch.isfinite(got[:Mv, cols]).all(), dead
        assert torch.equal(got[:Mv, cols], clean[:Mv, cols]), dead
    exact = packed_from(qkv, klen, row0, Mq, dev).reshape(-1)
    assert exact.numel() == Mq * 3 * H * D
    ctx = torch.full((Mq, H * D), NAN, device=dev)
    ops.attn_fwd_packed_f32(exact, ctx, i32(row0, dev), B, T, H, D, Mq, D ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(ctx, clean[:Mq])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals(dev):
    qkv = torch.zeros(192 * 3 * 2 * 136, device=dev)
    ctx = torch.zeros(192 * 2 * 136, device=dev)
    r0 = i32([0, 40, 100], dev)
    for D in (32, 136, 76):
        with pytest.raises(SclError, match="head dim 64"):
            ops.attn_fwd_packed_f32(qkv, ctx, r0, 2, 60, 2, D, 128, D ** -0.5)
    with pytest.raises(SclError, match="multiple of 64"):
        ops.attn_fwd_packed_f32(qkv, ctx, r0, 2, 60, 2, 80, 70, 80 ** -0.5)
    ops.attn_fwd_packed_f32(qkv, ctx, r0, 2, 60, 2, 80, 128, 80 ** -0.5)          # and the call they guard
    torch.cuda.synchronize()
    assert (ctx == 0).all()      # zero inputs: uniform soft-max over zero V rows
