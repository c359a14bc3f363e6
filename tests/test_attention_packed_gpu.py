"""The packed variable-length layout at kernel level (csrc/attention_packed.hip): valid frames of all utterances back to back, utterance b
at rows row0[b] .. row0[b + 1] - 1.  No tolerance anywhere: the packed attention forward and backward against the padded kernels of
csrc/attention_varlen.hip bit for bit (the same body with other addressing), the zero tail [Mv, Mq), a NaN sentinel behind row Mq and NaN
in everything that must not be read; pack / unpack; the refusals.  The shapes are tests/test_varlen_train_gpu.py's: utterance boundaries
off every tile edge (64 queries, 32 rows, 128 keys) and 1-frame utterances wedged between neighbours."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from tests.test_varlen_train_gpu import SHAPES, i32  # noqa: E402

GUARD = 70      # sentinel rows behind the launch's Mq rows
NAN = float("nan")


def bits(t):
    """The tensor's bit patterns, so that NaN compares equal to itself."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def layout(klen, T):
    row0, Mq = ops.packed_rows(klen, T, 64)
    assert Mq % 64 == 0 and row0[-1] <= Mq
    return row0, row0[-1], Mq


def packed_from(padded, klen, row0, Mq, dev):
    """scl_pack_rows of a padded [B, T, C] tensor whose rows beyond each utterance hold NaN, into Mq + GUARD rows of NaN."""
    B, T, C = padded.shape
    src = padded.clone()
    for b, n in enumerate(klen):
        src[b, n:] = NAN
    dst = torch.full((Mq + GUARD, C), NAN, dtype=padded.dtype, device=dev)
    ops.pack_rows(src, dst, i32(row0, dev), B, T, C, Mq)
    return dst


def check_rows(packed, padded, klen, row0, Mv, Mq, what):
    """Rows of every utterance carry the padded tensor's bits, the tail [Mv, Mq) is zero, the sentinel behind Mq is intact."""
    for b, n in enumerate(klen):
        assert same(packed[row0[b]:row0[b] + n], padded[b, :n]), (what, b, n)
    assert (packed[Mv:Mq] == 0).all(), what
    assert torch.isnan(packed[Mq:].float()).all(), what


def _case(B, H, T, dev):
    D, E = 64, H * 64
    gen = torch.Generator().manual_seed(T * 13 + H)
    qkv = (0.7 * torch.randn(B, T, 3 * E, generator=gen)).to(torch.bfloat16).to(dev)
    dctx = torch.randn(B, T, E, generator=gen).to(torch.bfloat16).to(dev)
    return D, E, qkv, dctx


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,T,klen", SHAPES)
def test_packed_attention_carries_the_bits_of_the_padded_kernels(dev, B, H, T, klen, drop_p):
    D, E, qkv, dctx = _case(B, H, T, dev)
    seed, scale = 0x13579BD, D ** -0.5
    row0, Mv, Mq = layout(klen, T)
    kl, r0 = i32(klen, dev), i32(row0, dev)
    # the padded kernels
    ctx = torch.full((B, T, E), NAN, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    ops.attn_fwd_varlen_drop(qkv, ctx, lse, kl, B, T, H, D, scale, drop_p=drop_p, drop_seed=seed)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    dqkv = torch.full((B, T, 3 * E), NAN, dtype=torch.bfloat16, device=dev)
    ops.attn_bwd_varlen(qkv, ctx, dctx, lse, kl, dqkv, ws, B, T, H, D, scale, drop_p=drop_p, drop_seed=seed)
    # the packed kernels: inputs packed by scl_pack_rows (NaN in the padded source rows and behind row Mq), outputs prefilled with NaN
    qkv_p = packed_from(qkv, klen, row0, Mq, dev)
    check_rows(qkv_p, qkv, klen, row0, Mv, Mq, "pack qkv")
    ctx_p = torch.full((Mq + GUARD, E), NAN, dtype=torch.bfloat16, device=dev)
    lse_p = torch.full((B, H, T), NAN, device=dev)
    if drop_p > 0:
        ops.attn_fwd_packed_drop(qkv_p, ctx_p, lse_p, r0, B, T, H, D, Mq, scale, drop_p=drop_p, drop_seed=seed)
    else:
        ops.attn_fwd_packed(qkv_p, ctx_p, lse_p, r0, B, T, H, D, Mq, scale)
    torch.cuda.synchronize()
    check_rows(ctx_p, ctx, klen, row0, Mv, Mq, "ctx")
    assert same(lse_p, lse)      # the padded space in both layouts: zeros beyond each utterance
    assert torch.isfinite(ctx_p[:Mq].float()).all()
    # backward: ctx as the forward left it (NaN behind Mq), dctx packed likewise
    dctx_p = packed_from(dctx, klen, row0, Mq, dev)
    dqkv_p = torch.full((Mq + GUARD, 3 * E), NAN, dtype=torch.bfloat16, device=dev)
    ws_p = torch.full((ops.attn_long_ws_bytes(B, T, H) // 4,), NAN, device=dev)
    ops.attn_bwd_packed(qkv_p, ctx_p, dctx_p, lse_p, r0, dqkv_p, ws_p, B, T, H, D, Mq, scale, drop_p=drop_p, drop_seed=seed)
    again = torch.full_like(dqkv_p, NAN)
    ops.attn_bwd_packed(qkv_p, ctx_p, dctx_p, lse_p, r0, again, ws_p, B, T, H, D, Mq, scale, drop_p=drop_p, drop_seed=seed)
    torch.cuda.synchronize()
    check_rows(dqkv_p, dqkv, klen, row0, Mv, Mq, "dqkv")
    assert same(again, dqkv_p)
    assert torch.isfinite(dqkv_p[:Mq].float()).all() and dqkv_p[:Mv].float().abs().max() > 0


def test_a_recorded_row_count_serves_other_lengths(dev):
    """Mv is read from row0[B] on the device: the same launch arguments (Mq) with other offsets in the same buffer."""
    B, H, T = 4, 2, 130
    D, E, qkv, _ = _case(B, H, T, dev)
    r0 = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    for klen in ([1, 63, 64, 130], [130, 2, 70, 100], [60, 60, 60, 60]):
        row0, Mv = [0], 0
        for n in klen:
            row0.append(row0[-1] + n)
        Mv, Mq = row0[-1], 320
        ops.check_packed_rows(row0, T, Mq)
        r0.copy_(i32(row0, dev))
        ctx = torch.empty(B, T, E, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, H, T, device=dev)
        ops.attn_fwd_varlen(qkv, ctx, lse, i32(klen, dev), B, T, H, D, D ** -0.5)
        qkv_p = packed_from(qkv, klen, row0, Mq, dev)
        ctx_p = torch.full((Mq + GUARD, E), NAN, dtype=torch.bfloat16, device=dev)
        lse_p = torch.full((B, H, T), NAN, device=dev)
        ops.attn_fwd_packed(qkv_p, ctx_p, lse_p, r0, B, T, H, D, Mq, D ** -0.5)
        torch.cuda.synchronize()
        check_rows(ctx_p, ctx, klen, row0, Mv, Mq, klen)
        assert same(lse_p, lse)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [128, 1024])
@pytest.mark.parametrize("B,T,klen", [(s[0], s[2], s[3]) for s in SHAPES[:1] + SHAPES[3:]] + [(3, 7, [7, 7, 7])])
def test_pack_and_unpack_rows(dev, dtype, C, B, T, klen):
    gen = torch.Generator().manual_seed(C + T)
    x = torch.randn(B, T, C, generator=gen).to(dtype).to(dev)
    row0, Mv, Mq = layout(klen, T)
    packed = packed_from(x, klen, row0, Mq, dev)      # NaN in the padded source rows: not read
    torch.cuda.synchronize()
    check_rows(packed, x, klen, row0, Mv, Mq, "pack")
    back = torch.full((B, T, C), NAN, dtype=dtype, device=dev)
    ops.unpack_rows(packed, back, i32(row0, dev), B, T, C, Mq)
    torch.cuda.synchronize()
    for b, n in enumerate(klen):
        assert same(back[b, :n], x[b, :n]) and (back[b, n:] == 0).all(), (b, n)
    assert same(packed[Mq:], torch.full_like(packed[Mq:], NAN))


def test_the_refusals(dev):
    z = torch.zeros(64 * 3 * 64, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(4096, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    r0 = i32([0, 4], dev)
    with pytest.raises(SclError, match="head dim 64"):
        ops.attn_fwd_packed(z, z, f, r0, 1, 4, 2, 32, 64, 0.1)
    with pytest.raises(SclError, match="head dim 64"):
        ops.attn_fwd_packed_drop(z, z, f, r0, 1, 4, 2, 32, 64, 0.1, drop_p=0.1, drop_seed=1)
    with pytest.raises(SclError, match="head dim 64"):
        ops.attn_bwd_packed(z, z, z, f, r0, z, ws, 1, 4, 2, 32, 64, 0.1)
    for row0, T, Mq in (([0, 5, 3, 9], 8, 64),       # not monotone
                        ([0, 4, 4, 9], 8, 64),       # an utterance without a frame
                        ([0, 9, 12, 13], 8, 64),     # longer than T
                        ([0, 60, 120, 180], 64, 128)):      # row0[B] > Mq
        with pytest.raises(SclError, match="packed"):
            ops.check_packed_rows(row0, T, Mq)
