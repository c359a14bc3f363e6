"""The streaming attention for 72- to 128-wide heads (csrc/attention_wide.hip: the bodies of csrc/attn_wide_body.h on a padded head dim
of 96 or 128), at head dims 80 (XLS-R 1B), 96, 120 (XLS-R 2B) and 128, in the fixed, zero-padded and packed row layouts.

  1. the fixed layout against fp64 (tests/attention_cases.py), with and without attention dropout;
  2. the fixed layout against the shipped materialised-score chain (MatChain of tests/test_attention_mat_gpu.py, which takes any D);
  3. the padded layout: the bits of the fixed-layout kernels on each utterance alone, zero rows beyond, NaN in the padded rows unread;
  4. the packed layout: the bits of the padded kernels, the zero tail, the sentinel rows, a second backward launch;
  5. head isolation: columns D..DP-1 of a head's row are the NEXT head's data — NaN in the neighbouring heads changes no bit;
  6. the refusals.

The bars of 1 and 2 are test_attention_mat_gpu.py's cross-path formula, from the reference alone: with floor = the distance of the bf16
rounding model to fp64, 2 floor + 1.2e-2 for ctx and 2 floor + 2.5e-2 for dq / dk / dv (rel-L2), lse to 1e-5.  Everything else is bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from tests import attention_cases as AC  # noqa: E402
from tests.attention_cases import keep_scale_range, rl2  # noqa: E402
from tests.test_attention_mat_gpu import LONG_RL2_CTX, LONG_RL2_DQKV, MatChain  # noqa: E402
from tests.test_attention_packed_gpu import GUARD, check_rows, layout, packed_from, same  # noqa: E402
from tests.test_varlen_train_gpu import SHAPES, _nan_tail, i32  # noqa: E402

NAN = float("nan")
SEED = 0x2468ACE
DIMS = [80, 96, 120, 128]


def inputs(B, H, T, D, seed):
    """0.7 N(0, 1) operands in bf16, as test_attention_packed_gpu.py::_case: qkv [B, T, 3, H, D], dctx [B, T, H * D] (on the host)."""
    gen = torch.Generator().manual_seed(seed)
    qkv = (0.7 * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16)
    dctx = torch.randn(B, T, H * D, generator=gen).to(torch.bfloat16)
    return qkv, dctx


@functools.lru_cache(maxsize=None)
def reference(B, H, T, D, p):
    """Computed once per case and never modified: the inputs, fp64 ctx / (dq, dk, dv) / lse, and the rounding model's distance to fp64."""
    qkv, dctx = inputs(B, H, T, D, T * 7 + H + D)
    keep = None if p == 0 else keep_scale_range(SEED, 0, B * H * T * T, p).view(B, H, T, T)
    ref_ctx, ref_g = AC.attention_fp64(qkv, dctx, keep)
    mod_ctx, mod_g = AC.attention_rounding_model(qkv, dctx, keep)
    q, k, _ = AC._heads(qkv)
    lse = torch.logsumexp((q * D ** -0.5) @ k.transpose(-1, -2), -1)
    floors = [rl2(mod_ctx, ref_ctx)] + [rl2(mod_g[i], ref_g[i]) for i in range(3)]
    return qkv, dctx, ref_ctx, ref_g, lse, floors


def fixed_path(dev, qkv, dctx, B, H, T, D, p=0.0, seed=SEED):
    """scl_attn_fwd_long / scl_attn_bwd_long into NaN-filled outputs -> ctx [B, T, E], lse [B, H, T], dqkv [B, T, 3, H, D]."""
    E, scale = H * D, D ** -0.5
    ctx = torch.full((B, T, E), NAN, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    ops.attn_fwd_long(qkv, ctx, lse, B, T, H, D, scale, drop_p=p, drop_seed=seed)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    dqkv = torch.full((B, T, 3, H, D), NAN, dtype=torch.bfloat16, device=dev)
    ops.attn_bwd_long(qkv, ctx, dctx, lse, dqkv, ws, B, T, H, D, scale, drop_p=p, drop_seed=seed)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


def padded_path(dev, qkv, dctx, klen, B, H, T, D, p=0.0, seed=SEED, ctx_in=None, lse_in=None):
    """scl_attn_fwd_varlen_drop / scl_attn_bwd_varlen likewise; ctx_in / lse_in: what the backward reads instead of the forward's outputs."""
    E, scale = H * D, D ** -0.5
    kl = i32(klen, dev)
    ctx = torch.full((B, T, E), NAN, dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    ops.attn_fwd_varlen_drop(qkv, ctx, lse, kl, B, T, H, D, scale, drop_p=p, drop_seed=seed)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    dqkv = torch.full((B, T, 3, H, D), NAN, dtype=torch.bfloat16, device=dev)
    ops.attn_bwd_varlen(qkv, ctx if ctx_in is None else ctx_in, dctx, lse if lse_in is None else lse_in, kl, dqkv, ws, B, T, H, D, scale,
                        drop_p=p, drop_seed=seed)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


# ---- 1. the fixed layout against fp64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,T", [(2, 3, 1), (2, 3, 63), (2, 2, 130), (1, 2, 577)])
@pytest.mark.parametrize("D", DIMS)
def test_fixed_layout_against_fp64(dev, D, B, H, T, drop_p):
    qkv, dctx, ref_ctx, ref_g, ref_lse, floors = reference(B, H, T, D, drop_p)
    ctx, lse, dqkv = fixed_path(dev, qkv.to(dev), dctx.to(dev), B, H, T, D, drop_p)
    e, bar = rl2(ctx, ref_ctx), 2.0 * floors[0] + LONG_RL2_CTX
    print("D=%d B=%d H=%d T=%d p=%.1f ctx rl2 %.3e (bar %.3e)  lse rl2 %.3e" % (D, B, H, T, drop_p, e, bar, rl2(lse, ref_lse)))
    assert e <= bar, ("ctx", e, bar)
    assert rl2(lse, ref_lse) < 1e-5, rl2(lse, ref_lse)
    for i in range(3):
        got = dqkv[:, :, i]
        if T == 1 and i < 2:      # one key: dq, dk are exactly 0 in fp64; the kernel leaves bf16 round-off of dP - delta (test_long_clip_gpu.py:76)
            assert got.double().abs().max().item() <= 1e-2 * ref_g[2].abs().max().item()
            continue
        e, bar = rl2(got, ref_g[i]), 2.0 * floors[1 + i] + LONG_RL2_DQKV
        print("    d%s rl2 %.3e (bar %.3e)" % ("qkv"[i], e, bar))
        assert e <= bar, ("d" + "qkv"[i], e, bar)
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(dqkv.float()).all()


# ---- 2. against the shipped materialised-score chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("D", [80, 120])
def test_fixed_layout_agrees_with_the_materialised_chain(dev, D, drop_p):
    B, H, T = 2, 2, 300
    qkv, dctx, _, _, _, floors = reference(B, H, T, D, drop_p)
    qd, dd = qkv.to(dev), dctx.to(dev)
    ch = MatChain(dev, B, H, T, D)
    ch.load(qd, dd)
    mctx, mdqkv = ch.run(drop_p, SEED)
    ctx, _, dqkv = fixed_path(dev, qd, dd, B, H, T, D, drop_p)
    e, bar = rl2(ctx, mctx), 2.0 * floors[0] + LONG_RL2_CTX
    print("D=%d p=%.1f streaming vs materialised: ctx rl2 %.3e (bar %.3e)" % (D, drop_p, e, bar))
    assert e <= bar, ("ctx", e, bar)
    for i in range(3):
        e, bar = rl2(dqkv[:, :, i], mdqkv[:, :, i]), 2.0 * floors[1 + i] + LONG_RL2_DQKV
        print("    d%s rl2 %.3e (bar %.3e)" % ("qkv"[i], e, bar))
        assert e <= bar, ("d" + "qkv"[i], e, bar)


# ---- 3. the padded layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,T,klen", SHAPES)
@pytest.mark.parametrize("D", [80, 120])
def test_padded_layout_carries_the_bits_of_the_fixed_kernels_on_each_utterance(dev, D, B, H, T, klen):
    clean, dclean = inputs(B, H, T, D, T * 11 + H + D)
    qkv, dctx = clean.to(dev), dclean.to(dev)
    ctx, lse, dqkv = padded_path(dev, qkv, dctx, klen, B, H, T, D)
    for b, n in enumerate(klen):
        c1, l1, d1 = fixed_path(dev, clean[b:b + 1, :n].contiguous().to(dev), dclean[b:b + 1, :n].contiguous().to(dev), 1, H, n, D)
        assert same(ctx[b, :n], c1[0]) and same(lse[b, :, :n], l1[0]) and same(dqkv[b, :n], d1[0]), (b, n)
        assert (ctx[b, n:] == 0).all() and (lse[b, :, n:] == 0).all() and (dqkv[b, n:] == 0).all(), (b, n)
    # NaN in every padded row of qkv, ctx, dctx and lse: the same bits, so none of them is loaded
    lse_nan = lse.clone()
    for b, n in enumerate(klen):
        lse_nan[b, :, n:] = NAN
    ctx2, lse2, dqkv2 = padded_path(dev, _nan_tail(qkv, klen), _nan_tail(dctx, klen), klen, B, H, T, D, ctx_in=_nan_tail(ctx, klen), lse_in=lse_nan)
    assert same(ctx2, ctx) and same(lse2, lse) and same(dqkv2, dqkv)


# ---- 4. the packed layout (the structure of test_packed_attention_carries_the_bits_of_the_padded_kernels) -------------------------------
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,T,klen", SHAPES)
@pytest.mark.parametrize("D", [80, 120])
def test_packed_layout_carries_the_bits_of_the_padded_kernels(dev, D, B, H, T, klen, drop_p):
    E, scale, seed = H * D, D ** -0.5, 0x13579BD
    qkv, dctx = (t.to(dev) for t in inputs(B, H, T, D, T * 13 + H + D))
    qkv = qkv.view(B, T, 3 * E)
    row0, Mv, Mq = layout(klen, T)
    r0 = i32(row0, dev)
    ctx, lse, dqkv = padded_path(dev, qkv, dctx, klen, B, H, T, D, drop_p, seed)
    dqkv = dqkv.view(B, T, 3 * E)
    # the packed kernels: inputs packed by scl_pack_rows (NaN in the padded source rows and behind row Mq), outputs prefilled with NaN
    qkv_p = packed_from(qkv, klen, row0, Mq, dev)
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


# ---- 5. head isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("klen", [None, [130, 37]], ids=["fixed", "padded"])
@pytest.mark.parametrize("D", [80, 120])
def test_a_head_does_not_read_its_neighbours(dev, D, klen, drop_p):
    """H = 3: the padded columns D..DP-1 of head 1 are head 2's first DP - D columns (head 0's are head 1's, head 2's the next section's or
    the next row's).  Head 1's ctx, lse and dqkv carry the same bits whether heads 0 and 2 of qkv and dctx hold finite values or NaN."""
    B, H, T = 2, 3, 130
    qkv, dctx = (t.to(dev) for t in inputs(B, H, T, D, 5 + D))
    qkv_nan, dctx_nan = qkv.clone(), dctx.clone().view(B, T, H, D)
    qkv_nan[:, :, :, 0] = NAN; qkv_nan[:, :, :, 2] = NAN
    dctx_nan[:, :, 0] = NAN; dctx_nan[:, :, 2] = NAN
    dctx_nan = dctx_nan.view(B, T, H * D)
    run = (lambda q, d: fixed_path(dev, q, d, B, H, T, D, drop_p)) if klen is None else \
          (lambda q, d: padded_path(dev, q, d, klen, B, H, T, D, drop_p))
    ctx, lse, dqkv = run(qkv, dctx)
    ctx_n, lse_n, dqkv_n = run(qkv_nan, dctx_nan)
    head1 = lambda c: c.view(B, T, H, D)[:, :, 1]
    assert torch.isfinite(head1(ctx).float()).all() and torch.isfinite(dqkv[:, :, :, 1].float()).all()
    assert same(head1(ctx_n), head1(ctx)) and same(lse_n[:, 1], lse[:, 1]) and same(dqkv_n[:, :, :, 1], dqkv[:, :, :, 1])
    assert dqkv[:, :, :, 1].float().abs().max() > 0


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 56, 84, 136])
def test_other_head_dims_are_refused(dev, D):
    z = torch.zeros(64 * 3 * 2 * 136, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(4096, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    kl, r0 = i32([4], dev), i32([0, 4], dev)
    calls = [lambda: ops.attn_fwd_long(z, z, f, 1, 4, 2, D, 0.1),
             lambda: ops.attn_bwd_long(z, z, z, f, z, ws, 1, 4, 2, D, 0.1),
             lambda: ops.attn_fwd_varlen(z, z, f, kl, 1, 4, 2, D, 0.1),
             lambda: ops.attn_fwd_varlen_drop(z, z, f, kl, 1, 4, 2, D, 0.1, drop_p=0.1, drop_seed=1),
             lambda: ops.attn_bwd_varlen(z, z, z, f, kl, z, ws, 1, 4, 2, D, 0.1),
             lambda: ops.attn_fwd_packed(z, z, f, r0, 1, 4, 2, D, 64, 0.1),
             lambda: ops.attn_fwd_packed_drop(z, z, f, r0, 1, 4, 2, D, 64, 0.1, drop_p=0.1, drop_seed=1),
             lambda: ops.attn_bwd_packed(z, z, z, f, r0, z, ws, 1, 4, 2, D, 64, 0.1)]
    for call in calls:
        with pytest.raises(SclError, match="head dim 64"):
            call()
