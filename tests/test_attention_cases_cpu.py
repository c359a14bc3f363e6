"""tests/attention_cases.py where there is no GPU: the rounding model of the materialised-score bf16 attention chain against the fp64
reference (the floor that tests/test_attention_mat_gpu.py's bars are multiples of), and the dropout-mask helpers."""
import torch

from tests import attention_cases as AC


def test_rounding_model_floor_at_257_frames():
    """D = 64, T = 257, 0.7 N(0,1) operands, attention dropout 0.1: bf16 stores of P, dS, ctx and dqkv put the chain 2 - 4e-3 (rel-L2)
    from fp64 with cosine 1.0000; a model that rounded nothing would sit at 0 and one that lost a term far above."""
    B, H, T, D, p = 1, 2, 257, 64, 0.1
    gen = torch.Generator().manual_seed(T * 7 + H)
    qkv = (0.7 * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16)
    dctx = torch.randn(B, T, H * D, generator=gen).to(torch.bfloat16)
    keep = AC.keep_scale(0x2468ACE, B * H * T * T, p).view(B, H, T, T)
    assert abs((keep == 0).float().mean().item() - p) < 5e-3
    assert torch.equal(AC.keep_scale_range(0x2468ACE, 1000, 77, p), keep.flatten()[1000:1077])
    for k in (None, keep):
        ref_ctx, ref_g = AC.attention_fp64(qkv, dctx, k)
        mod_ctx, mod_g = AC.attention_rounding_model(qkv, dctx, k)
        for name, mod, ref in [("ctx", mod_ctx, ref_ctx)] + [("d" + "qkv"[i], mod_g[i], ref_g[i]) for i in range(3)]:
            e, c = AC.rl2(mod, ref), AC.cosine(mod, ref)
            print("rounding model %s %-3s rl2 %.3e cos %.6f" % ("p=0.1" if k is not None else "p=0  ", name, e, c))
            assert 1e-3 < e < 5e-3 and c > 0.99999, (name, e, c)
    # the reference itself against plain autograd-free algebra: ctx rows are convex combinations of v when nothing is dropped
    ref_ctx, _ = AC.attention_fp64(qkv)
    v = qkv[:, :, 2].double()
    assert ref_ctx.abs().max() <= v.abs().max()
