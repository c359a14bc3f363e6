"""The four kernels of csrc/layer_mix.hip, each alone through scl_amd.ops, against fp64 at the shapes and bars of tests/layer_mix_cases.py
(bars derived from the number formats, none measured)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from tests import layer_mix_cases as LM  # noqa: E402

IDS = ["%dx%dx%d" % s for s in LM.KERNEL_SHAPES]


def case(dev, Mt, E, S, g_dtype=torch.float32):
    """states [S] f32 [Mt * E] of different scales, logits spread over a few nats, g = d(mix) in g_dtype; everything also in fp64 on the GPU."""
    gen = torch.Generator().manual_seed(1000 * S + Mt)
    n = Mt * E
    states = [(torch.randn(n, generator=gen) * (0.5 + (l % 5))).to(dev) for l in range(S)]
    logits = (1.5 * torch.randn(S, generator=gen)).to(dev)
    g = (0.01 * torch.randn(n, generator=gen)).to(dev).to(g_dtype)
    s64 = torch.softmax(logits.double(), 0)
    return n, states, logits, g, s64, [h.double() for h in states]


@pytest.mark.parametrize("Mt,E,S", LM.KERNEL_SHAPES, ids=IDS)
def test_fwd_is_the_weighted_sum_to_one_bf16_rounding(dev, Mt, E, S):
    n, states, logits, _, s64, h64 = case(dev, Mt, E, S)
    mix = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=dev)
    ops.layer_mix_fwd(states, logits, mix, n)
    torch.cuda.synchronize()
    y64 = sum(s64[l] * h64[l] for l in range(S))
    mag = sum((s64[l] * h64[l]).abs() for l in range(S))
    excess = ((mix[:n].double() - y64).abs() - (LM.BF16_EPS * y64.abs() + 64 * LM.F32_EPS * mag)).max().item()
    print("fwd %s: worst excess over the bar %.3e" % ((Mt, E, S), excess))
    assert excess <= 0
    assert (mix[n:] == 7.0).all()      # nothing written past n


@pytest.mark.parametrize("Mt,E,S", LM.KERNEL_SHAPES, ids=IDS)
def test_acc_f32_adds_one_state_at_a_time(dev, Mt, E, S):
    n, states, logits, _, s64, h64 = case(dev, Mt, E, S)
    acc = torch.full((n + 8,), 7.0, device=dev)      # the first call overwrites: whatever was there plays no part
    acc64 = torch.zeros(n, dtype=torch.float64, device=dev)
    for l in range(S):
        before = acc[:n].double() if l else acc64
        ops.layer_mix_acc_f32(states[l], logits, l, acc, n, accumulate=l > 0)
        torch.cuda.synchronize()
        term = s64[l] * h64[l]
        want = before + term
        excess = ((acc[:n].double() - want).abs() - 2 * LM.F32_EPS * (before.abs() + term.abs())).max().item()
        assert excess <= 0, (l, excess)
    assert (acc[n:] == 7.0).all()
    # and the whole sum against the forward kernel's bar without its bf16 rounding
    y64 = sum(s64[l] * h64[l] for l in range(S))
    mag = sum((s64[l] * h64[l]).abs() for l in range(S))
    assert ((acc[:n].double() - y64).abs() - 64 * LM.F32_EPS * mag).max().item() <= 0


@pytest.mark.parametrize("g_dtype", [torch.bfloat16, torch.float32], ids=["g_bf16", "g_f32"])
@pytest.mark.parametrize("Mt,E,S", LM.KERNEL_SHAPES, ids=IDS)
def test_bwd_w_gives_the_softmax_jacobian_of_the_dot_products_reproducibly(dev, Mt, E, S, g_dtype):
    n, states, logits, g, s64, h64 = case(dev, Mt, E, S, g_dtype)
    ws = torch.empty(ops.layer_mix_bwd_w_ws_bytes(n, S), dtype=torch.uint8, device=dev)
    runs = []
    for fill in (3.0, -5.0):      # the gradient is overwritten, not accumulated
        da = torch.full((S,), fill, device=dev)
        g_last = torch.full((n + 8,), 7.0, device=dev)
        ops.layer_mix_bwd_w(g, states, logits, g_last, ws, da, n)
        torch.cuda.synchronize()
        runs.append((da.clone(), g_last.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # identical bits
    da, g_last = runs[0]
    g64 = g.double()
    dS = torch.stack([(g64 * h64[l]).sum() for l in range(S)])
    want = s64 * (dS - (s64 * dS).sum())
    err = (da.double() - want).abs().max().item()
    print("bwd_w %s %s: max |da| %.3e, error %.3e" % ((Mt, E, S), g_dtype, want.abs().max().item(), err))
    assert err <= LM.BWD_W_REL * want.abs().max().item()
    wl = s64[-1] * g64
    assert ((g_last[:n].double() - wl).abs() - 2 * LM.F32_EPS * wl.abs()).max().item() <= 0
    assert (g_last[n:] == 7.0).all()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("g_dtype", [torch.bfloat16, torch.float32], ids=["g_bf16", "g_f32"])
@pytest.mark.parametrize("Mt,E,S", LM.KERNEL_SHAPES, ids=IDS)
def test_inject_adds_to_the_f32_gradient_and_rewrites_the_masked_bf16_pair(dev, Mt, E, S, g_dtype, p):
    n, states, logits, g, s64, _ = case(dev, Mt, E, S, g_dtype)
    index, seed = S // 2, 0x1234567
    dx0 = 0.02 * torch.randn(n + 8, generator=torch.Generator().manual_seed(5)).to(dev)
    dx = dx0.clone()
    dxb = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=dev)
    ops.layer_mix_bwd_inject(g, logits, index, dx, dxb, n, seed=seed, p=p)
    torch.cuda.synchronize()
    term = s64[index] * g.double()
    want = dx0[:n].double() + term
    assert ((dx[:n].double() - want).abs() - 2 * LM.F32_EPS * (dx0[:n].double().abs() + term.abs())).max().item() <= 0
    assert torch.equal(dx[n:], dx0[n:]) and (dxb[n:] == 7.0).all()
    # the bf16 side: exactly what scl_dropout_f32 makes of the f32 result under the same seed
    ref_b = torch.empty(n, dtype=torch.bfloat16, device=dev)
    ops.dropout(dx, None, ref_b, n, seed, p)
    torch.cuda.synchronize()
    assert torch.equal(dxb[:n], ref_b)
    if p == 0.0:
        assert torch.equal(dxb[:n], dx[:n].to(torch.bfloat16))
    else:
        dropped = (dxb[:n] == 0).float().mean().item()
        assert 0.05 < dropped < 0.15, dropped
    # f32 only (index 0 behind the loop): same f32 result, no companion
    dx2 = dx0.clone()
    ops.layer_mix_bwd_inject(g, logits, index, dx2, None, n)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
