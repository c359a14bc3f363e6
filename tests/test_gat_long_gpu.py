"""The tiled pair-score kernels (csrc/gat.hip, graphs of 129 to 1024 nodes) against the torch formulation of tests/test_gat_gpu.py run in
float64 on the GPU: forward 1e-5 and gradients 1e-4 of the tensor's maximum, as test_gat_gpu.py uses.

A parameter gradient here is a sum over up to B * N * N pairs accumulated in fp32.  Where one does not hold 1e-4, the test measures what the
same torch formulation in fp32 loses against float64 on the same inputs, and the bar is 4 x that (both accumulate in fp32; the 4 covers the
different summation order).  Measured on the MI355X (kernel error / fp32 torch error, of the tensor's maximum; every case prints its own):
    (1, 1024, 64, 64, 1024, 1): forward 1.5e-7; dx 3.5e-7 / 2.5e-7, dW 9.7e-7 / 6.8e-6, dbias 9.6e-7 / 4.8e-7, da 3.3e-7 / 2.1e-6
    the five smaller cases: forward <= 2.1e-7, every gradient <= 6.9e-7
so every case holds the 1e-4 bar itself and the 4 x branch is not taken at these sizes."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scl_amd import ops  # noqa: E402
from scl_amd.gat import gat_score  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 1024
FWD_BAR, GRAD_BAR = 1e-5, 1e-4

CASES = [(2, 129, 64, 64, 129, 1),      # first size beyond the whole-graph kernels; ragged last 16-block and j tile
         (3, 144, 64, 32, 100, 3),      # n1 inside the first tile
         (2, 171, 64, 64, 171, 1),      # the 513-frame T layer
         (2, 151, 64, 32, 130, 3),      # the 780-frame heterogeneous layer; n1 in the second tile
         (1, 260, 32, 32, 128, 3),      # two full tiles + 4; n1 on a tile edge
         (1, CAP, 64, 64, CAP, 1)]      # at the cap


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def ref_score(x, W, bias, a, n1):      # tests/test_gat_gpu.py::ref_score
    pair = x.unsqueeze(2) * x.unsqueeze(1)                       # [B, N, N, D]
    h = torch.tanh(torch.nn.functional.linear(pair, W, bias))    # [B, N, N, Do]
    if a.shape[0] == 1:
        return (h @ a[0].unsqueeze(-1)).squeeze(-1)
    board = torch.zeros_like(h[..., 0])
    board[:, :n1, :n1] = (h[:, :n1, :n1] @ a[0].unsqueeze(-1)).squeeze(-1)
    board[:, n1:, n1:] = (h[:, n1:, n1:] @ a[1].unsqueeze(-1)).squeeze(-1)
    board[:, :n1, n1:] = (h[:, :n1, n1:] @ a[2].unsqueeze(-1)).squeeze(-1)
    board[:, n1:, :n1] = (h[:, n1:, :n1] @ a[2].unsqueeze(-1)).squeeze(-1)
    return board


def inputs(dev, B, N, D, Do, n1, na):
    g = torch.Generator().manual_seed(N * 7 + Do)
    x = torch.randn(B, N, D, generator=g).to(dev)
    W = (torch.randn(Do, D, generator=g) / D ** 0.5).to(dev)
    bias = (0.1 * torch.randn(Do, generator=g)).to(dev)
    a = torch.randn(na, Do, generator=g).to(dev)
    gs = torch.randn(B, N, N, generator=g).to(dev)
    return x, W, bias, a, gs


def run_ref(ts, gs, n1, dtype):
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in ts]
    out = ref_score(*leaves, n1)
    out.backward(gs.to(dtype))
    return out.detach(), [t.grad for t in leaves]


def run_kernel(ts, gs, n1):
    leaves = [t.detach().clone().requires_grad_(True) for t in ts]
    out = gat_score(*leaves, n1)
    out.backward(gs)
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("B,N,D,Do,n1,na", CASES)
def test_gat_score_long_fwd_bwd_against_float64(dev, B, N, D, Do, n1, na):
    x, W, bias, a, gs = inputs(dev, B, N, D, Do, n1, na)
    ref, gref = run_ref((x, W, bias, a), gs, n1, torch.float64)
    got, ggot = run_kernel((x, W, bias, a), gs, n1)
    assert got.shape == (B, N, N) and got.dtype == torch.float32
    e_fwd = rel(got, ref)
    errs = [rel(g_, r_) for g_, r_ in zip(ggot, gref)]
    print("gat_long", (B, N, D, Do, n1, na), "fwd %.2e" % e_fwd, "dx %.2e dW %.2e dbias %.2e da %.2e" % tuple(errs))
    assert e_fwd < FWD_BAR, e_fwd
    e32 = None
    for name, e in zip(("dx", "dW", "dbias", "da"), errs):
        if e < GRAD_BAR:
            continue
        if e32 is None:      # what the fp32 torch formulation loses on the same sums
            e32 = dict(zip(("dx", "dW", "dbias", "da"), [rel(g_, r_) for g_, r_ in zip(run_ref((x, W, bias, a), gs, n1, torch.float32)[1], gref)]))
            print("gat_long", (B, N, D, Do, n1, na), "fp32 torch vs float64:", {k: "%.2e" % v for k, v in e32.items()})
        assert e <= 4 * e32[name], (name, e, e32[name])


def test_fp32_torch_formulation_error_is_printed_at_the_cap(dev):
    """The figures the docstring quotes: the kernel's and the fp32 torch formulation's error against float64 at the cap."""
    B, N, D, Do, n1, na = CASES[-1]
    x, W, bias, a, gs = inputs(dev, B, N, D, Do, n1, na)
    _, gref = run_ref((x, W, bias, a), gs, n1, torch.float64)
    _, g32 = run_ref((x, W, bias, a), gs, n1, torch.float32)
    _, ggot = run_kernel((x, W, bias, a), gs, n1)
    for name, k_, t_, r_ in zip(("dx", "dW", "dbias", "da"), ggot, g32, gref):
        ek, et = rel(k_, r_), rel(t_, r_)
        print("gat_long cap %s: kernel %.2e, fp32 torch %.2e" % (name, ek, et))
        assert ek < max(GRAD_BAR, 4 * et), (name, ek, et)


def test_same_call_twice_gives_the_same_bits(dev):
    B, N, D, Do, n1, na = CASES[3]
    x, W, bias, a, gs = inputs(dev, B, N, D, Do, n1, na)
    o1, g1 = run_kernel((x, W, bias, a), gs, n1)
    o2, g2 = run_kernel((x, W, bias, a), gs, n1)
    assert torch.equal(o1, o2)
    for p, q in zip(g1, g2):
        assert torch.equal(p, q)


def test_beyond_the_cap_is_an_error_that_names_it(dev):
    x, W, bias, a, gs = inputs(dev, 1, CAP + 1, 64, 64, CAP + 1, 1)
    with pytest.raises(SclError, match=str(CAP)):
        gat_score(x, W, bias, a, CAP + 1)
    s = torch.empty(1, CAP + 1, CAP + 1, device=dev)
    a3 = torch.zeros(3, 64, device=dev)
    with pytest.raises(SclError, match=str(CAP)):      # the backward entry on its own (no allocation of its scratch: refused before any use)
        ops.gat_score_bwd(x, W, bias, a3, gs, s, s, torch.empty_like(x), 1, CAP + 1, 64, 64, CAP + 1)


def test_scalar_fallback_beyond_128_nodes_is_still_refused(dev):
    B, N, D, Do, n1, na = 2, 129, 32, 17, 100, 3
    x, W, bias, a, gs = inputs(dev, B, N, D, Do, n1, na)
    with pytest.raises(SclError, match="N <= 128"):
        gat_score(x, W, bias, a, n1)


def test_nblocks_unchanged_up_to_128_nodes():
    for N in range(1, 129):
        assert ops.gat_score_nblocks(N) == (N * N + 255) // 256
