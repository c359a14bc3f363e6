"""The persistent wide-tile GEMM (gemm_w8.hip, scl_gemm_persist_w8_kernel) against the one-tile single-barrier kernel (w8s) BIT FOR BIT on the
same descriptors — C, the second output and the column-sum partial rows, sentinel padding included — and against the fp64 descriptor
reference of tests/gemm_ref.py at its existing bounds.

Shapes: the smallest at which the hand-over between two tiles of a block can go wrong.  M = 3 * 206 + 5 = 623 (the plan makes three row
tiles of 208 / 208 / 207 rows: the row limit cuts the last one) and M = 206 (one row tile, two rows cut); N = 256, 768 (1, 3 tile
columns) and 1536 (18 tiles: EVERY one of the 8 forced blocks walks two or three); K = 192 (3 steps, the least the kernel takes), 256
(even step count: the B image parity flips from tile to tile) and 1024; K-contiguous and transposed B.  SCL_W8_PERSIST=8 (read per
launch) forces 8 resident blocks, so block 0 of the 9-tile problems walks two tiles, and the 1- and 3-tile problems leave blocks
without a tile.  Which kernel ran is read from the launch log (variant 8 = persistent, 1 / 2 = one-tile blocks on 208- / 256-row tiles).
The 256-row tile has a test of its own at the smallest problem the plan gives that tile.  (Full row tiles followed by a small
partial one cannot occur: the planner divides M evenly among the row tiles, so the row limit cuts the last tile by a few rows.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from scl_amd.lib import KID_GEMM  # noqa: E402
from tests import gemm_epilogue_cases as GC  # noqa: E402
from tests import gemm_ref as GR  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
EPIS = {      # the epilogue kinds the persistent kernels are built for
    "bias_bf16": dict(c=BF, bias=True),                      # kind 1: QKV forward, plain data gradients
    "fc1_fwd":   dict(c=BF, bias=True, act=5, c2=BF),        # kind 2: gelu + gelu'
    "bias_f32":  dict(c=F32, bias=True),                     # kind 5: conv forward
}
W8S, W8P = 1, 8


@pytest.fixture(autouse=True)
def _wide_208(monkeypatch):
    monkeypatch.setenv("SCL_W8_TILE112", "0")      # the 112-row tile would take these small un-batched launches
    monkeypatch.delenv("SCL_W8_MODE", raising=False)


class _Log:
    """The variants of the GEMM launches issued inside the block."""
    def __enter__(self):
        ops.prof_read(KID_GEMM)
        ops.prof_reserve(KID_GEMM, 4096)
        ops.prof_enable(KID_GEMM, True)
        self.variants = None
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        ops.prof_enable(KID_GEMM, False)
        self.variants = [meta[5] for _, meta in ops.prof_read_launches(KID_GEMM)]
        ops.prof_read(KID_GEMM)
        return False


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _operands(M, N, K, b_t, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    sc = K ** -0.25
    A = (torch.randn(M, K, device=dev, generator=g) * sc).to(BF)
    B = (torch.randn((K, N) if b_t else (N, K), device=dev, generator=g) * sc).to(BF)
    bias = torch.randn(N, device=dev, generator=g)
    return ops.Op(A, K), ops.Op(B, N if b_t else K), bias


def _launch(A, B, bias, M, N, K, b_t, epi, colsum, dev, **over):
    """One launch into sentinel buffers (ldc = N + 8, a prefix and spare rows): returns the raw outputs."""
    e = EPIS[epi] if epi in EPIS else dict(c=F32)      # "plain_f32": no bias (split-K slabs)
    ldc, c_off = N + 8, 8
    numel = c_off + (M + 2) * ldc
    if over.get("splitk", 1) > 1:      # one slab per K split, a spare one behind
        over["c_split_stride"] = numel
        numel *= over["splitk"] + 1
    C = GR.sentinel_buffer(numel, e["c"], dev)
    C2 = GR.sentinel_buffer(numel, e["c2"], dev) if e.get("c2") is not None else None
    kw = dict(b_t=b_t, bias=bias if e.get("bias") else None, act=e.get("act", 0), c2=C2, ldc=ldc, c_offset=c_off, force_w8=True)
    kw.update(over)
    part = None
    if colsum:
        rows = ops.gemm_colsum_rows(A, B, C, M, N, K, **kw)
        assert rows > 0
        part = torch.full((rows, N), float("nan"), device=dev)
        kw.update(colsum_part=part)
    ops.gemm(A, B, C, M, N, K, **kw)
    return [t for t in (C, C2, part) if t is not None]


def _pair(monkeypatch, expect, *args, one_tile=W8S, **kw):
    """The same launch on one-tile blocks and with 8 persistent blocks forced; the variants of both from the launch log."""
    with _Log() as log:
        monkeypatch.setenv("SCL_W8_PERSIST", "0")
        ref = _launch(*args, **kw)
        monkeypatch.setenv("SCL_W8_PERSIST", "8")
        got = _launch(*args, **kw)
    assert log.variants == [one_tile, expect], log.variants
    assert len(ref) == len(got)
    for r, g in zip(ref, got):
        assert torch.equal(_bits(r), _bits(g))


@pytest.mark.parametrize("b_t", [False, True], ids=["NN", "NT"])
@pytest.mark.parametrize("K", [192, 256, 1024])
@pytest.mark.parametrize("M,N", [(623, 256), (623, 768), (206, 256), (206, 768), (623, 1536)])
def test_persistent_blocks_equal_one_tile_blocks_bit_for_bit(dev, monkeypatch, M, N, K, b_t):
    A, B, bias = _operands(M, N, K, b_t, dev, seed=M + N + K + int(b_t))
    for epi in EPIS:
        for colsum in (False, True):
            _pair(monkeypatch, W8P, A, B, bias, M, N, K, b_t, epi, colsum, dev)


@pytest.mark.parametrize("K", [192, 256])
@pytest.mark.parametrize("b_t,epi", [(False, "bias_f32"), (True, "bias_bf16")], ids=["NN-f32", "NT-bf16"])
def test_persistent_256_row_tiles_equal_one_tile_blocks_bit_for_bit(dev, monkeypatch, b_t, epi, K):
    """The conv stack's long launches: the plan takes 256-row tiles where they save a round of the 256 CUs — here 128 x 2 tiles (one
    round) against 158 x 2 of 208 rows (two), the smallest such problem; three rows short, so the row limit cuts the last row tile.
    8 forced blocks walk 32 tiles each.  Built for the conv forward (NN, f32 + bias) and the conv data gradient (NT, bf16) only: any
    other launch on this tiling stays on one-tile blocks."""
    M, N, W8S_256 = 128 * 256 - 3, 512, 2
    A, B, bias = _operands(M, N, K, b_t, dev, seed=K + int(b_t))
    for colsum in (False, True):
        _pair(monkeypatch, W8P, A, B, bias, M, N, K, b_t, epi, colsum, dev, one_tile=W8S_256)
    _pair(monkeypatch, W8S_256, A, B, bias, M, N, K, b_t, "fc1_fwd", False, dev, one_tile=W8S_256)


def test_rejected_launches_fall_back_to_one_tile_blocks(dev, monkeypatch):
    """Two K steps, split-K, both operands transposed, an epilogue with a residual operand: the rule rejects them even when persistent
    blocks are forced; and left to itself it takes no launch with fewer than two tiles per resident block."""
    M, N = 624, 768
    A, B, bias = _operands(M, N, 128, False, dev, seed=5)
    _pair(monkeypatch, W8S, A, B, bias, M, N, 128, False, "bias_bf16", False, dev)                     # nk = 2
    A, B, bias = _operands(M, N, 384, False, dev, seed=6)
    _pair(monkeypatch, W8S, A, B, bias, M, N, 384, False, "plain_f32", False, dev, splitk=2)             # split-K slabs
    At = ops.Op(A.t.t().contiguous(), M)
    Bt = ops.Op(B.t.t().contiguous(), N)
    _pair(monkeypatch, W8S, At, Bt, bias, M, N, 384, True, "bias_f32", False, dev, a_t=True)           # both transposed
    R = torch.randn(8 + (M + 2) * (N + 8), device=dev)
    _pair(monkeypatch, W8S, A, B, bias, M, N, 384, False, "bias_f32", False, dev, R=R, rmode=1)        # kind 4: + R
    monkeypatch.delenv("SCL_W8_PERSIST", raising=False)
    with _Log() as log:
        _launch(A, B, bias, M, N, 384, False, "bias_bf16", False, dev)                                  # 9 tiles on 256 CUs
    assert log.variants == [W8S]


@pytest.mark.parametrize("b_t", [False, True], ids=["NN", "NT"])
@pytest.mark.parametrize("flagset", ["bias_bf16", "fc1_fwd", "bias_f32"])
def test_persistent_blocks_against_fp64_descriptor_reference(dev, monkeypatch, flagset, b_t):
    """The independent check: the case builder and the bounds of tests/test_gemm_epilogue_gpu.py (NaN around the operands, sentinels
    around the outputs), 9 tiles on 8 forced blocks, column sums on."""
    monkeypatch.setenv("SCL_W8_PERSIST", "8")
    i = list(GC.FLAGSETS).index(flagset)
    b = GC.build(GC._spec("wide", "aligned", flagset, i, M=623, N=768, K=256, a_t=False, b_t=b_t, colsum=True, kind=1))
    C = GR.sentinel_buffer(b.cnumel, b.c_dtype, dev)
    C2 = GR.sentinel_buffer(b.cnumel, b.c2_dtype, dev) if b.c2_dtype is not None else None
    A, B = ops.Op(b.A.t.to(dev), b.A.ld, **b.A.kw()), ops.Op(b.B.t.to(dev), b.B.ld, **b.B.kw())
    kw = dict(b.kw, force_w8=True, c2=C2, bias=b.bias.to(dev))
    rows = ops.gemm_colsum_rows(A, B, C, b.M, b.N, b.K, **kw)
    assert rows > 0
    part = torch.full((rows, b.N), float("nan"), device=dev)
    with _Log() as log:
        ops.gemm(A, B, C, b.M, b.N, b.K, colsum_part=part, **kw)
    assert log.variants == [W8P]
    ref = GC.reference(b)
    worst = [GR.check_output(C.cpu(), ref.off, ref.c, ref.c_bound, what="C")]
    if C2 is not None:
        worst.append(GR.check_output(C2.cpu(), ref.off, ref.c2, ref.c2_bound, what="C2"))
    worst.append(GR.check_colsum(part.cpu(), ref))
    print("%s %s: worst |err| / bound %s" % (flagset, "NT" if b_t else "NN", ["%.4f" % w for w in worst]))
    assert max(worst) <= 1.0
