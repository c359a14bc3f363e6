"""The fp64 descriptor interpreter (tests/gemm_ref.py) is right, and its checker bites (CPU only).

1. The interpreter against torch fp64 on the operations the descriptor stands for — F.linear in all four layouts, conv1d as overlapping
   rows, grouped conv1d through the 2-level contiguous index, conv2d through the 2-level index with batch entries, batched QK^T and PV —
   to 1e-12 of the result's scale, output addressing included (the values are scattered to the offsets the interpreter names and read
   back through torch's own strides).
2. Mutations: for every case of the GPU table, every way a kernel's epilogue could be subtly wrong that applies to the case's flags
   is applied to the fp64 reference, rounded as the store would, and must be REJECTED by the same checker the GPU test uses; the
   unmutated reference, rounded, must pass.  A mutation that slips through means the case's inputs hide that step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_epilogue_cases as GC
from tests import gemm_ref as GR
from tests.gemm_ref import HostOp, gemm_ref


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _scatter(ref, numel):
    buf = torch.zeros(numel, dtype=torch.float64)
    buf[torch.from_numpy(ref.off)] = torch.from_numpy(ref.c)
    return buf


def _agree(got, want):
    err = ((got - want).abs().max() / want.abs().max()).item()
    assert err <= 1e-12, err


@pytest.mark.parametrize("a_t,b_t", [(False, False), (False, True), (True, False), (True, True)])
def test_interpreter_matches_linear(a_t, b_t):
    M, N, K = 37, 29, 53
    A, B, bias = _rand((M, K), 1), _rand((N, K), 2), _rand((N + 3,), 3)
    def op(mat, t):
        m = mat.t().contiguous() if t else mat
        buf = torch.full((m.shape[0] + 1, m.shape[1] + 4), float("nan"))
        buf[: m.shape[0], : m.shape[1]] = m
        return HostOp(buf, buf.shape[1])
    ldc = N + 5
    ref = gemm_ref(op(A, a_t), op(B, b_t), torch.float32, M, N, K, a_t=a_t, b_t=b_t, bias=bias, bias_offset=3, alpha=0.75, ldc=ldc, c_offset=7)
    want = 0.75 * (A.double() @ B.double().t()) + bias[3:].double()
    _agree(_scatter(ref, 7 + M * ldc)[7:].view(M, ldc)[:, :N], want)
    # K tail that is no multiple of a vector, both activations of F
    ref = gemm_ref(op(A, a_t), op(B, b_t), torch.float32, M, N, K, a_t=a_t, b_t=b_t, bias=bias, act=1)
    _agree(torch.from_numpy(ref.c).view(M, N), F.gelu(A.double() @ B.double().t() + bias[:N].double()))
    ref = gemm_ref(op(A, a_t), op(B, b_t), torch.float32, M, N, K, a_t=a_t, b_t=b_t, bias=bias, act=3)
    want = F.leaky_relu(A.double() @ B.double().t() + bias[:N].double(), GR.LEAKY)
    _agree(torch.from_numpy(ref.c).view(M, N), want)


def test_interpreter_matches_conv1d_overlapping_rows():
    Bsz, Tin, Cc, Co, k, s = 3, 41, 8, 12, 3, 2
    Tout = (Tin - k) // s + 1
    x, w = _rand((Bsz, Tin, Cc), 4), _rand((Co, Cc, k), 5)
    want = F.conv1d(x.double().transpose(1, 2), w.double(), stride=s).transpose(1, 2)
    wk = w.permute(0, 2, 1).contiguous().view(Co, k * Cc)
    ref = gemm_ref(HostOp(x, s * Cc, rpb=Tout, rbstride=Tin * Cc), HostOp(wk, k * Cc), torch.float32, Bsz * Tout, Co, k * Cc)
    _agree(torch.from_numpy(ref.c).view(Bsz, Tout, Co), want)
    # the transposed convolution's phase split: rows of utterance b at b * c_rbstride, one phase of every s column blocks
    ldc, rb = s * Co, (Tout * s + 1) * Co
    ref = gemm_ref(HostOp(x, s * Cc, rpb=Tout, rbstride=Tin * Cc), HostOp(wk, k * Cc), torch.float32, Bsz * Tout, Co, k * Cc,
                   ldc=ldc, c_rpb=Tout, c_rbstride=rb, c_offset=Co)
    got = _scatter(ref, Bsz * rb + ldc)
    _agree(torch.as_strided(got, (Bsz, Tout, Co), (rb, ldc, 1), Co), want)


def test_interpreter_matches_grouped_conv1d():
    Bsz, G, Cg, kk, T = 2, 3, 8, 4, 19
    Ctot = G * Cg
    xp, wg, bias, R = _rand((Bsz, T + kk, Ctot), 6), _rand((Ctot, Cg, kk), 7), _rand((Ctot,), 8), _rand((Bsz * T, Ctot), 9)
    want = F.conv1d(xp.double().transpose(1, 2), wg.double(), bias.double(), groups=G).transpose(1, 2)[:, :T] + R.double().view(Bsz, T, Ctot)
    wgk = wg.view(G, Cg, Cg, kk).permute(0, 1, 3, 2).contiguous()
    ref = gemm_ref(HostOp(xp, Ctot, rpb=T, rbstride=(T + kk) * Ctot, cin=Cg, cout=Ctot, bs2=Cg), HostOp(wgk, kk * Cg, bs2=Cg * kk * Cg),
                   torch.float32, Bsz * T, Cg, kk * Cg, nb2=G, ldc=Ctot, c_bs2=Cg, bias=bias, bias_bs2=Cg, R=R, rmode=1)
    _agree(_scatter(ref, Bsz * T * Ctot).view(Bsz, T, Ctot), want)


def test_interpreter_matches_conv2d():
    Bz, H, W, C, Co, kh, kw, sh, sw = 3, 21, 18, 16, 24, 3, 3, 2, 1
    x, w, b = _rand((Bz, C, H, W), 10), _rand((Co, C, kh, kw), 11), _rand((Co,), 12)
    want = F.conv2d(x.double(), w.double(), b.double(), stride=(sh, sw), padding=1)
    OH, OW = want.shape[2], want.shape[3]
    Hp, Wp = H + 2, W + 2
    xp = torch.zeros(Bz, Hp, Wp, C); xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    wk = w.permute(0, 2, 3, 1).reshape(Co, kh * kw * C).contiguous()
    ref = gemm_ref(HostOp(xp, sw * C, rpb=OW, rbstride=sh * Wp * C, cin=kw * C, cout=Wp * C, bs1=Hp * Wp * C), HostOp(wk, kh * kw * C),
                   torch.float32, OH * OW, Co, kh * kw * C, nb1=Bz, c_bs1=OH * OW * Co, bias=b)
    _agree(_scatter(ref, Bz * OH * OW * Co).view(Bz, OH, OW, Co).permute(0, 3, 1, 2), want)


def test_interpreter_matches_batched_attention_products():
    Bsz, H, T, D = 2, 3, 23, 8
    qkv = _rand((Bsz, T, 3, H, D), 13)
    q, k, v = (qkv[:, :, i].double() for i in range(3))
    ld = 3 * H * D
    ref = gemm_ref(HostOp(qkv, ld, bs1=T * ld, bs2=D), HostOp(qkv, ld, bs1=T * ld, bs2=D, offset=H * D), torch.float32, T, T, D,
                   nb1=Bsz, nb2=H, alpha=0.125, c_bs1=H * T * T, c_bs2=T * T)
    S = torch.einsum("bihd,bjhd->bhij", q, k) * 0.125
    _agree(_scatter(ref, Bsz * H * T * T).view(Bsz, H, T, T), S)
    Tp = T + 1
    P = torch.zeros(Bsz, H, T, Tp); P[..., :T] = torch.softmax(S, -1).float()
    ref = gemm_ref(HostOp(P, Tp, bs1=H * T * Tp, bs2=T * Tp), HostOp(qkv, ld, bs1=T * ld, bs2=D, offset=2 * H * D), torch.float32, T, D, T,
                   b_t=True, nb1=Bsz, nb2=H, ldc=H * D, c_bs1=T * H * D, c_bs2=D)
    want = torch.einsum("bhij,bjhd->bihd", P[..., :T].double(), v).reshape(Bsz, T, H * D)
    _agree(_scatter(ref, Bsz * T * H * D).view(Bsz, T, H * D), want)


def test_dropout_index_is_the_memory_offset_and_split_k_sums_slabs():
    M, N, K = 9, 7, 16
    A, B = _rand((M, K), 14), _rand((N, K), 15)
    ref = gemm_ref(HostOp(A, K), HostOp(B, K), torch.float32, M, N, K, ldc=N + 3, c_offset=5, drop_p=0.5, drop_seed=77)
    f = GR.dropout_factor(77, (np.arange(M)[:, None] * (N + 3) + np.arange(N)[None, :]).astype(np.int64), 0.5)
    _agree(torch.from_numpy(ref.c).view(M, N), (A.double() @ B.double().t()) * torch.from_numpy(f))
    assert set(np.unique(f)) == {0.0, 2.0}
    ref = gemm_ref(HostOp(A, K), HostOp(B, K), torch.float32, M, N, K, splitk=3, c_split_stride=100)
    slabs = GR.sentinel_buffer(400, torch.float32)
    third = torch.from_numpy(ref.c / 3).float()
    for s in range(3):
        slabs[torch.from_numpy(ref.off) + 100 * s] = third
    assert GR.check_output(slabs, ref.off, ref.c, ref.c_bound, 3, 100) <= 1.0


def test_x3_formula_distance_is_reported():
    M, N, K = 16, 12, 40
    A, B = _rand((M, K), 16), _rand((N, K), 17)
    ref = gemm_ref(HostOp(A, K), HostOp(B, K), torch.float32, M, N, K, x3=True)
    exact = A.double() @ B.double().t()
    d = ((torch.from_numpy(ref.c).view(M, N) - exact).abs().max() / exact.abs().max()).item()
    assert 0 < d < 2.0 ** -14 and abs(d - ref.x3_dist) <= 1e-12      # the dropped lo x lo terms: ~2^-16 per product


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
SPECS = GC.all_specs()


def _store(ref, numel, dtype, which="c"):
    """What a launch computing exactly ref's values would leave in a sentinel buffer (rounded to the store type; slabs: the sum in slab 0)."""
    buf = GR.sentinel_buffer(numel, dtype)
    off = torch.from_numpy(ref.off)
    for s in range(1, ref.nslab):
        buf[off + s * ref.split_stride] = 0.0
    buf[off] = torch.from_numpy(getattr(ref, which)).float().to(dtype)
    stray = getattr(ref, "stray", None)
    if stray is not None:
        buf[stray] = 1.0
    return buf


def _check(b, ref, got_ref):
    """Check the buffers a launch computing got_ref would leave against ref; the worst ratio, or CheckFailed."""
    worst = GR.check_output(_store(got_ref, b.cnumel, b.c_dtype), ref.off, ref.c, ref.c_bound, ref.nslab, ref.split_stride, "C")
    if ref.c2 is not None:
        worst = max(worst, GR.check_output(_store(got_ref, b.cnumel, b.c2_dtype, "c2"), ref.off, ref.c2, ref.c2_bound, what="C2"))
    return worst


def test_the_table_covers_what_the_issue_lists():
    names = [s["name"] for s in SPECS]
    assert len(set(names)) == len(names)
    for impl in ("t128_reg", "t128_dma", "wide", "finish", "f32_64", "f32_128", "x3_stage", "x3_frag", "x3_stage_128", "x3_frag_128"):
        paths = {s["path"] for s in SPECS if s["impl"] == impl}
        assert {"aligned", "padded_odd", "n_odd", "misaligned"} <= paths, impl
    assert any(s["impl"] == "wide" and s["path"] == "ldc4" for s in SPECS)
    for fs in GC.FLAGSETS:      # every flag set on the 112-row and on the 208-row wide tiling
        assert {s["kind"] for s in SPECS if s["impl"] == "wide" and s["flagset"] == fs} >= {1, 4}, fs
    assert any(s["kind"] == 2 for s in SPECS)
    # K of one step, of two steps plus a tail, and one that is no multiple of the 16-byte vector
    for impl, step, vec in (("t128_reg", 64, 8), ("f32_64", 32, 4), ("x3_stage", 32, 4), ("x3_frag", 32, 4)):
        ks = {s["K"] for s in SPECS if s["impl"] == impl}
        assert step in ks and any(k > 2 * step and k % step for k in ks) and any(k % vec for k in ks), (impl, ks)
    for impl in ("f32_128", "x3_stage_128", "x3_frag_128"):
        assert all(s["K"] > 64 for s in SPECS if s["impl"] == impl)
    # the dispatch conditions of csrc/gemm.hip / gemm_f32.hip that the library cannot be asked about at run time
    for s in SPECS:
        if s["impl"] in ("t128_dma", "wide", "wide_256"):      # LDS-DMA staging: no partially valid 16-byte vector in either operand
            assert (s["M"] if s["a_t"] else s["K"]) % 8 == 0 and (s["N"] if s["b_t"] else s["K"]) % 8 == 0, s["name"]
        if s["ab"] == "f32":
            t128 = ((s["M"] + 127) // 128) * ((s["N"] + 127) // 128) * s["nb1"] * s["nb2"] * s["splitk"]
            assert (t128 >= 512 and s["M"] >= 128 and s["N"] >= 128) == s["impl"].endswith("_128"), s["name"]
        if s["impl"].startswith("x3_stage"):
            assert not s["a_t"] and not s["b_t"], s["name"]
        if s["impl"].startswith("x3_frag"):
            assert s["a_t"] or s["b_t"], s["name"]
    for m in GR.MUTATIONS:
        assert any(GC.applicable(m, s) for s in SPECS), m


@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
def test_checker_accepts_the_reference_and_rejects_every_mutation(spec):
    b = GC.build(spec)
    acc = None if b.slabs is not None else GR.accumulate(b.A, b.B, b.M, b.N, b.K, b.kw["a_t"], b.kw["b_t"], b.kw["nb1"], b.kw["nb2"], x3=b.x3)
    ref = GC.reference(b, acc=acc)
    assert (ref.c_bound >= 0).all() and (ref.c_bound[ref.c != 0] > 0).all()      # a zero bound only where a factor is exactly 0
    assert _check(b, ref, ref) <= 1.0
    slipped = []
    for m in GR.MUTATIONS:
        if not GC.applicable(m, spec):
            continue
        try:
            _check(b, ref, GC.reference(b, mutation=m, acc=acc))
            slipped.append(m)
        except GR.CheckFailed:
            pass
    assert not slipped, "mutations the checker accepted: %s" % slipped
