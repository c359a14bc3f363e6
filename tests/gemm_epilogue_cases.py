"""The case table of the GEMM epilogue tests (CPU only, no scl_amd import): implementations x store paths x flag sets, and the host
buffers of each case.  tests/test_gemm_ref_cpu.py proves on the CPU that every case's inputs make the mutations of its flag set
visible to the checker; tests/test_gemm_epilogue_gpu.py runs the same cases on the kernels.

Inputs: A, B ~ N(0, K^-1/2) per product, so the accumulator is ~ N(0, 1); bias and R ~ N(0, 1): every epilogue step moves the value by
its own order of magnitude, which is what lets a step in the wrong place show.  Operand buffers are NaN outside the addressed elements
(the rest of a K-contiguous row's last 16-byte vector included: the kernels mask a partial K vector themselves); output buffers are
sentinels with a c_offset prefix, ldc > N, spare rows, gaps between batch entries and a spare slab behind."""
import numpy as np
import torch

from tests.gemm_ref import FLAT, HostOp, operand_offsets, output_offsets

BF, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF, "f32": F32, None: None}

# ---- flag sets: the production ones at their real structure, plus what completes ACT / RACT / dtype / dropout coverage -----------------
FLAGSETS = {
    "plain_bf16":      dict(c="bf16"),                                                               # QKV data gradients (kind 1)
    "bias_bf16":       dict(c="bf16", bias=True),                                                    # QKV forward (kind 1)
    "fc1_fwd":         dict(c="bf16", bias=True, act=5, c2="bf16"),                                  # fc1 forward, stored gelu' (kind 2)
    "fc2_dgrad":       dict(c="bf16", r="bf16", rmode=2, ract=4),                                    # fc2 data gradient (kind 3)
    "resid_f32":       dict(c="f32", bias=True, r="f32", rmode=1),                                   # out-proj / fc2 forward (kind 4)
    "bias_f32":        dict(c="f32", bias=True),                                                     # conv layers, slabs (kind 5 of gemm_epilogue_blk; the wide kernel compiles its kind 5 out: generic loop)
    "relu_f32":        dict(c="f32", bias=True, act=2),                                              # generic loop
    "dropout_bf16":    dict(c="bf16", drop_p=0.25),                                                  # generic loop
    "gelu_c2f32":      dict(c="bf16", bias=True, act=1, c2="f32"),                                   # SCL_GEMM_C2_F32
    "head_fwd":        dict(c="f32", bias=True, act=3, c2="f32", drop_p=0.2),                        # heads: bias + leaky + c2 + dropout
    "head_bwd_relu":   dict(c="f32", r="f32", rmode=2, ract=2),                                      # linear head backward
    "head_bwd_leaky":  dict(c="f32", r="bf16", rmode=2, ract=3, drop_p=0.2),                         # BTSE head backward
    "fc2_dgrad_drop":  dict(c="bf16", r="bf16", rmode=2, ract=4, drop_p=0.1),                        # encoder fc2 data gradient + dropout
    "gelu_grad_alpha": dict(c="bf16", bias=True, alpha=0.3, r="bf16", rmode=2, ract=1),              # alpha with bias, RACT 1
    "resid_bf16r":     dict(c="f32", bias=True, alpha=0.3, r="bf16", rmode=1, drop_p=0.25),          # bf16 R under RMODE 1, dropout + R
}
DEFAULT_FLAGS = dict(c="f32", c2=None, r=None, bias=False, act=0, rmode=0, ract=0, alpha=1.0, drop_p=0.0)

# ---- store paths: (N delta, ldc - N, c_offset) -------------------------------------------------------------------------------------
PATHS = {
    "aligned":    dict(dn=0, pad=8, c_off=8),          # everything aligned: vector path
    "n_odd":      dict(dn=-1, pad=0, c_off=8),         # N % 4 == 3 with ldc = N: element-wise path
    "padded_odd": dict(dn=-1, pad=9, c_off=8),         # padded ldc (% 8 == 0), odd N: both paths in one launch
    "misaligned": dict(dn=0, pad=8, c_off=9),          # C / C2 / R off by one element
    "ldc4":       dict(dn=0, pad=4, c_off=8),          # wide kernel: ldc % 8 == 4: R not through LDS-DMA, vector path on
}

# ---- implementations ------------------------------------------------------------------------------------------------------------------
# M, N: one full tile plus a ragged edge (wide: one tile row + 8 rows, one tile column + 72 columns); Ks: K of one step (64 for the bf16
# kernels, 32 for the f32 kernels), two steps + a tail, one that is no multiple of the 16-byte vector (where the implementation takes it;
# the wide kernel takes whole steps only and runs the least K it accepts)
IMPLS = {
    "t128_reg": dict(sel=dict(no_dma=True), M=136, N=136, Ks=(64, 136, 140), ab="bf16", wide=0),
    "t128_dma": dict(sel=dict(no_w8=True), M=136, N=136, Ks=(64, 136), ab="bf16", wide=0),
    "wide":     dict(sel=dict(force_w8=True), M=264, N=328, Ks=(64,), ab="bf16", wide=1),
    "finish":   dict(sel={}, M=136, N=136, Ks=(0,), ab="bf16", wide=0),
    "f32_64":   dict(sel=dict(x3=False), M=72, N=72, Ks=(32, 70, 38), ab="f32", wide=0),
    "x3_stage": dict(sel=dict(x3=True), M=72, N=72, Ks=(32, 70, 38), ab="f32", wide=0),
    "x3_frag":  dict(sel=dict(x3=True), M=72, N=72, Ks=(32, 70, 38), ab="f32", wide=0, force_t=(False, True)),
}


def _spec(impl, path, fs, i, **over):
    im = IMPLS[impl]
    s = dict(DEFAULT_FLAGS)
    s.update(FLAGSETS[fs] if fs in FLAGSETS else {})
    s.update(impl=impl, path=path, flagset=fs, sel=dict(im["sel"]), ab=im["ab"], M=im["M"], N=im["N"] + PATHS[path]["dn"],
             K=im["Ks"][i % len(im["Ks"])], pad=PATHS[path]["pad"], c_off=PATHS[path]["c_off"], wide=im["wide"], struct="flat",
             nb1=1, nb2=1, splitk=1, colsum=False, seed=1000 + 17 * i)
    # transposes rotate with the flag set where the implementation can address them (LDS-DMA: whole 16-byte vectors along M / N)
    a_t, b_t = im.get("force_t", (i % 4 >= 2, i % 2 == 1))
    if impl == "wide":      # an un-batched launch with K-contiguous A takes the 112-row tile, a transposed A the 208-row tile: rotate with the
        pidx = list(PATHS).index(path)      # path as well, so that every flag set (every epilogue kind) meets both tilings
        a_t, b_t = (i + pidx) % 2 == 1, (i // 2 + pidx) % 2 == 1
    if impl in ("t128_dma", "wide"):
        a_t, b_t = a_t and s["M"] % 8 == 0, b_t and s["N"] % 8 == 0
    if impl in ("x3_stage",):
        a_t = b_t = False
    s.update(a_t=a_t, b_t=b_t)
    s.update(over)
    s["impl"] = s.pop("as_impl", s["impl"])
    if s["wide"] and "kind" not in s:      # what ops.gemm_wide_kind must answer: 1 = 208-row tiles, 2 = 256-row, 4 = 112-row (un-batched, K-contiguous A)
        s["kind"] = 4 if not s["a_t"] and s["nb1"] * s["nb2"] * s["splitk"] == 1 and not s["colsum"] else 1
    s.setdefault("kind", 0)
    s["name"] = "%s-%s-%s" % (s["impl"], s["path"], s["flagset"])
    return s


def all_specs():
    out = []
    for impl in IMPLS:
        paths = [p for p in PATHS if p != "ldc4" or impl == "wide"]
        for path in paths:
            for i, fs in enumerate(FLAGSETS):
                out.append(_spec(impl, path, fs, i, colsum=impl == "wide" and path == "aligned" and fs in ("fc2_dgrad", "fc2_dgrad_drop")))
    # the f32 kernels on their 128 x 128 tiles: 4 tiles x 128 batch entries = 512 (the kernel's threshold), two K steps + a tail
    for path in ("aligned", "n_odd", "padded_odd", "misaligned"):
        big = dict(M=136, N=136 + PATHS[path]["dn"], K=70, nb1=16, nb2=8)
        for i, fs in enumerate(("bias_f32", "head_fwd", "head_bwd_leaky")):
            if path == "aligned" or i == list(PATHS).index(path) - 1:      # all three where everything is aligned, one on each other path
                out.append(_spec("f32_64", path, fs, i, as_impl="f32_128", a_t=False, b_t=False, **big))
        out.append(_spec("x3_stage", path, "head_fwd", 0, as_impl="x3_stage_128", **big))
        out.append(_spec("x3_frag", path, "resid_bf16r", 1, as_impl="x3_frag_128", **big))
    # the wide kernel's 256-row tile: the plan picks it where it saves a round of the CUs (66 batch entries of one ragged 216-row tile
    # x two tile columns: 132 tiles instead of 264 of the 208-row plan)
    for path, fss in (("aligned", ("plain_bf16", "fc2_dgrad", "resid_f32", "relu_f32")), ("padded_odd", ("resid_f32",))):
        for fs in fss:
            out.append(_spec("wide", path, fs, list(FLAGSETS).index(fs), as_impl="wide_256", M=216, nb1=6, nb2=11, a_t=False, b_t=False, kind=2))
    # structured launches on every implementation that takes them
    for impl in ("t128_reg", "t128_dma", "wide", "f32_64", "x3_stage"):
        im = IMPLS[impl]
        wide, f32 = impl == "wide", im["ab"] == "f32"
        k1 = 192 if wide else (38 if f32 else (140 if impl == "t128_reg" else 200))
        out.append(_spec(impl, "aligned", "batch_bias_bs2", 0, c="f32", bias=True, alpha=0.3, nb1=2, nb2=3, a_t=False, b_t=False))
        out.append(_spec(impl, "padded_odd", "batch_bias_bs2", 0, c="bf16", bias=True, alpha=0.3, act=2, nb1=2, nb2=3, a_t=False, b_t=False))
        out.append(_spec(impl, "aligned", "splitk3", 1, c="f32", splitk=3, K=k1, a_t=not f32 and not wide, b_t=not f32))
        out.append(_spec(impl, "n_odd", "splitk3", 1, c="f32", alpha=0.3, splitk=3, K=k1, a_t=False, b_t=False))
        # conv backward-data phase: C = one phase of every s columns, R read through c_rpb / c_rbstride / c_offset
        out.append(_spec(impl, "aligned", "conv_dgrad_phase", 2, struct="dgrad", c="bf16", r="bf16", rmode=2, ract=1, a_t=False, b_t=True,
                         K=64 if not f32 else 40, **({"as_impl": "x3_frag"} if impl == "x3_stage" else {})))      # transposed B: the fragment form
        # grouped positional-conv fallback: R = dx, RMODE 1, ldc = E, c_bs2 = Cg, bias_bs2 = Cg
        if not f32:
            out.append(_spec(impl, "aligned", "posconv_grouped", 3, struct="grouped", c="f32", bias=True, act=1, c2="bf16", r="f32", rmode=1,
                             a_t=False, b_t=False, K=128, nb2=2))
    return out


class Built:
    pass


def _fill(numel, offs, dtype, g, scale):
    """NaN buffer with N(0, scale) at the addressed offsets."""
    buf = torch.full((numel,), float("nan"), dtype=torch.float32)
    uniq = torch.from_numpy(np.unique(offs))
    buf[uniq] = torch.randn(uniq.numel(), generator=g) * scale
    return buf.to(dtype)


def _flat_operand(rows, contig, transposed, dtype, nb1, nb2, g, scale):
    """[rows x contig] logical matrix (contig = K): K-contiguous [rows][ld] or transposed [K][ld], ld padded, 3 spare rows, NaN around."""
    vec = 8 if dtype == BF else 4
    r, c = (contig, rows) if transposed else (rows, contig)
    ld = (c + vec - 1) // vec * vec + vec
    bs2 = (r + 3) * ld
    op = HostOp(None, ld, bs1=nb2 * bs2 if nb1 > 1 else 0, bs2=bs2 if nb2 > 1 else 0)
    offs = operand_offsets(op, r, c, nb1, nb2)
    op.t = _fill(nb1 * nb2 * bs2 + 64, offs, dtype, g, scale)
    return op


def build(s):
    """Host buffers and the keyword arguments of ops.gemm / gemm_ref for one spec."""
    g = torch.Generator().manual_seed(s["seed"])
    b = Built()
    b.spec = s
    M, N, K, nb1, nb2 = s["M"], s["N"], s["K"], s["nb1"], s["nb2"]
    abdt = BF if s["ab"] == "bf16" else F32
    kw = dict(a_t=s["a_t"], b_t=s["b_t"], act=s["act"], rmode=s["rmode"], ract=s["ract"], alpha=s["alpha"], nb1=nb1, nb2=nb2,
              splitk=s["splitk"], drop_p=s["drop_p"], drop_seed=0x5EED0000 + s["seed"] if s["drop_p"] > 0 else 0)
    c_off = s["c_off"]
    if s["struct"] == "flat":
        sc = K ** -0.25 if K else 1.0
        if K:
            b.A = _flat_operand(M, K, s["a_t"], abdt, nb1, nb2, g, sc)
            b.B = _flat_operand(N, K, s["b_t"], abdt, nb1, nb2, g, sc)
        ldc = N + s["pad"]
        ent = (M + 1) * ldc + 8 if ldc % 4 == 0 else (M + 1) * ldc
        kw.update(ldc=ldc, c_offset=c_off)
        if nb2 > 1:
            kw.update(c_bs2=ent)
        if nb1 > 1:
            kw.update(c_bs1=nb2 * ent + 16)
        extent = (nb1 - 1) * kw.get("c_bs1", 0) + nb2 * ent + 16
    elif s["struct"] == "dgrad":
        # M = Bz * Tout rows, written as phase 1 of every s = 2 column blocks of N; A = the padded output gradient, two overlapping taps
        Bz, sdn, Cd = 3, 2, K // 2
        Tout = M // Bz
        M = Bz * Tout
        Tin = sdn * Tout + 1
        b.A = HostOp(None, Cd, rpb=Tout, rbstride=(Tout + 2) * Cd)
        b.A.t = _fill(Bz * (Tout + 2) * Cd + 64, operand_offsets(b.A, M, K, 1, 1), abdt, g, K ** -0.25)
        b.B = _flat_operand(N, K, True, abdt, 1, 1, g, K ** -0.25)
        c_off = 8 + N
        kw.update(ldc=sdn * N, c_rpb=Tout, c_rbstride=Tin * N, c_offset=c_off)
        extent = Bz * Tin * N + sdn * N
    elif s["struct"] == "grouped":
        Bz, G, Cg, Kt = 3, 2, 64, K // 64
        T = M // Bz
        M, N, E = Bz * T, Cg, G * Cg
        b.A = HostOp(None, E, rpb=T, rbstride=(T + Kt) * E, cin=Cg, cout=E, bs2=Cg)
        b.A.t = _fill(Bz * (T + Kt) * E + 64, operand_offsets(b.A, M, K, 1, G), abdt, g, K ** -0.25)
        b.B = HostOp(None, K, bs2=Cg * K)
        b.B.t = _fill(G * Cg * K + 64, operand_offsets(b.B, N, K, 1, G), abdt, g, K ** -0.25)
        nb2 = G
        kw.update(nb2=G, ldc=E + 8, c_bs2=Cg, c_offset=c_off, bias_bs2=Cg)
        extent = (M + 1) * (E + 8)
    else:
        raise ValueError(s["struct"])
    b.M, b.N, b.K = M, N, K
    if s["splitk"] > 1:
        kw.update(c_split_stride=(extent + 31) // 8 * 8)
        extent = (s["splitk"] + 1) * kw["c_split_stride"]          # a spare slab behind the last one
    b.cnumel = c_off + extent + 64
    b.c_dtype, b.c2_dtype = DT[s["c"]], DT[s["c2"]]
    offs = output_offsets(M, N, nb1, nb2, kw["ldc"], kw.get("c_rpb", FLAT), kw.get("c_rbstride", 0), kw.get("c_bs1", 0), kw.get("c_bs2", 0))
    assert offs.max() + kw["c_offset"] + s["splitk"] * kw.get("c_split_stride", 0) < b.cnumel - 32
    b.bias = b.R = None
    if s["bias"]:
        if s["struct"] == "flat" and nb2 > 1:
            kw.update(bias_bs2=N + 4 - N % 4 if N % 4 else N + 4, bias_offset=4)
        bb, bo = kw.get("bias_bs2", 0), kw.get("bias_offset", 0)
        z2 = np.arange(nb2, dtype=np.int64)[:, None]
        b.bias = _fill(bo + nb2 * max(bb, N) + 8, bo + z2 * bb + np.arange(N, dtype=np.int64)[None, :], F32, g, 1.0)
    if s["r"]:
        b.R = _fill(b.cnumel, offs + kw["c_offset"], DT[s["r"]], g, 1.0)
    b.kw = kw
    b.x3 = bool(s["sel"].get("x3", False))
    b.slabs = None
    if s["impl"] == "finish":      # hand-made slabs [3][M][N]: three partial sums of an N(0, 1) accumulator
        b.slabs = torch.randn(3, M, N, generator=g) * 3 ** -0.5
    return b


def reference(b, mutation=None, acc=None):
    """The fp64 reference of a built case (gemm_ref, or finish_ref for the split-K finishing pass over the case's slabs)."""
    from tests.gemm_ref import finish_ref, gemm_ref
    kw = dict(b.kw)
    if b.slabs is not None:
        kw = {k: kw[k] for k in ("act", "rmode", "ract", "ldc", "c_offset", "drop_p", "drop_seed")}
        return finish_ref(b.slabs, b.c_dtype, b.M, b.N, bias=b.bias, c2_dtype=b.c2_dtype, R=b.R, mutation=mutation, **kw)
    return gemm_ref(b.A, b.B, b.c_dtype, b.M, b.N, b.K, bias=b.bias, c2_dtype=b.c2_dtype, R=b.R, colsum=b.spec["colsum"], x3=b.x3,
                    mutation=mutation, acc=acc, **kw)


def applicable(mutation, s):
    """Does this mutation change what a launch of spec s must store?"""
    act, rmode, ract, drop = s["act"], s["rmode"], s["ract"], s["drop_p"] > 0
    finish = s["impl"] == "finish"
    return {
        "bias_after_act": s["bias"] and act != 0,
        "alpha_after_bias": s["bias"] and s["alpha"] != 1.0 and not finish,
        "tanh_gelu": act in (1, 5),
        "leaky_slope_0": act == 3,
        "relu_grad_for_leaky": rmode == 2 and ract == 3,
        "dropout_rowcol_index": drop and (s["pad"] != 0 or s["struct"] != "flat"),
        "dropout_after_residual": drop and rmode == 1,
        "r_one_late": rmode != 0,
        "c2_after_act": s["c2"] is not None and act in (1, 2, 3),
        "acc_bf16": s["c"] == "f32",
        "k_tail_dropped": not finish,
        "store_past_n": True,
        "wrong_bias_row": s["bias"] and s["nb2"] > 1,
    }[mutation]
