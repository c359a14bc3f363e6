"""SclGemmDesc in float64: a plain numpy interpreter of the GEMM descriptor as include/scl_hip.h documents it (CPU only, no scl_amd
import).  It is the anchor of the GEMM tests: it shares no code with any kernel, and the bit-identity tests of tests/test_gemm_gpu.py
inherit their meaning from the kernels it checks.

    ref = gemm_ref(A, B, C_dtype, M, N, K, <the keyword arguments of ops.gemm>, <host copies of bias / R>)

A, B are HostOp (the fields of ops.Op over a CPU tensor).  The result names, for C and C2 (and colsum_part), the set of element offsets
the launch must write, the fp64 value of each and a per-element error bound; check_output() compares a buffer with it and with the
sentinel everywhere else.

What is interpreted
-------------------
* operand addressing: offset(r, c) = (r // rpb) * rbstride + (r % rpb) * ld + (c // cin) * cout + c % cin, plus z1 * bs1 + z2 * bs2
  (z1 = z // nb2, z2 = z % nb2) plus `offset`; rows are M / N (K-contiguous operand) or K (transposed operand).
* output addressing: offset(z, m, n) = c_offset + z1 * c_bs1 + z2 * c_bs2 + slab * c_split_stride + (m // c_rpb) * c_rbstride +
  (m % c_rpb) * ldc + n.  R and C2 use C's offsets; bias is bias[bias_offset + z2 * bias_bs2 + n].
* epilogue, in the documented order: t = alpha * acc; t += bias; C2 = t (ACT 5: C2 = gelu'(t)); t = act(t) (1 / 5 erf-GELU, 2 ReLU,
  3 leaky 0.01); RMODE 2: t *= act'(R) (RACT 1..3 name the activation, RACT 4: R holds the derivative); t *= dropout factor;
  RMODE 1: t += R; store f32 or bf16.
* dropout: factor = dropout_scale(seed, index, p) with index = the element's offset from the descriptor's C pointer (the offset above
  without c_offset: ops.gemm folds c_offset into the pointer), NOT row * N + col.
* split-K: the checked value is the sum over the slabs; which K range lands in which slab is the kernel's business.
* colsum_part: sum over rows of the f32 value the epilogue stores to C (before a bf16 store rounds it), partial rows summed.
* SCL_GEMM_F32X3: the kernel's formula, read in csrc/gemm_f32.hip (f32_split8 / f32_split4): hi = bf16(a) round-to-nearest-even,
  lo = bf16(a - hi) (a - hi is exact in f32), acc = sum_k (a_hi b_lo + a_lo b_hi + a_hi b_hi); the lo x lo term is dropped.  The value
  compared with the kernel is this formula in fp64; its distance to the exact product is returned separately (x3_dist).

Bounds (derived, not measured).  u = 2^-24 (one f32 round-to-nearest), U = 2^-23.
* Accumulator, bf16 operands.  A bf16 x bf16 product has 16 significant bits: exact in f32.  A sum of K exact terms in any order with
  K - 1 roundings obeys |acc - S| <= (K - 1) u (1 + O(K u)) sum|a_k b_k|; K * U * sum|a_k b_k| is twice that and so also covers an adder
  that truncates (one U per addition) instead of rounding.
* Accumulator, exact-f32 operands: each product is rounded once more: (K + 1) * U * sum|a_k b_k|.
* X3: 3 K exact bf16 products: 3 K * U * sum(|a_hi b_lo| + |a_lo b_hi| + |a_hi b_hi|), against the formula value.
* split-K slabs: slab s holds the rounded alpha * acc_s of its K range; acc_s obeys the accumulator bound over that range, and the
  ranges' bounds add up to at most the whole K's.  The rounding of alpha * acc_s is <= u |alpha| (|acc_s| + its bound) <= u |alpha|
  sum_{k in s} |a_k b_k| (1 + K U); over the slabs: u |alpha| sum_k |a_k b_k|, the factor 1 + K U inside the accumulator bound's spare
  half.  The allowance does not use |S|: the partial sums may cancel.
* split-K finish over given slabs: the inputs are the f32 slabs, summed in f32: nslabs * U * sum_s |slab_s|.
* Epilogue.  (v, e) = (fp64 value, bound so far).  Every arithmetic step maps e through its Lipschitz factor and adds one f32 rounding
  of the running magnitude, rnd = u * (|v'| + e'):
    alpha:    e' = |alpha| e + rnd                      bias:  e' = e + rnd
    GELU:     e' = 1.13 e + |gelu_poly(v) - gelu_erf(v)| + 16 U max(|v|, 1)        (max gelu' = 1.129)
    ReLU:     e' = e (continuous, Lipschitz 1: no exclusion near 0)   leaky: e' = e + rnd  (slope = the f32 constant 0.01f)
    x act'(R): g is a function of an input read exactly; RACT 2 / 3 / 4: g exact, e' = |g| e + rnd; RACT 1: g = gelu'(r) carries
              dg = |gelu'_poly(r) - gelu'_erf(r)| + 16 U max(|r|, 1), e' = |g| e + (|v| + e) dg + rnd
    dropout:  f = 0 or 1 / (1 - p) computed in f32 as the kernel does, e' = f e + rnd         + R:  e' = e + rnd
  The kernels' GELU is the Abramowitz-Stegun 7.1.26 polynomial (csrc/common.h::gelu_parts); the reference evaluates that polynomial AND
  the erf form in fp64: the allowance is their difference at the reference's own argument, plus 16 f32 ulp of max(|x|, 1) for the
  counted roundings of gelu_parts (one multiply, fma, rcp, exp, four fma, three multiplies, the subtraction, the final multiply / fma).
  C2 under ACT 5: e' = 0.8 e + |gelu'_poly - gelu'_erf| + 16 U max(|v|, 1)  (max |gelu''| = 2 phi(0) = 0.798).
* f32 store: the value is already f32, nothing added.  bf16 store: + 2^-8 |ref|.  (Round-to-nearest-even to 8 significant bits errs
  by <= 2^-8 |x| at the value x = ref +- e the kernel rounds, i.e. <= 2^-8 |ref| + 2^-8 e; the second term, 0.4 % of e, lies inside
  the factor two that e holds in hand over the K - 1 rounding adder: see the accumulator bound.  Measured ratios of bf16 outputs
  therefore approach 1: the bound is the rounding itself.)
* colsum: sum_rows e(f32 value) + M * u * sum_rows |v|  (M - 1 f32 additions in any order).
Nothing is excluded from a comparison."""
import math

import numpy as np
import torch

from tests.attention_cases import keep_scale_range

FLAT = 0x7fffffff
u24 = 2.0 ** -24
U23 = 2.0 ** -23
LEAKY = float(np.float32(0.01))
SQRT1_2 = float(np.float32(0.70710678118654752))
INV_SQRT_2PI = float(np.float32(0.39894228040143268))

def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


class HostOp:
    """The fields of scl_amd.ops.Op over a CPU tensor (bf16 or f32)."""
    __slots__ = ("t", "ld", "rpb", "rbstride", "cin", "cout", "bs1", "bs2", "offset")

    def __init__(self, t, ld, rpb=FLAT, rbstride=0, cin=FLAT, cout=0, bs1=0, bs2=0, offset=0):
        self.t, self.ld, self.rpb, self.rbstride = t, ld, rpb, rbstride
        self.cin, self.cout, self.bs1, self.bs2, self.offset = cin, cout, bs1, bs2, offset

    def kw(self):
        return dict(rpb=self.rpb, rbstride=self.rbstride, cin=self.cin, cout=self.cout, bs1=self.bs1, bs2=self.bs2, offset=self.offset)


def operand_offsets(op, rows, contig, nb1, nb2):
    """int64 [nb1 * nb2, rows, contig]: element offsets of one operand."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(contig, dtype=np.int64)[None, :]
    o = (r // op.rpb) * op.rbstride + (r % op.rpb) * op.ld + (c // op.cin) * op.cout + c % op.cin
    z = np.arange(nb1 * nb2, dtype=np.int64)
    return (op.offset + (z // nb2) * op.bs1 + (z % nb2) * op.bs2)[:, None, None] + o[None]


def output_offsets(M, N, nb1, nb2, ldc, c_rpb, c_rbstride, c_bs1, c_bs2):
    """int64 [nb1 * nb2, M, N]: offsets from the descriptor's C pointer (c_offset and the slab term not included)."""
    m = np.arange(M, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    o = (m // c_rpb) * c_rbstride + (m % c_rpb) * ldc + n
    z = np.arange(nb1 * nb2, dtype=np.int64)
    return ((z // nb2) * c_bs1 + (z % nb2) * c_bs2)[:, None, None] + o[None]


def _gather(op, rows, contig, nb1, nb2):
    flat = op.t.reshape(-1).double().numpy()
    return flat[operand_offsets(op, rows, contig, nb1, nb2)]


def _bf16(x):
    """fp64 array -> nearest-even bf16 of its f32 value, as fp64."""
    return torch.from_numpy(np.ascontiguousarray(x)).float().to(torch.bfloat16).double().numpy()


def dropout_factor(seed, idx, p):
    """csrc/common.h::dropout_scale at element indices idx (any shape) -> fp64 factors (0 or the f32 value of 1 / (1 - p))."""
    return keep_scale_range(seed, 0, int(idx.max()) + 1, p).double().numpy()[idx]


# ---- GELU: the erf form and the kernels' polynomial, both in fp64 ---------------------------------------------------------------------
def gelu_erf(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad_erf(x):
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _poly_parts(x):
    """gelu_parts with its f32 constants, evaluated in fp64: (cdf, e)."""
    c = [float(np.float32(v)) for v in (0.3275911, 1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
    z = np.abs(x) * SQRT1_2
    t = 1.0 / (c[0] * z + 1.0)
    e = np.exp(-(z * z))
    p = t * c[1] + c[2]
    p = t * p + c[3]
    p = t * p + c[4]
    p = t * p + c[5]
    half_tail = 0.5 * (t * p) * e
    return np.where(x >= 0, 1.0 - half_tail, half_tail), e


def gelu_poly(x):
    return x * _poly_parts(x)[0]


def gelu_grad_poly(x):
    cdf, e = _poly_parts(x)
    return x * INV_SQRT_2PI * e + cdf


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _gelu_allow(x):
    return np.abs(gelu_poly(x) - gelu_erf(x)) + 16 * U23 * np.maximum(np.abs(x), 1.0)


def _gelu_grad_allow(x):
    return np.abs(gelu_grad_poly(x) - gelu_grad_erf(x)) + 16 * U23 * np.maximum(np.abs(x), 1.0)


class Ref:
    """off: int64 offsets into the C / C2 / R buffers (c_offset included, slab 0); c, c_bound (and c2, c2_bound): fp64 per offset;
    nslab / split_stride: the written set is off + s * split_stride, s < nslab, the value is the sum over s; colsum / colsum_bound:
    fp64 [N]; x3_dist: max |formula - exact| / max |exact| of the accumulator (X3 only)."""
    def __init__(self, **kw):
        self.c2 = self.c2_bound = self.colsum = self.colsum_bound = self.x3_dist = None
        self.nslab, self.split_stride = 1, 0
        self.__dict__.update(kw)


MUTATIONS = ("bias_after_act", "alpha_after_bias", "tanh_gelu", "leaky_slope_0", "relu_grad_for_leaky", "dropout_rowcol_index",
             "dropout_after_residual", "r_one_late", "c2_after_act", "acc_bf16", "k_tail_dropped", "store_past_n", "wrong_bias_row")


def epilogue(S, e, off_rel, c_offset, N, *, c_dtype, c2_dtype=None, bias_zn=None, act=0, R=None, rmode=0, ract=0, alpha=1.0,
             drop_p=0.0, drop_seed=0, mutation=None, bias_zn_wrong=None):
    """(S, e): fp64 accumulator and its bound, any shape [Z, M, N]; off_rel: offsets from the C pointer; R: CPU tensor (the whole
    buffer) or None; bias_zn: fp64 [Z, 1, N] or None.  Returns (c, c_bound, c2, c2_bound, v_f32, e_f32)."""
    alpha = float(np.float32(alpha))
    mut = mutation
    rnd = lambda v, e: u24 * (np.abs(v) + e)
    if mut == "acc_bf16":
        S = _bf16(S)
    b = bias_zn
    if mut == "wrong_bias_row":
        b = bias_zn_wrong
    if mut == "alpha_after_bias" and b is not None:
        v = alpha * (S + b)
        e = abs(alpha) * e
    else:
        v = alpha * S
        e = abs(alpha) * e
        e = e + rnd(v, e)
        if b is not None and mut != "bias_after_act":
            v = v + b
            e = e + rnd(v, e)
    pre, pre_e = v, e
    gelu = gelu_tanh if mut == "tanh_gelu" else gelu_erf
    if act in (1, 5):
        e = 1.13 * e + _gelu_allow(v)
        v = gelu(v)
    elif act == 2:
        v = np.maximum(v, 0.0)
    elif act == 3:
        v = np.where(v > 0, v, (0.0 if mut == "leaky_slope_0" else LEAKY) * v)
        e = e + rnd(v, e)
    elif act != 0:
        raise ValueError("ACT %d" % act)
    if mut == "bias_after_act" and b is not None:
        v = v + b
    c2 = c2_bound = None
    if c2_dtype is not None:
        if act == 5:
            c2 = gelu_grad_erf(pre)
            c2_bound = 0.8 * pre_e + _gelu_grad_allow(pre)
        else:
            c2, c2_bound = (v, e) if mut == "c2_after_act" else (pre, pre_e)
        if c2_dtype == torch.bfloat16:
            c2_bound = c2_bound + 2.0 ** -8 * np.abs(c2)
    r = None
    if rmode:
        rflat = R.reshape(-1).double().numpy()
        r = rflat[off_rel + c_offset + (1 if mut == "r_one_late" else 0)]
    if rmode == 2:
        if ract == 1:
            g, dg = gelu_grad_erf(r), _gelu_grad_allow(r)
        elif ract == 2:
            g, dg = np.where(r > 0, 1.0, 0.0), 0.0
        elif ract == 3:
            g, dg = np.where(r > 0, 1.0, 0.0 if mut == "relu_grad_for_leaky" else LEAKY), 0.0
        elif ract == 4:
            g, dg = r, 0.0
        else:
            raise ValueError("RACT %d" % ract)
        e = np.abs(g) * e + (np.abs(v) + e) * dg
        v = v * g
        e = e + rnd(v, e)
    if mut == "dropout_after_residual" and rmode == 1:
        v = v + r
    if drop_p > 0.0:
        idx = off_rel
        if mut == "dropout_rowcol_index":
            Z, M, Nn = S.shape
            idx = np.broadcast_to(np.arange(M, dtype=np.int64)[:, None] * N + np.arange(Nn, dtype=np.int64)[None, :], S.shape)
        f = dropout_factor(drop_seed, idx, drop_p)
        v = v * f
        e = f * e
        e = e + rnd(v, e)
    if rmode == 1 and mut != "dropout_after_residual":
        v = v + r
        e = e + rnd(v, e)
    elif rmode not in (0, 1, 2):
        raise ValueError("RMODE %d" % rmode)
    c_bound = e + (2.0 ** -8 * np.abs(v) if c_dtype == torch.bfloat16 else 0.0)
    return v, c_bound, c2, c2_bound, v, e


def accumulate(A, B, M, N, K, a_t, b_t, nb1, nb2, x3=False, mutation=None):
    """fp64 [Z, M, N] accumulator, its bound, (X3) the formula's distance to the exact product, and sum_k |a_k b_k|."""
    a = _gather(A, K if a_t else M, M if a_t else K, nb1, nb2)
    b = _gather(B, K if b_t else N, N if b_t else K, nb1, nb2)
    a = a.transpose(0, 2, 1) if a_t else a      # [Z, M, K]
    b = b.transpose(0, 2, 1) if b_t else b      # [Z, N, K]
    assert np.isfinite(a).all() and np.isfinite(b).all(), "the descriptor addresses an element outside the operand's data"
    if mutation == "k_tail_dropped":
        a, b = a[:, :, :K - 1], b[:, :, :K - 1]
    f32 = A.t.dtype == torch.float32
    x3_dist = None
    if f32 and x3:
        ah, bh = _bf16(a), _bf16(b)
        al, bl = _bf16(a - ah), _bf16(b - bh)
        mm = lambda x, y: np.matmul(x, y.transpose(0, 2, 1))
        S = mm(ah, bl) + mm(al, bh) + mm(ah, bh)
        absS = mm(np.abs(ah), np.abs(bl)) + mm(np.abs(al), np.abs(bh)) + mm(np.abs(ah), np.abs(bh))
        e = 3 * K * U23 * absS
        exact = mm(a, b)
        x3_dist = float(np.abs(S - exact).max() / max(np.abs(exact).max(), 1e-300))
    else:
        S = np.matmul(a, b.transpose(0, 2, 1))
        absS = np.matmul(np.abs(a), np.abs(b).transpose(0, 2, 1))
        e = (K + 1 if f32 else K) * U23 * absS
    return S, e, x3_dist, absS


def gemm_ref(A, B, c_dtype, M, N, K, *, a_t=False, b_t=False, bias=None, act=0, c2_dtype=None, R=None, rmode=0, ract=0, alpha=1.0,
             nb1=1, nb2=1, splitk=1, ldc=None, c_rpb=FLAT, c_rbstride=0, c_bs1=0, c_bs2=0, c_offset=0, bias_bs2=0, bias_offset=0,
             drop_p=0.0, drop_seed=0, c_split_stride=0, colsum=False, x3=False, mutation=None, acc=None):
    """The descriptor ops.gemm(A, B, C, M, N, K, ...) builds, interpreted in fp64.  bias / R: CPU tensors (whole buffers).
    acc: the result of accumulate() for the same operands, to share it among several epilogues."""
    ldc = N if ldc is None else ldc
    if acc is None or mutation == "k_tail_dropped":
        acc = accumulate(A, B, M, N, K, a_t, b_t, nb1, nb2, x3=x3, mutation=mutation)
    S, e, x3_dist, absS = acc
    off_rel = output_offsets(M, N, nb1, nb2, ldc, c_rpb, c_rbstride, c_bs1, c_bs2)
    assert len(np.unique(off_rel)) == off_rel.size, "the descriptor writes an element twice"
    bias_zn = bias_wrong = None
    if bias is not None:
        bf = bias.reshape(-1).double().numpy()
        z2 = np.arange(nb1 * nb2, dtype=np.int64) % nb2
        n = np.arange(N, dtype=np.int64)
        bias_zn = bf[bias_offset + z2[:, None] * bias_bs2 + n[None, :]][:, None, :]
        bias_wrong = bf[bias_offset + ((z2 + 1) % nb2)[:, None] * bias_bs2 + n[None, :]][:, None, :]
    if splitk > 1:
        assert bias is None and act == 0 and rmode == 0 and c2_dtype is None and c_dtype == torch.float32 and drop_p == 0.0
    c, cb, c2, c2b, vf, ef = epilogue(S, e, off_rel, c_offset, N, c_dtype=c_dtype, c2_dtype=c2_dtype, bias_zn=bias_zn, act=act, R=R,
                                      rmode=rmode, ract=ract, alpha=alpha, drop_p=drop_p, drop_seed=drop_seed, mutation=mutation,
                                      bias_zn_wrong=bias_wrong)
    if splitk > 1:
        cb = cb + u24 * abs(float(np.float32(alpha))) * absS      # the roundings of alpha * acc_s, slab by slab (docstring)
    ref = Ref(off=(off_rel + c_offset).reshape(-1), c=c.reshape(-1), c_bound=np.broadcast_to(cb, c.shape).reshape(-1), nslab=splitk,
              split_stride=c_split_stride, x3_dist=x3_dist, N=N, c_dtype=c_dtype, c2_dtype=c2_dtype)
    if c2 is not None:
        ref.c2, ref.c2_bound = c2.reshape(-1), np.broadcast_to(c2b, c2.shape).reshape(-1)
    if colsum:
        assert nb1 == 1 and nb2 == 1
        ref.colsum = vf[0].sum(0)
        ref.colsum_bound = np.broadcast_to(ef, vf.shape)[0].sum(0) + M * u24 * np.abs(vf[0]).sum(0)
    if mutation == "store_past_n":
        ref.stray = int(off_rel[-1, -1, -1] + c_offset + 1)      # one element past the last column of the last row
    return ref


def finish_ref(slabs, c_dtype, M, N, *, bias=None, act=0, c2_dtype=None, R=None, rmode=0, ract=0, ldc=None, c_rpb=FLAT, c_rbstride=0,
               c_offset=0, bias_offset=0, drop_p=0.0, drop_seed=0, mutation=None):
    """scl_gemm_splitk_finish over given f32 slabs [nslabs, M, N] (CPU tensor): C = epilogue(sum of the slabs), alpha already applied."""
    ldc = N if ldc is None else ldc
    s = slabs.double().numpy()
    S = s.sum(0)[None]
    e = s.shape[0] * U23 * np.abs(s).sum(0)[None]
    off_rel = output_offsets(M, N, 1, 1, ldc, c_rpb, c_rbstride, 0, 0)
    bias_zn = None if bias is None else bias.reshape(-1).double().numpy()[bias_offset: bias_offset + N][None, None, :]
    c, cb, c2, c2b, _, _ = epilogue(S, e, off_rel, c_offset, N, c_dtype=c_dtype, c2_dtype=c2_dtype, bias_zn=bias_zn, act=act, R=R,
                                    rmode=rmode, ract=ract, alpha=1.0, drop_p=drop_p, drop_seed=drop_seed, mutation=mutation,
                                    bias_zn_wrong=bias_zn)
    ref = Ref(off=(off_rel + c_offset).reshape(-1), c=c.reshape(-1), c_bound=np.broadcast_to(cb, c.shape).reshape(-1), N=N,
              c_dtype=c_dtype, c2_dtype=c2_dtype)
    if c2 is not None:
        ref.c2, ref.c2_bound = c2.reshape(-1), np.broadcast_to(c2b, c2.shape).reshape(-1)
    if mutation == "store_past_n":
        ref.stray = int(off_rel[-1, -1, -1] + c_offset + 1)
    return ref


# ---- sentinel buffers and the checker -----------------------------------------------------------------------------------------------
SENTINEL_BITS = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5}      # quiet NaNs that no arithmetic produces
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def sentinel_buffer(numel, dtype, device="cpu"):
    """A buffer filled with one fixed (quiet NaN) bit pattern."""
    return torch.full((numel,), SENTINEL_BITS[dtype], dtype=_INT[dtype], device=device).view(dtype)


class CheckFailed(AssertionError):
    pass


def check_output(buf, off, val, bound, nslab=1, split_stride=0, what="C"):
    """buf: the CPU tensor a launch wrote into a sentinel_buffer.  Every element at off (+ s * split_stride) must hold a finite value
    with |sum_s got - val| <= bound, every other element must still hold the sentinel's bits.  Returns the worst |err| / bound."""
    flat = buf.reshape(-1)
    bits = flat.view(_INT[flat.dtype]).numpy()
    written = np.zeros(flat.numel(), dtype=bool)
    got = np.zeros(off.shape, dtype=np.float64)
    vals = flat.double().numpy()
    for s in range(nslab):
        o = off + s * split_stride
        written[o] = True
        got = got + vals[o]
    stray = np.flatnonzero(~written & (bits != SENTINEL_BITS[flat.dtype]))
    if stray.size:
        raise CheckFailed("%s: %d elements outside the addressed set were written, first at offset %d" % (what, stray.size, stray[0]))
    if not np.isfinite(got).all():
        bad = np.flatnonzero(~np.isfinite(got))
        raise CheckFailed("%s: %d addressed elements are not finite (unwritten or NaN), first at offset %d" % (what, bad.size, off[bad[0]]))
    err = np.abs(got - val)
    ratio = err / np.maximum(bound, 1e-300)
    worst = int(np.argmax(ratio))
    if ratio[worst] > 1.0:
        raise CheckFailed("%s: %d of %d elements beyond their bound; worst at offset %d: got %.9g, ref %.9g, |err| %.3e, bound %.3e" %
                          (what, int((ratio > 1.0).sum()), ratio.size, off[worst], got[worst], val[worst], err[worst], bound[worst]))
    return float(ratio[worst])


def check_colsum(part, ref):
    """part: CPU tensor [rows, N] of partial rows; their fp64 sum against the reference's column sums."""
    got = part.double().numpy().sum(0)
    if not np.isfinite(got).all():
        raise CheckFailed("colsum: a partial row holds a non-finite value")
    ratio = np.abs(got - ref.colsum) / np.maximum(ref.colsum_bound, 1e-300)
    if ratio.max() > 1.0:
        j = int(np.argmax(ratio))
        raise CheckFailed("colsum: column %d: got %.9g, ref %.9g, bound %.3e" % (j, got[j], ref.colsum[j], ref.colsum_bound[j]))
    return float(ratio.max())
