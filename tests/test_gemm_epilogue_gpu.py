"""Every GEMM epilogue implementation, on its vector and its element-wise store path, against the fp64 descriptor reference of
tests/gemm_ref.py: |got - ref| <= the derived per-element bound on EVERY addressed element of C and C2 (and the column sums), and
every byte of the output buffers outside the addressed set still the sentinel's.  The cases (tests/gemm_epilogue_cases.py) are the
ones tests/test_gemm_ref_cpu.py proves sharp on the CPU: each mutation of an epilogue step that applies to a case's flags is rejected
at that case's inputs.

Implementations: the 128 x 128 tiles register-staged (no_dma) and through LDS-DMA (no_w8): kinds 1-5 of gemm_epilogue_blk and its
generic form by flag set; the wide tiles (force_w8): kinds 1-4 of w8_epilogue_pass and its generic loop (which also serves the flag
set of kind 5: the wide kernel compiles that kind out), every flag set on the 112-row and on the 208-row tiling, four on the 256-row
tiling, the tiling asserted through ops.gemm_wide_kind; scl_gemm_splitk_finish over hand-made slabs; the exact-f32 kernel and both
bf16-pair forms (split at staging: K-contiguous operands; per fragment: a transposed operand) on 64 x 64 and on 128 x 128 tiles; the
experiment kernels where the library was built with them.  What the library cannot be asked at run time — LDS-DMA or register
staging on the 128 x 128 tiles, the f32 kernels' tile — follows from the dispatch conditions, which tests/test_gemm_ref_cpu.py
asserts of the table's shapes.

SCL_GEMM_EPILOGUE_RECORD=<file>: the worst |err| / bound per implementation x path x flag set is written there (profiles/gemm_epilogue_ref.txt
is such a run: the measured margin under the bounds, not a bar)."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import ops  # noqa: E402
from tests import gemm_epilogue_cases as GC  # noqa: E402
from tests import gemm_ref as GR  # noqa: E402

SPECS = GC.all_specs()
RECORD = {}


def _has_experiments():
    return bool(ops.L.load().scl_build_flags() & 1)


needs_experiments = pytest.mark.skipif("not _has_experiments()", reason="library built without -DSCL_EXPERIMENTS")


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("SCL_GEMM_EPILOGUE_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# worst |err| / bound per case and output (C, C2, column sums; the element type beside it); kind = ops.gemm_wide_kind;\n")
        f.write("# x3_dist = max |formula - exact| / max |exact| of the accumulator\n")
        f.write("%-12s %-11s %-18s %4s %13s %13s %8s %10s\n" % ("impl", "path", "flag set", "kind", "C", "C2", "colsum", "x3_dist"))
        fmt = lambda r: "-" if r is None else ("%.4f" % r if not isinstance(r, tuple) else "%.4f %s" % r)
        for (impl, path_, fs), (rc, rc2, rcs, kind, x3d) in RECORD.items():
            f.write("%-12s %-11s %-18s %4s %13s %13s %8s %10s\n" % (impl, path_, fs, kind, fmt(rc), fmt(rc2), fmt(rcs), "-" if x3d is None else "%.3e" % x3d))
        for dt in ("f32", "bf16"):
            rs = [r[0] for v in RECORD.values() for r in v[:2] if r is not None and r[1] == dt]
            f.write("# max over %d %s outputs: %.4f\n" % (len(rs), dt, max(rs)))


def _dev_op(h, dev):
    return ops.Op(h.t.to(dev), h.ld, **h.kw())


def _run(spec, dev):
    b = GC.build(spec)
    s = b.spec
    C = GR.sentinel_buffer(b.cnumel, b.c_dtype, dev)
    C2 = GR.sentinel_buffer(b.cnumel, b.c2_dtype, dev) if b.c2_dtype is not None else None
    R = b.R.to(dev) if b.R is not None else None
    bias = b.bias.to(dev) if b.bias is not None else None
    kw = dict(b.kw)
    part, kind = None, "-"
    if b.slabs is not None:
        slabs = b.slabs.to(dev)
        dummy = torch.zeros(64, dtype=torch.bfloat16, device=dev)
        fk = {k: kw[k] for k in ("act", "rmode", "ract", "ldc", "c_offset", "drop_p", "drop_seed")}
        dsc = ops._gemm_desc(ops.Op(dummy, 8), ops.Op(dummy, 8), C, b.M, b.N, 8, c2=C2, R=R, bias=bias, **fk)
        ops._call("scl_gemm_splitk_finish", ctypes.byref(dsc), ops._ptr(slabs), slabs.shape[0], b.M * b.N, ops._stream(), keep=dsc)
    else:
        A, B = _dev_op(b.A, dev), _dev_op(b.B, dev)
        kw.update(s["sel"])
        kw.update(c2=C2, R=R, bias=bias)
        if s["colsum"]:
            rows = ops.gemm_colsum_rows(A, B, C, b.M, b.N, b.K, **kw)
            assert rows > 0
            part = torch.full((rows, b.N), float("nan"), device=dev)
            kw.update(colsum_part=part)
        if b.A.t.dtype == torch.bfloat16:
            kind = ops.gemm_wide_kind(A, B, C, b.M, b.N, b.K, **kw)
            assert kind == s["kind"], "kernel selection: wide kind %d, the case was written for %d" % (kind, s["kind"])
        ops.gemm(A, B, C, b.M, b.N, b.K, **kw)
    got_c = C.cpu()
    ref = GC.reference(b)
    rc = GR.check_output(got_c, ref.off, ref.c, ref.c_bound, ref.nslab, ref.split_stride, s["name"] + " C")
    rc2 = GR.check_output(C2.cpu(), ref.off, ref.c2, ref.c2_bound, what=s["name"] + " C2") if C2 is not None else None
    rcs = GR.check_colsum(part.cpu(), ref) if part is not None else None
    worst = max(r for r in (rc, rc2, rcs) if r is not None)
    RECORD[(s["impl"], s["path"], s["flagset"])] = ((rc, s["c"]), None if rc2 is None else (rc2, s["c2"]), rcs, kind, ref.x3_dist)
    print("%s: worst |err| / bound %.4f%s" % (s["name"], worst, "" if ref.x3_dist is None else ", x3 formula to exact %.3e" % ref.x3_dist))
    return worst


@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
def test_epilogue_against_fp64_descriptor_reference(dev, spec):
    assert _run(spec, dev) <= 1.0


@needs_experiments
@pytest.mark.parametrize("sel", ["force_big", "force_p8", "force_x2"])
@pytest.mark.parametrize("path", ["aligned", "padded_odd", "misaligned"])
@pytest.mark.parametrize("flagset", ["fc1_fwd", "resid_f32", "head_bwd_leaky", "gelu_grad_alpha"])
def test_experiment_kernels_against_fp64_descriptor_reference(dev, sel, path, flagset):
    """The opt-in kernels (256 x 128 ring, 256 x 256 ping-pong, two blocks per CU) share gemm_epilogue_blk / w8_epilogue_pass."""
    i = list(GC.FLAGSETS).index(flagset)
    spec = GC._spec("t128_dma", path, flagset, i, as_impl=sel, M=264, K=192, a_t=False, b_t=False, sel={sel: True},
                    kind=3 if sel == "force_x2" else 0)
    assert _run(spec, dev) <= 1.0
