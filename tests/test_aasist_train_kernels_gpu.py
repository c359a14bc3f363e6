"""The column-masked train-mode BatchNorm kernels (scl_bn_fwd_cols / scl_bn_bwd_cols) and their autograd wrappers (hipnn.batch_norm_cols_train,
hipnn.zero_cols) on the GPU, against the float64 reference of tests/aasist_train_cases.py (pinned by tests/test_aasist_varlen_train_cpu.py).

Bounds: those of tests/test_resnet_varlen_train_gpu.py::test_masked_bn_train_forward_backward for the row form - max |got - ref| / max |ref|
per tensor < 2e-5, running statistics 1e-5 absolute; every figure is printed (`nn-err <kind> <case> <value>`) before it is asserted.
x, dy and y hold NaN at and beyond the widths; outputs and dx must be exactly +0.0 there, and two runs (and a run with zeros in place of the
NaN) must give the same bits.

The node side of the same training mode: scl_gat_score_bwd_var (the backward of the var pair scores) per utterance against the float64 torch
formulation on the utterance alone, parameter gradients against the float64 sum over the utterances; scl_gat_softmax_agg_var_bwd against the
float64 closed form of softmax(s / temp) @ x per utterance.  Bar: 1e-4 of the tensor's maximum, and where one misses it 4 x what the fp32
torch formulation loses against float64 on the same inputs, measured in the test and printed (the rule of tests/test_gat_long_gpu.py).
Rows beyond an utterance's nodes are exact zeros, NaN beyond the own graph changes no bit, `part` rows of blocks beyond N_b are zeros, two
runs give the same bits, and an utterance's dx / ds carry the bits of the run on it alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import aasist_train_cases as AC  # noqa: E402
from tests import nn_cases as NC  # noqa: E402

TOL, TOL_STATS = 2e-5, 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    from scl_amd import lib
    lib.load()
    return torch.device("cuda:0")


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _close(got, ref, kind, name, tol=TOL, failed=None, absolute=False):
    err = NC.maxabs(got, ref) if absolute else NC.maxrel(got, ref)
    print("nn-err %s %s %.3e" % (kind, name, err))
    if not err < tol:
        failed.append((kind, name, err))


def _plus_zero(t, keep):
    """Exact +0.0 (no sign bit) wherever keep is False."""
    pad = t.cpu()[~keep]
    return bool((pad == 0).all()) and not bool(torch.signbit(pad).any())


def _run_cols_bn(dev, inp, B, H, W, C, widths, act):
    """One forward, one plain backward and one accumulating backward through ops -> dict of device tensors."""
    from scl_amd import ops
    up = lambda t: None if t is None else t.to(dev)          # noqa: E731
    x, gamma, beta, dy = up(inp.x), up(inp.gamma), up(inp.beta), up(inp.dy)
    rm, rv, nbt = up(inp.running_mean), up(inp.running_var), up(inp.nbt)
    v = i32(widths, dev)
    keep = AC.keep_map(widths, H, W)
    nan = lambda *s, **kw: torch.full(s, NAN, device=dev, **kw)          # noqa: E731
    nslab = ops.bn_masked_nslabs(B, H, W)
    part, mean, rstd, y = nan(nslab * 2 * C, dtype=torch.float64), nan(C), nan(C), nan(B, H, W, C)
    ops.bn_fwd_cols(x, B, H, W, C, gamma, beta, rm, rv, nbt, NC.BN_MOMENTUM, NC.BN_EPS, act, v, widths, part, mean, rstd, y)
    y_in = y.clone()
    y_in[~keep.to(dev)] = NAN          # the backward must not read y at or beyond the widths either

    def backward(dg, db, accumulate):
        sums, dx = nan(2 * C + 1), nan(B, H, W, C)
        ops.bn_bwd_cols(dy, y_in, x, mean, rstd, gamma, B, H, W, C, act, v, widths, torch.full_like(part, NAN), sums, dg, db, dx, accumulate=accumulate)
        return sums, dx

    dg, db = nan(C), nan(C)
    sums, dx = backward(dg, db, False)
    ag, ab = up(inp.prior_dgamma).clone(), up(inp.prior_dbeta).clone()
    sums2, dx2 = backward(ag, ab, True)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, nbt=nbt, dx=dx, sums=sums, dg=dg, db=db, ag=ag, ab=ab, sums2=sums2, dx2=dx2)


@pytest.mark.parametrize("act", AC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
@pytest.mark.parametrize("case", AC.COLS_BN_CASES, ids=AC.case_id)
def test_cols_bn_train_forward_backward(dev, case, act):
    B, H, W, C, widths = case
    inp = AC.cols_bn_inputs(B, H, W, C, widths, act)          # NaN at and beyond the widths of x and dy
    ref = AC.cols_bn_reference(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, widths, NC.BN_MOMENTUM, NC.BN_EPS, act, inp.dy)
    got = _run_cols_bn(dev, inp, B, H, W, C, widths, act)
    keep = AC.keep_map(widths, H, W)
    tag = "%s-%s" % (AC.case_id(case), NC.ACT_NAMES[act])
    failed = []
    _close(got["y"], ref.y, "cbn_y", tag, failed=failed)
    _close(got["mean"], ref.mean, "cbn_mean", tag, failed=failed)
    _close(got["rstd"], ref.rstd, "cbn_rstd", tag, failed=failed)
    _close(got["rm"], ref.running_mean, "cbn_running_mean", tag, TOL_STATS, failed, absolute=True)
    _close(got["rv"], ref.running_var, "cbn_running_var", tag, TOL_STATS, failed, absolute=True)
    _close(got["dx"], ref.dx, "cbn_dx", tag, failed=failed)
    _close(got["sums"][:2 * C].view(2, C), ref.sums, "cbn_sums", tag, failed=failed)
    _close(got["dg"], ref.dgamma, "cbn_dgamma", tag, failed=failed)
    _close(got["db"], ref.dbeta, "cbn_dbeta", tag, failed=failed)
    _close(got["ag"], ref.dgamma + inp.prior_dgamma.double(), "cbn_dgamma", tag + "-acc", failed=failed)
    _close(got["ab"], ref.dbeta + inp.prior_dbeta.double(), "cbn_dbeta", tag + "-acc", failed=failed)
    assert not failed, failed
    assert got["nbt"].item() == inp.nbt.item() + 1
    assert abs(got["sums"][2 * C].item() * ref.n_valid - 1) < 1e-6          # N_v = H * sum(widths), counted on the device
    assert torch.isfinite(got["y"]).all() and torch.isfinite(got["dx"]).all()
    assert _plus_zero(got["y"], keep) and _plus_zero(got["dx"], keep)
    assert torch.equal(got["dx2"], got["dx"]) and torch.equal(got["sums2"], got["sums"])          # the accumulate form changes dgamma / dbeta only
    again = _run_cols_bn(dev, inp, B, H, W, C, widths, act)
    zeros = _run_cols_bn(dev, AC.cols_bn_inputs(B, H, W, C, widths, act, fill=0.0), B, H, W, C, widths, act)
    for k, t in got.items():
        assert torch.equal(t, again[k]), ("two runs", k)
        assert torch.equal(t, zeros[k]), ("zero padding", k)


def test_cols_bn_refuses_a_batch_without_a_valid_position(dev):
    from scl_amd import ops
    from scl_amd.lib import SclError
    B, H, W, C = 2, 3, 4, 16
    z = lambda *s, **kw: torch.zeros(*s, device=dev, **kw)          # noqa: E731
    part = z(ops.bn_masked_nslabs(B, H, W) * 2 * C, dtype=torch.float64)
    with pytest.raises(SclError, match="no valid position"):
        ops.bn_fwd_cols(z(B, H, W, C), B, H, W, C, None, None, None, None, None, 0.1, 1e-5, 2, i32([0, 0], dev), [0, 0], part, z(C), z(C), z(B, H, W, C))
    with pytest.raises(SclError, match="no valid position"):
        ops.bn_bwd_cols(z(B, H, W, C), z(B, H, W, C), z(B, H, W, C), z(C), z(C), None, B, H, W, C, 2, i32([0, 0], dev), [0, 0], part, z(2 * C + 1),
                        None, None, z(B, H, W, C))


def test_batch_norm_cols_train_and_zero_cols_under_autograd(dev):
    """hipnn.batch_norm_cols_train followed by hipnn.zero_cols of a product with a NaN-padded factor: the chain a residual block's output
    takes.  Gradients, outputs and buffers against the float64 reference; the NaN reaches nothing."""
    from scl_amd import hipnn
    B, H, W, C, widths = AC.COLS_BN_CASES[1]
    act = NC.ACT_SELU
    inp = AC.cols_bn_inputs(B, H, W, C, widths, act)
    ref = AC.cols_bn_reference(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, widths, NC.BN_MOMENTUM, NC.BN_EPS, act, inp.dy)
    keep = AC.keep_map(widths, H, W)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(inp.gamma); bn.bias.copy_(inp.beta); bn.running_mean.copy_(inp.running_mean); bn.running_var.copy_(inp.running_var)
        bn.num_batches_tracked.copy_(inp.nbt[0])
    x = inp.x.to(dev).requires_grad_(True)
    v = i32(widths, dev)
    y = hipnn.batch_norm_cols_train(x, bn, act, v, counts=widths)
    junk = torch.where(keep.to(dev)[..., None], torch.ones((), device=dev), torch.full((), NAN, device=dev)).expand(B, H, W, C)
    out = hipnn.zero_cols(y + junk, v)          # NaN at and beyond the widths before zero_cols, exact zeros behind it
    dy = inp.dy.to(dev)                         # NaN at and beyond the widths: zero_cols' backward selects it away
    out.backward(dy)
    torch.cuda.synchronize()
    failed = []
    _close(out, ref.y + keep[..., None].double(), "fn_out", "cols", failed=failed)
    _close(x.grad, ref.dx, "fn_dx", "cols", failed=failed)
    _close(bn.weight.grad, ref.dgamma, "fn_dgamma", "cols", failed=failed)
    _close(bn.bias.grad, ref.dbeta, "fn_dbeta", "cols", failed=failed)
    _close(bn.running_mean, ref.running_mean, "fn_running_mean", "cols", TOL_STATS, failed, absolute=True)
    _close(bn.running_var, ref.running_var, "fn_running_var", "cols", TOL_STATS, failed, absolute=True)
    assert not failed, failed
    assert bn.num_batches_tracked.item() == inp.nbt.item() + 1
    assert _plus_zero(out.detach(), keep) and _plus_zero(x.grad, keep)


# ---- scl_gat_score_bwd_var ----------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def _ragged(mats, Nmax, fill, dev, inner=1):
    """Per-utterance [N_b, N_b(, inner)] matrices -> [B, Nmax * Nmax * inner]: each at the start of its block (row stride N_b), `fill` behind."""
    out = torch.full((len(mats), Nmax * Nmax * inner), fill, device=dev)
    for b, m in enumerate(mats):
        out[b, : m.numel()] = m.reshape(-1)
    return out


def _score_inputs(dev, nodes, D, Do, na):
    g = torch.Generator().manual_seed(sum(nodes) * 7 + Do + na)
    xs = [torch.randn(n, D, generator=g).to(dev) for n in nodes]
    W = (torch.randn(Do, D, generator=g) / D ** 0.5).to(dev)
    bias = (0.1 * torch.randn(Do, generator=g)).to(dev)
    a = torch.randn(na, Do, generator=g).to(dev)
    gs = [torch.randn(n, n, generator=g).to(dev) for n in nodes]
    return xs, W, bias, a, gs


def _score_ref(xs, W, bias, a, gs, n1s, dtype):
    """Per utterance alone through the torch formulation -> ([dx_b], dW, dbias, da summed over the utterances)."""
    Wr, br, ar = (t.detach().to(dtype).requires_grad_(True) for t in (W, bias, a))
    dxs = []
    for x, g, n1 in zip(xs, gs, n1s):
        xr = x.detach().to(dtype).requires_grad_(True)
        AC.ref_score(xr, Wr, br, ar, n1).backward(g.to(dtype))
        dxs.append(xr.grad)
    return dxs, Wr.grad, br.grad, ar.grad


def _run_score_bwd_var(dev, xs, W, bias, a, gs, nodes, n1s, fill):
    from scl_amd import ops
    B, Nmax, D, Do = len(nodes), max(nodes), xs[0].shape[1], W.shape[0]
    x = torch.full((B, Nmax, D), fill, device=dev)
    for b, t in enumerate(xs):
        x[b, : t.shape[0]] = t
    ds = _ragged(gs, Nmax, fill, dev)
    a3 = torch.zeros(3, Do, device=dev)
    a3[: a.shape[0]] = a
    nb, ncol = ops.gat_score_nblocks(Nmax), Do * D + 4 * Do
    nan = lambda *s: torch.full(s, NAN, device=dev)          # noqa: E731
    dP, part, dx = nan(B * Nmax * Nmax * D), nan(B * nb, ncol), nan(B, Nmax, D)
    ops.gat_score_bwd_var(x, W, bias, a3, ds, dP, part, dx, i32(nodes, dev), None if n1s is None else i32(n1s, dev), B, Nmax, D, Do)
    red = torch.empty(ncol, device=dev)
    ops.colreduce(part, red, B * nb, ncol)
    torch.cuda.synchronize()
    return dict(dx=dx, part=part.view(B, nb, ncol), dW=red[: Do * D].view(Do, D), dbias=red[Do * D: Do * D + Do],
                da=red[Do * D + Do:].view(3, Do)[: a.shape[0]])


@pytest.mark.parametrize("hetero", (False, True), ids=("homogeneous", "heterogeneous"))
@pytest.mark.parametrize("D,Do", AC.GAT_WIDTHS)
@pytest.mark.parametrize("nodes,n1", ((AC.NODES_TILED, AC.N1_TILED), (AC.NODES_WHOLE, AC.N1_WHOLE)), ids=("tiled", "whole"))
def test_gat_score_bwd_var(dev, nodes, n1, D, Do, hetero):
    na = 3 if hetero else 1
    n1s = n1 if hetero else None
    xs, W, bias, a, gs = _score_inputs(dev, nodes, D, Do, na)
    n1_ref = n1 if hetero else nodes
    dx64, *p64 = _score_ref(xs, W, bias, a, gs, n1_ref, torch.float64)
    got = _run_score_bwd_var(dev, xs, W, bias, a, gs, nodes, n1s, NAN)          # NaN in x and ds beyond the own graph
    Nmax, tag = max(nodes), ("score_bwd_var", "tiled" if max(nodes) > 128 else "whole", D, Do, na)
    errs = {"dx%d" % b: _rel(got["dx"][b, :n], dx64[b]) for b, n in enumerate(nodes)}
    errs.update(dW=_rel(got["dW"], p64[0]), dbias=_rel(got["dbias"], p64[1]), da=_rel(got["da"], p64[2]))
    print(tag, {k: "%.2e" % v for k, v in errs.items()})
    e32 = None
    for k, e in errs.items():
        if e < AC.GRAD_BAR:
            continue
        if e32 is None:      # what the fp32 torch formulation loses against float64 on the same inputs
            dx32, *p32 = _score_ref(xs, W, bias, a, gs, n1_ref, torch.float32)
            e32 = {"dx%d" % b: _rel(dx32[b], dx64[b]) for b in range(len(nodes))}
            e32.update(dW=_rel(p32[0], p64[0]), dbias=_rel(p32[1], p64[1]), da=_rel(p32[2], p64[2]))
            print(tag, "fp32 torch vs float64:", {k_: "%.2e" % v for k_, v in e32.items()})
        assert e <= 4 * e32[k], (k, e, e32[k])
    assert torch.isfinite(got["dx"]).all() and torch.isfinite(got["part"]).all()
    from scl_amd import ops
    nb = ops.gat_score_nblocks(Nmax)
    for b, n in enumerate(nodes):
        pad = got["dx"][b, n:]
        assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), ("dx rows beyond", b)
        ipb = 8 if Nmax > 128 else (n + nb - 1) // nb
        first_beyond = (n + ipb - 1) // ipb          # the first block whose rows start at or beyond N_b
        assert bool((got["part"][b, first_beyond:] == 0).all()), ("part rows beyond", b)
    # two runs, and zeros in place of the NaN beyond the own graph: the same bits
    again = _run_score_bwd_var(dev, xs, W, bias, a, gs, nodes, n1s, NAN)
    zeros = _run_score_bwd_var(dev, xs, W, bias, a, gs, nodes, n1s, 0.0)
    for k, t in got.items():
        assert torch.equal(t, again[k]), ("two runs", k)
        assert torch.equal(t, zeros[k]), ("zero padding", k)
    # an utterance alone, where that run takes the same kernel form: dx bit for bit
    for b, n in enumerate(nodes):
        if (n > 128) != (Nmax > 128):
            continue
        alone = _run_score_bwd_var(dev, xs[b:b + 1], W, bias, a, gs[b:b + 1], [n], None if n1s is None else [n1s[b]], NAN)
        assert torch.equal(alone["dx"][0], got["dx"][b, :n]), ("alone", b)


def test_gat_score_var_under_autograd(dev):
    """gat.gat_score_var followed by gat.gat_softmax_agg_var: the chain of a heterogeneous layer, differentiated, against float64 per utterance."""
    from scl_amd import gat
    nodes, n1, D, Do, temp = [151, 106, 28], [130, 85, 7], 64, 32, 100.0
    xs, W, bias, a, _ = _score_inputs(dev, nodes, D, Do, 3)
    g = torch.Generator().manual_seed(5)
    douts = [torch.randn(n, D, generator=g).to(dev) for n in nodes]
    B, Nmax = len(nodes), max(nodes)
    x = torch.zeros(B, Nmax, D, device=dev)
    dout = torch.full((B, Nmax, D), NAN, device=dev)
    for b, n in enumerate(nodes):
        x[b, :n], dout[b, :n] = xs[b], douts[b]
    leaves = [t.clone().requires_grad_(True) for t in (x, W, bias, a)]
    nd = i32(nodes, dev)
    out = gat.gat_softmax_agg_var(gat.gat_score_var(*leaves, nd, i32(n1, dev)), leaves[0], nd, temp)
    out.backward(dout)
    Wr, br, ar = (t.double().requires_grad_(True) for t in (W, bias, a))
    failed = []
    for b, n in enumerate(nodes):
        xr = xs[b].double().requires_grad_(True)
        o = torch.softmax(AC.ref_score(xr, Wr, br, ar, n1[b]) / temp, -1) @ xr
        o.backward(douts[b].double())
        _close(out[b, :n], o.detach(), "chain_out", str(b), 1e-5, failed)
        _close(leaves[0].grad[b, :n], xr.grad, "chain_dx", str(b), AC.GRAD_BAR, failed)
        assert bool((leaves[0].grad[b, n:] == 0).all()) and bool((out[b, n:] == 0).all())
    _close(leaves[1].grad, Wr.grad, "chain_dW", "", AC.GRAD_BAR, failed)
    _close(leaves[2].grad, br.grad, "chain_dbias", "", AC.GRAD_BAR, failed)
    _close(leaves[3].grad, ar.grad, "chain_da", "", AC.GRAD_BAR, failed)
    assert not failed, failed


# ---- scl_gat_softmax_agg_var_bwd ----------------------------------------------------------------------------------------------------------
def _run_agg_bwd(dev, ss, xs, douts, nodes, temp, one_row, fill):
    from scl_amd import ops
    B, Nmax, D = len(nodes), max(nodes), xs[0].shape[1]
    x = torch.full((B, Nmax, D), fill, device=dev)
    for b, t in enumerate(xs):
        x[b, : t.shape[0]] = t
    if one_row:
        s, dout = torch.full((B, Nmax), fill, device=dev), torch.stack([d[0] for d in douts])
        for b, t in enumerate(ss):
            s[b, : t.shape[1]] = t[0]
    else:
        s, dout = _ragged(ss, Nmax, fill, dev), torch.full((B, Nmax, D), fill, device=dev)
        for b, t in enumerate(douts):
            dout[b, : t.shape[0]] = t
    ds, dx = torch.full_like(s, 7.0), torch.full((B, Nmax, D), NAN, device=dev)
    stats = torch.full((B * (1 if one_row else Nmax) * 2,), NAN, device=dev)
    ops.gat_softmax_agg_var_bwd(s.contiguous(), x, i32(nodes, dev), dout.contiguous(), ds, dx, stats, B, Nmax, D, temp, one_row)
    torch.cuda.synchronize()
    return ds, dx


@pytest.mark.parametrize("one_row", (False, True), ids=("matrix", "one_row"))
@pytest.mark.parametrize("temp", (2.0, 100.0))
@pytest.mark.parametrize("D", (32, 64))
@pytest.mark.parametrize("nodes", (AC.NODES_TILED, AC.NODES_WHOLE), ids=("tiled", "whole"))
def test_gat_softmax_agg_var_bwd(dev, nodes, D, temp, one_row):
    g = torch.Generator().manual_seed(sum(nodes) + D)
    rows = lambda n: 1 if one_row else n          # noqa: E731
    ss = [(3.0 * torch.randn(rows(n), n, generator=g)).to(dev) for n in nodes]
    xs = [torch.randn(n, D, generator=g).to(dev) for n in nodes]
    douts = [torch.randn(rows(n), D, generator=g).to(dev) for n in nodes]
    ds, dx = _run_agg_bwd(dev, ss, xs, douts, nodes, temp, one_row, NAN)
    tag = ("agg_bwd", "tiled" if max(nodes) > 128 else "whole", D, temp, "one_row" if one_row else "matrix")
    for b, n in enumerate(nodes):
        _, ds64, dx64 = AC.agg_reference(ss[b], xs[b], douts[b], temp)
        got_ds, got_dx = ds[b, : rows(n) * n].view(rows(n), n), dx[b, :n]
        e_ds, e_dx = _rel(got_ds, ds64), _rel(got_dx, dx64)
        line = "%s b=%d ds %.2e dx %.2e" % (tag, b, e_ds, e_dx)
        if not (e_ds < AC.GRAD_BAR and e_dx < AC.GRAD_BAR):      # what the fp32 torch chain loses against float64 on the same inputs
            s32, x32 = ss[b].clone().requires_grad_(True), xs[b].clone().requires_grad_(True)
            (torch.softmax(s32 / temp, -1) @ x32).backward(douts[b])
            t_ds, t_dx = _rel(s32.grad, ds64), _rel(x32.grad, dx64)
            print(line, "fp32 torch: ds %.2e dx %.2e" % (t_ds, t_dx))
            assert e_ds < max(AC.GRAD_BAR, 4 * t_ds) and e_dx < max(AC.GRAD_BAR, 4 * t_dx), (b, e_ds, t_ds, e_dx, t_dx)
        else:
            print(line)
        pad = dx[b, n:]
        assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), ("dx rows beyond", b)
        assert bool((ds[b, rows(n) * n:] == 7.0).all()), ("ds beyond the own matrix is not written", b)
        # the utterance alone: the same bits
        ds1, dx1 = _run_agg_bwd(dev, ss[b:b + 1], xs[b:b + 1], douts[b:b + 1], [n], temp, one_row, NAN)
        assert torch.equal(ds1[0, : rows(n) * n], ds[b, : rows(n) * n]) and torch.equal(dx1[0], dx[b, :n]), ("alone", b)
    assert torch.isfinite(dx).all() and torch.isfinite(ds).all()
    ds0, dx0 = _run_agg_bwd(dev, ss, xs, douts, nodes, temp, one_row, 0.0)
    ds2, dx2 = _run_agg_bwd(dev, ss, xs, douts, nodes, temp, one_row, NAN)
    assert torch.equal(ds, ds0) and torch.equal(dx, dx0), "zero padding"
    assert torch.equal(ds, ds2) and torch.equal(dx, dx2), "two runs"
