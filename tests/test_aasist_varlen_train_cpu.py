"""The kernels of AASIST training on zero-padded batches - the column-masked train-mode BatchNorm (scl_bn_fwd_cols / scl_bn_bwd_cols,
hipnn.batch_norm_cols_train, hipnn.zero_cols), scl_gat_score_bwd_var and scl_gat_softmax_agg_var_bwd - without a GPU:
(d) the float64 references of tests/aasist_train_cases.py are torch autograd on the compact tensors; (e) the new entry
points refuse NULL and bad arguments before they touch a device pointer, and the Python wrappers refuse the modes that belong to the
scoring forms - whose own refusals stay what they were.
Further down, the float64 DEFINITION of the train-mode back-end on a zero-padded batch (tests/aasist_train_cases.py::masked_train_forward):
(a) equal frames on a padded batch and (c) B = 1 equal the oracle head in train mode on the compact batch - outputs, every gradient, every
buffer; (b) on ragged batches every masked BatchNorm's recorded statistics are torch's on the concatenation of the valid positions, whose
count is the count table's, and NaN padding changes no bit; (f) the GPU head tests' seeds keep every GraphPool top-k margin above 1e-5;
(e) main.py's opt-in routing: one switch without the other exits naming both, VARLEN_MODELS stays the tuple it is."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from scl_amd import hipnn, lib
from tests import aasist_train_cases as AC
from tests import nn_cases as NC


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("act", AC.ACTS, ids=lambda a: NC.ACT_NAMES[a])
@pytest.mark.parametrize("case", AC.COLS_BN_CASES, ids=AC.case_id)
def test_cols_batch_norm_reference_is_torch_autograd_on_the_compact_tensor(case, act):
    B, H, W, C, widths = case
    inp = AC.cols_bn_inputs(B, H, W, C, widths, act)          # NaN at and beyond the widths of x and dy
    ref = AC.cols_bn_reference(inp.x, inp.gamma, inp.beta, inp.running_mean, inp.running_var, widths, NC.BN_MOMENTUM, NC.BN_EPS, act, inp.dy)
    c = inp.compact
    x = c.x.double().requires_grad_(True)
    gm, bt = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    rm, rv = c.running_mean.double().clone(), c.running_var.double().clone()
    z = F.batch_norm(x, rm, rv, gm, bt, True, NC.BN_MOMENTUM, NC.BN_EPS)
    y = (z, torch.relu(z), torch.selu(z))[act]
    y.backward(c.dy.double())
    keep = AC.keep_map(widths, H, W)
    assert ref.n_valid == x.shape[0] == H * sum(widths)
    # boolean indexing walks (b, h, w) in order: the order cols_bn_inputs scattered the compact rows in
    worst = max(_rel(ref.y[keep].reshape(-1, C), y.detach()), _rel(ref.dx[keep].reshape(-1, C), x.grad), _rel(ref.dgamma, gm.grad),
                _rel(ref.dbeta, bt.grad), _rel(ref.running_mean, rm), _rel(ref.running_var, rv))
    print("column-masked BatchNorm reference against torch autograd: %.2e" % worst)
    assert worst < 1e-12
    assert (ref.y[~keep] == 0).all() and (ref.dx[~keep] == 0).all() and torch.isfinite(ref.y).all() and torch.isfinite(ref.dx).all()
    full = NC.bn_reference(c.x, c.gamma, c.beta, c.running_mean, c.running_var, True, NC.BN_MOMENTUM, NC.BN_EPS, act, c.dy)
    assert _rel(ref.sums, full.sums) < 1e-12 and _rel(ref.rstd, full.rstd) < 1e-12


def test_new_entry_points_refuse_null_and_bad_arguments_without_touching_the_gpu():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    host = (ctypes.c_int32 * 2)(3, 1)
    none_valid = (ctypes.c_int32 * 2)(0, 0)
    shapes = (dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(C=0), dict(C=3), dict(C=1024), dict(act=3), dict(act=-1),
              dict(H=1 << 15, W=1 << 12))      # H * W * C = 2^31
    fwd_args = (("x", p), ("B", 2), ("H", 3), ("W", 4), ("C", 16), ("gamma", p), ("beta", p), ("rm", p), ("rv", p), ("nbt", p), ("momentum", 0.1),
                ("eps", 1e-5), ("act", 2), ("widths", p), ("widths_host", host), ("part", p), ("mean", p), ("rstd", p), ("y", p), ("stream", None))
    fwd = lambda **kw: L.scl_bn_fwd_cols(*[kw.get(k, d) for k, d in fwd_args])          # noqa: E731
    for kw in (dict(x=None), dict(widths=None), dict(widths_host=None), dict(part=None), dict(mean=None), dict(rstd=None), dict(y=None)) + shapes:
        assert fwd(**kw) == -1 and b"bn_fwd_cols" in L.scl_last_error(), kw
    assert fwd(x=odd) == -1 and b"16-byte" in L.scl_last_error()
    assert fwd(y=odd) == -1 and b"16-byte" in L.scl_last_error()
    assert fwd(widths_host=none_valid) == -1 and b"no valid position" in L.scl_last_error()

    bwd_args = (("dy", p), ("y", p), ("x", p), ("mean", p), ("rstd", p), ("gamma", p), ("B", 2), ("H", 3), ("W", 4), ("C", 16), ("act", 2),
                ("widths", p), ("widths_host", host), ("part", p), ("sums", p), ("dgamma", p), ("dbeta", p), ("dx", p), ("accumulate", 0),
                ("stream", None))
    bwd = lambda **kw: L.scl_bn_bwd_cols(*[kw.get(k, d) for k, d in bwd_args])          # noqa: E731
    for kw in (dict(dy=None), dict(x=None), dict(mean=None), dict(rstd=None), dict(widths=None), dict(widths_host=None), dict(part=None),
               dict(sums=None), dict(dx=None), dict(y=None)) + shapes:      # y: the activation gradient needs it (act = 2)
        assert bwd(**kw) == -1 and b"bn_bwd_cols" in L.scl_last_error(), kw
    assert bwd(dx=odd) == -1 and b"16-byte" in L.scl_last_error()
    assert bwd(widths_host=none_valid) == -1 and b"no valid position" in L.scl_last_error()


def test_the_wrappers_refuse_the_other_forms_modes_and_the_scoring_refusals_stay():
    x = torch.zeros(2, 3, 4, 16)
    widths = torch.tensor([4, 2], dtype=torch.int32)
    bn = torch.nn.BatchNorm2d(16)
    # the train form: train mode with autograd on, nothing else
    bn.eval()
    with pytest.raises(NotImplementedError, match="train mode with autograd on"):
        hipnn.batch_norm_cols_train(x, bn, hipnn.ACT_SELU, widths)
    bn.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="train mode with autograd on"):
        hipnn.batch_norm_cols_train(x, bn, hipnn.ACT_SELU, widths)
    with pytest.raises(NotImplementedError, match="train mode with autograd on"):
        hipnn.batch_norm_cols_train(x[0], bn, hipnn.ACT_SELU, widths)
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        hipnn.zero_cols(x[0], widths)
    # the scoring forms keep refusing train mode and autograd
    with pytest.raises(NotImplementedError, match="scoring mode"):
        hipnn.batch_norm_cols(x, bn, hipnn.ACT_SELU, widths)
    bn.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):
        hipnn.batch_norm_cols(x, bn, hipnn.ACT_SELU, widths)          # autograd on
    with pytest.raises(NotImplementedError, match="torch.no_grad"):
        hipnn.zero_cols_(x, widths)


@pytest.mark.parametrize("rows", (1, 9))
@pytest.mark.parametrize("temp", (2.0, 100.0))
def test_softmax_agg_reference_is_torch_autograd(rows, temp):
    g = torch.Generator().manual_seed(3)
    s = (3.0 * torch.randn(rows, 9, generator=g, dtype=torch.float64)).requires_grad_(True)
    x = torch.randn(9, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    dout = torch.randn(rows, 8, generator=g, dtype=torch.float64)
    out = torch.softmax(s / temp, -1) @ x
    out.backward(dout)
    ro, rds, rdx = AC.agg_reference(s.detach(), x.detach(), dout, temp)
    assert _rel(ro, out.detach()) < 1e-13 and _rel(rds, s.grad) < 1e-12 and _rel(rdx, x.grad) < 1e-13


def test_node_side_entry_points_refuse_null_and_bad_arguments_without_touching_the_gpu():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    sc_args = (("x", p), ("W", p), ("bias", p), ("a", p), ("ds", p), ("dP", p), ("part", p), ("dx", p), ("nodes", p), ("n1", p), ("B", 2),
               ("Nmax", 66), ("D", 64), ("Do", 32), ("stream", None))
    sc = lambda **kw: L.scl_gat_score_bwd_var(*[kw.get(k, d) for k, d in sc_args])          # noqa: E731
    for kw in (dict(x=None), dict(W=None), dict(bias=None), dict(a=None), dict(ds=None), dict(dP=None), dict(part=None), dict(dx=None),
               dict(nodes=None), dict(B=0), dict(B=65536), dict(Nmax=0), dict(Nmax=1025), dict(D=48), dict(D=32, Do=64), dict(Do=17),
               dict(Nmax=129, n1=None)):      # the tiled form reads both tables
        assert sc(**kw) == -1 and b"gat_score_bwd_var" in L.scl_last_error(), kw
    ag_args = (("s", p), ("x", p), ("nodes", p), ("dout", p), ("ds", p), ("dx", p), ("stats", p), ("B", 2), ("Nmax", 66), ("D", 64), ("one_row", 0),
               ("temp", 2.0), ("stream", None))
    ag = lambda **kw: L.scl_gat_softmax_agg_var_bwd(*[kw.get(k, d) for k, d in ag_args])          # noqa: E731
    for kw in (dict(s=None), dict(x=None), dict(nodes=None), dict(dout=None), dict(ds=None), dict(dx=None), dict(stats=None), dict(B=0),
               dict(B=65536), dict(Nmax=0), dict(Nmax=1025), dict(D=48), dict(temp=0.0), dict(temp=-1.0)):
        assert ag(**kw) == -1 and b"gat_softmax_agg_var_bwd" in L.scl_last_error(), kw


# ---- the definition of the train-mode back-end on a zero-padded batch (tests/aasist_train_cases.py::masked_train_forward) -------------------
def _train_mode(m):
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _definition_step(t, x, frames, T, fill, step):
    feats = torch.full((len(frames), T, 128), fill, dtype=torch.float64)
    for b, n in enumerate(frames):
        feats[b, :n] = x[b, :n]
    feats.requires_grad_(True)
    rec = {}
    out, hid = AC.masked_train_forward(t, feats, frames, rec)
    torch.autograd.backward([out, hid], list(AC.head_cotangents(step, len(frames))))
    return out.detach(), hid.detach(), feats.grad, rec


@pytest.mark.parametrize("case", sorted(AC.HEAD_EQUAL))
def test_equal_frames_on_a_padded_batch_equal_the_oracle_head_in_train_mode(case):
    """(a) and (c): outputs, d(feats), every parameter gradient and every buffer, two steps, float64; the padding holds NaN."""
    B, t0, T, seed = AC.HEAD_EQUAL[case]
    ref, t = AC.oracle_state(seed)
    _train_mode(ref)
    for step in range(2):
        x = AC.head_input(step, B, t0).double()
        xr = x.clone().requires_grad_(True)
        ro, rh = ref(xr)
        torch.autograd.backward([ro, rh], list(AC.head_cotangents(step, B)))
        out, hid, dx, rec = _definition_step(t, x, [t0] * B, T + 7, float("nan"), step)
        assert min(rec["margins"]) > AC.TOPK_MARGIN, min(rec["margins"])          # (f) for these cases
        worst = max(_rel(out, ro.detach()), _rel(hid, rh.detach()), _rel(dx[:, :t0], xr.grad))
        assert (dx[:, 3 * (t0 // 3):] == 0).all()
        # gradients on the scale of the step's largest one: some are analytically zero (attention.2.bias shifts a soft-max's scores), where
        # both sides hold rounding noise and a ratio of the two says nothing
        casemax = max(p.grad.abs().max().item() for _, p in ref.named_parameters() if p.grad is not None)
        for k, p in ref.named_parameters():
            if p.grad is None:
                assert t[k].grad is None or not t[k].grad.any(), k
            else:
                worst = max(worst, (t[k].grad - p.grad).abs().max().item() / casemax)
                p.grad, t[k].grad = None, None
        for k, v in ref.named_buffers():
            assert _rel(t[k].double(), v.double()) < 1e-12, k
        print("definition against the oracle, %s step %d: %.2e" % (case, step, worst))
        assert worst < 1e-9


@pytest.mark.parametrize("case", sorted(AC.HEAD_RAGGED))
def test_ragged_frames_statistics_run_over_the_valid_positions_and_padding_changes_nothing(case):
    """(b) and (f): every masked BatchNorm's recorded statistics are torch's on the concatenation of the valid positions, whose count is the
    count table's; NaN instead of zeros in the padding changes no bit, gradients included; the GPU tests' top-k margins hold in float64."""
    from scl_amd.aasist_head import node_counts
    frames, seed = AC.HEAD_RAGGED[case]
    c = node_counts(frames)
    B, T = len(frames), max(frames)
    runs = []
    for fill in (float("nan"), 0.0):
        _, t = AC.oracle_state(seed)
        per_step = []
        for step in range(2):
            out, hid, dx, rec = _definition_step(t, AC.head_input(step, B, T).double(), frames, T, fill, step)
            per_step.append((out, hid, dx, {k: v.grad.clone() for k, v in t.items() if v.grad is not None}, rec))
            for v in t.values():
                v.grad = None
        runs.append((per_step, {k: v.clone() for k, v in t.items() if not v.requires_grad}))
    (nan_steps, nan_buf), (zero_steps, zero_buf) = runs
    for k in nan_buf:
        assert torch.equal(nan_buf[k], zero_buf[k]), k
    stack, nodes = 42 * sum(c["W"]), {"GAT_layer_S.bn": 42 * B, "GAT_layer_T.bn": sum(c["W"]), "HtrgGAT_layer_ST11.bn": sum(c["N1"]),
                                      "HtrgGAT_layer_ST21.bn": sum(c["N1"]), "HtrgGAT_layer_ST12.bn": sum(c["N2"]), "HtrgGAT_layer_ST22.bn": sum(c["N2"])}
    for step, ((o1, h1, d1, g1, rec), (o2, h2, d2, g2, _)) in enumerate(zip(nan_steps, zero_steps)):
        assert torch.equal(o1, o2) and torch.equal(h1, h2) and torch.equal(d1, d2) and set(g1) == set(g2)
        assert all(torch.equal(g1[k], g2[k]) for k in g1) and torch.isfinite(d1).all() and all(torch.isfinite(g).all() for g in g1.values())
        for b, n in enumerate(frames):
            assert (d1[b, 3 * (n // 3):] == 0).all() and d1[b, :3 * (n // 3)].any()
        assert min(rec["margins"]) > AC.TOPK_MARGIN, (step, min(rec["margins"]))
        names = [k for k in rec if k != "margins"]
        assert len(names) == 1 + 5 + 6 + 2 + 6          # first_bn, five bn1, six bn2, first_bn1 + attention.2, six graph layers
        for k in names:
            mean, var, n, flat = rec[k]
            rv, rm = torch.var_mean(flat, 0, unbiased=False)
            scale = flat.abs().max().item()
            assert (mean - rm).abs().max().item() < 1e-12 * scale and (var - rv).abs().max().item() < 1e-12 * scale * scale, k
            # conv1 is 2 x 3 with padding (1, 1): its output, bn2's input, has 43 rows; conv2 (padding (0, 1)) brings the map back to 42
            want = 43 * sum(c["W"]) if k.endswith("bn2") else nodes.get(k, stack)
            assert n == flat.shape[0] == want, (k, n, want)
    assert all(int(nan_buf[k]) == 2 for k in nan_buf if k.endswith("num_batches_tracked"))


# ---- (e) main.py and the plugin behind their switches ------------------------------------------------------------------------------------------
def _train_args(tmp_path, monkeypatch):
    import yaml
    cfg = {"model": {"name": "wav2vec2_aasist", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "asvspoof_2019_augall_3", "kwargs": {}}}
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)      # the refusal comes before anything touches a device
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    return ["--config", str(tmp_path / "conf.yaml"), "--database_path", str(tmp_path), "--padding_type", "zero", "--batch_size", "2"]


@pytest.mark.parametrize("train,score", [("1", None), (None, "1"), (None, "long")])
def test_one_switch_without_the_other_makes_main_exit_naming_both(tmp_path, monkeypatch, train, score):
    import main as M
    for k, v in (("SCL_AASIST_TRAIN_LENGTHS", train), ("SCL_AASIST_LENGTHS", score)):
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        M.main(_train_args(tmp_path, monkeypatch))
    assert "SCL_AASIST_TRAIN_LENGTHS" in str(e.value) and "SCL_AASIST_LENGTHS" in str(e.value) and "wav2vec2_aasist" in str(e.value)


@pytest.mark.parametrize("both", (False, True))
def test_with_both_switches_or_neither_main_passes_its_start_up_checks(tmp_path, monkeypatch, both):
    import main as M

    class Reached(Exception):
        pass

    def build(*a, **k):
        raise Reached()
    for k in ("SCL_AASIST_TRAIN_LENGTHS", "SCL_AASIST_LENGTHS"):
        monkeypatch.setenv(k, "1") if both else monkeypatch.delenv(k, raising=False)
    monkeypatch.setitem(M.MODEL_REGISTRY, "wav2vec2_aasist", build)
    with pytest.raises(Reached):
        M.main(_train_args(tmp_path, monkeypatch))
    assert M._trains_varlen("wav2vec2_aasist") is both and M._trains_varlen("wav2vec2_resnet_nll") and not M._trains_varlen("wav2vec2_btse")
    assert M.VARLEN_MODELS == ("wav2vec2_linear_nll", "wav2vec2_resnet_nll") and "wav2vec2_aasist" not in M.VARLEN_MODELS
    assert M.VARLEN_TRAIN_OPT_IN == {"wav2vec2_aasist": "SCL_AASIST_TRAIN_LENGTHS"}


def test_the_plugin_declares_the_training_mode_only_behind_its_switch(monkeypatch):
    from scl_amd.model_aasist import Model
    m = Model.__new__(Model)
    monkeypatch.delenv("SCL_AASIST_TRAIN_LENGTHS", raising=False)
    monkeypatch.delenv("SCL_AASIST_LENGTHS", raising=False)
    assert m.head_trains_frames is False and m.head_takes_frames is False
    with pytest.raises(NotImplementedError) as e:      # the refusal as before
        m.forward(torch.zeros(1, 4000), lengths=[4000])
    assert "no padding mask" in str(e.value) and "SCL_AASIST_LENGTHS=1" in str(e.value)
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    assert m.head_trains_frames is True
