"""Variable-length scoring batches on the ResNet back-end, the parts that need no GPU: the host-side row counts against the shapes torch's
own convolution produces; the minimum frame count against the oracle; the DEFINITION of the masked forward — an fp64 restatement written
here (selection masks at every BatchNorm + activation that feeds a convolution, the average over the utterance's own rows) against
oracle/resnet_head.forward on each utterance alone; the data path's padding to the model's minimum; main.py's start-up refusal; the new
entry points refusing bad arguments.  The header / ctypes agreement is tests/test_abi.py's."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet_head as ORH
from oracle.aasist import fill_state
from scl_amd import lib, pack
from scl_amd import resnet_head as RH


def _conv_rows(T, resnet_type, num_nodes):
    """[T, conv1, layer1 .. layer4, conv5] rows from F.conv2d on one-channel maps (4 wide: only the rows matter), following a stage's
    FIRST block of the given kind — every other convolution of a stage is 3x3 / 1x1 at stride 1 with padding 1 / 0 and keeps the rows."""
    w = lambda kh, kw: torch.zeros(1, 1, kh, kw)
    x = F.conv2d(torch.zeros(1, 1, T, 4), w(9, 3), None, (3, 1), (1, 1))
    out = [T, x.shape[2]]
    bottleneck = RH.STAGES[resnet_type][1]
    for stride in (1, 2, 2, 2):
        skip = F.conv2d(x, w(1, 1), None, stride)
        if bottleneck:
            x = F.conv2d(F.conv2d(F.conv2d(x, w(1, 1)), w(3, 3), None, stride, 1), w(1, 1))
        else:
            x = F.conv2d(F.conv2d(x, w(3, 3), None, stride, 1), w(3, 3), None, 1, 1)
        assert x.shape == skip.shape
        out.append(x.shape[2])
    out.append(F.conv2d(x, w(num_nodes, 3), None, 1, (0, 1)).shape[2])
    return out


@pytest.mark.parametrize("resnet_type", ["18", "50"])
@pytest.mark.parametrize("num_nodes", [3, 1])
def test_row_counts_are_the_shapes_torch_conv2d_produces(resnet_type, num_nodes):
    lo = RH.min_frames(resnet_type, num_nodes)
    for T in range(lo, 701):
        assert RH.layer_rows(T, resnet_type, num_nodes) == _conv_rows(T, resnet_type, num_nodes), T
    assert RH.layer_rows(lo - 1, resnet_type, num_nodes)[-1] < 1 <= RH.layer_rows(lo, resnet_type, num_nodes)[-1]


def test_the_issue_examples_and_the_batch_table():
    assert RH.layer_rows(55)[1:] == [17, 17, 9, 5, 3, 1]
    assert RH.layer_rows(78)[1:] == [24, 24, 12, 6, 3, 1]
    assert RH.layer_rows(79)[1:] == [25, 25, 13, 7, 4, 2]
    rows = RH.batch_rows([55, 79, 78])
    assert len(rows) == RH.N_LEVELS and rows[0] == [55, 79, 78] and rows[1] == [17, 25, 24] and rows[6] == [1, 2, 1]
    with pytest.raises(ValueError, match="at least 55 frames"):
        RH.batch_rows([60, 54])
    with pytest.raises(ValueError):
        RH.layer_rows(60, "19")


def _oracle_state(cfg, seed, dtype=torch.float64):
    head = RH.ResNetHead(cfg)
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    return {k: torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in fill_state(shapes, seed=seed).items()}


@pytest.mark.parametrize("resnet_type,num_nodes", [("18", 3), ("18", 1), ("50", 3)])
def test_minimum_frame_count_is_the_smallest_the_oracle_runs(resnet_type, num_nodes):
    t = _oracle_state(dict(RH.DEFAULT_RESNET, resnet_type=resnet_type, num_nodes=num_nodes), 3, torch.float32)
    lo = RH.min_frames(resnet_type, num_nodes)

    def runs(T):
        try:
            with torch.no_grad():
                out, emb = ORH.forward(t, torch.zeros(1, T, 8), False)      # 8 wide: the row counts do not depend on the width
            return bool(torch.isfinite(emb).all())      # a mean over no rows is NaN where torch lets an empty map through
        except RuntimeError:
            return False
    assert runs(lo) and not any(runs(T) for T in range(max(1, lo - 12), lo))
    if (resnet_type, num_nodes) == ("18", 3):
        assert lo == 55


def _masked_forward(t, feats, frames, resnet_type, num_nodes):
    """The definition: oracle/resnet_head.forward in eval mode with (a) every BatchNorm + activation that feeds a convolution set to 0, by
    selection, in the rows at or beyond the utterance's own row count of that map and (b) bn5's output averaged over the utterance's own
    rows.  Written on the oracle's state-dict names, independent of the product code but for the row counts."""
    rows = torch.tensor(RH.batch_rows(frames, resnet_type, num_nodes))      # [levels, B]

    def bn(x, name):
        return F.batch_norm(x, t[name + ".running_mean"], t[name + ".running_var"], t[name + ".weight"], t[name + ".bias"], False, 0.1, 1e-5)

    def mask(x, level):      # x [B, C, H, W]
        keep = torch.arange(x.shape[2])[None, :] < rows[level][:, None]      # [B, H]
        return torch.where(keep[:, None, :, None], x, torch.zeros((), dtype=x.dtype))

    x = mask(F.selu(bn(feats.unsqueeze(1), "first_bn")), 0)
    x = F.relu(bn(F.conv2d(x, t["resnet.conv1.weight"], None, (3, 1), (1, 1)), "resnet.bn1"))
    for s in (1, 2, 3, 4):
        j = 0
        while "resnet.layer%d.%d.bn1.weight" % (s, j) in t:
            p = "resnet.layer%d.%d." % (s, j)
            stride = 2 if (s > 1 and j == 0) else 1
            lin, lout = (s if j == 0 else s + 1), s + 1
            a = mask(F.relu(bn(x, p + "bn1")), lin)
            skip = F.conv2d(a, t[p + "shortcut.0.weight"], None, stride) if (p + "shortcut.0.weight") in t else x
            if (p + "conv3.weight") in t:
                h = F.conv2d(a, t[p + "conv1.weight"])
                h = F.conv2d(mask(F.relu(bn(h, p + "bn2")), lin), t[p + "conv2.weight"], None, stride, 1)
                h = F.conv2d(mask(F.relu(bn(h, p + "bn3")), lout), t[p + "conv3.weight"])
            else:
                h = F.conv2d(a, t[p + "conv1.weight"], None, stride, 1)
                h = F.conv2d(mask(F.relu(bn(h, p + "bn2")), lout), t[p + "conv2.weight"], None, 1, 1)
            x = h + skip
            j += 1
    x = mask(F.relu(bn(F.conv2d(x, t["resnet.conv5.weight"], None, 1, (0, 1)), "resnet.bn5")), 6)
    emb = x.sum(dim=(2, 3)) / (rows[6][:, None] * x.shape[3]).to(x.dtype)
    return F.linear(emb, t["resnet.fc.weight"], t["resnet.fc.bias"]), emb


FRAMES = [55, 56, 78, 79, 103, 130, 201]


@pytest.mark.parametrize("resnet_type,width", [("18", 32), ("50", 16)])
def test_the_masked_definition_equals_the_oracle_on_each_utterance_alone(resnet_type, width):
    """fp64 on both sides, junk of magnitude 1e6 in the padding of feats (and whatever the convolutions make of it further down): every row
    of the padded batch within 1e-12 relative of the oracle on that utterance alone (measured for type 18 at full width: 1.2e-15).  Both
    block kinds; the maps are `width` wide instead of 128 to keep the fp64 CPU convolutions quick — no step of the definition looks at the
    width axis."""
    torch.manual_seed(11)
    t = _oracle_state(dict(RH.DEFAULT_RESNET, resnet_type=resnet_type), 5)
    T = max(FRAMES)
    clean = torch.randn(len(FRAMES), T, width, dtype=torch.float64)
    feats = clean.clone()
    for b, n in enumerate(FRAMES):
        feats[b, n:] = 1e6 * torch.randn(T - n, width, dtype=torch.float64)
    with torch.no_grad():
        out, emb = _masked_forward(t, feats, FRAMES, resnet_type, 3)
        worst = 0.0
        for b, n in enumerate(FRAMES):
            ro, re = ORH.forward(t, clean[b:b + 1, :n], False)
            for got, ref in ((out[b:b + 1], ro), (emb[b:b + 1], re)):
                worst = max(worst, ((got - ref).abs().max() / ref.abs().max()).item())
    print("resnet %s: worst relative difference %.2e" % (resnet_type, worst))
    assert worst < 1e-12


def test_eval_dataset_pads_a_short_file_to_min_samples(tmp_path):
    path = tmp_path / "short.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(0.1 * np.random.RandomState(0).randn(3000), -1, 1) * 32767).astype("<i2").tobytes())
    ds = pack.EvalDataset(["short.wav"], str(tmp_path), padding_type="none", subdir="")
    assert ds.min_samples == pack.VARLEN_MIN_SAMPLES == 400
    x, uid = ds[0]
    assert uid == "short.wav" and x.shape == (3000,)      # above the default minimum: the file as it is
    ds.min_samples = 17680
    x2, _ = ds[0]
    assert x2.shape == (17680,) and torch.equal(x2[:3000], x) and (x2[3000:] == 0).all() and x2.dtype == torch.float32


def test_min_samples_follow_the_back_end():
    from scl_amd.encoder import W2VConfig
    from scl_amd.model_front import FrontHeadModel
    from scl_amd.model_resnet import Model
    assert W2VConfig().samples_for(55) == 17680 and W2VConfig().samples_for(1) == W2VConfig().min_samples() == 400
    for n in (1, 55, 200):
        L = W2VConfig().samples_for(n)
        assert W2VConfig().conv_lens(L)[-1] == n and W2VConfig().conv_lens(L - 1)[-1] == n - 1
    assert Model.head_takes_frames is True and FrontHeadModel.head_takes_frames is False
    assert "wav2vec2_linear_nll" in FrontHeadModel.VARLEN_REFUSAL and "wav2vec2_resnet_nll" in FrontHeadModel.VARLEN_REFUSAL


@pytest.mark.parametrize("name", ["wav2vec2_aasist"])
def test_main_still_refuses_the_other_back_ends_at_start_up(name, tmp_path, monkeypatch):
    import yaml
    import main as M
    assert M.VARLEN_MODELS == ("wav2vec2_linear_nll", "wav2vec2_resnet_nll")
    cfg = {"model": {"name": name, "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "eval_only", "kwargs": {}}}
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)      # the refusal comes before anything touches a device
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    with pytest.raises(SystemExit) as e:
        M.main(["--config", str(tmp_path / "conf.yaml"), "--database_path", str(tmp_path), "--eval", "--padding_type", "none",
                "--eval_output", str(tmp_path / "x.txt")])
    assert "wav2vec2_linear_nll only" in str(e.value) and "wav2vec2_resnet_nll" in str(e.value) and name in str(e.value)


def test_entry_points_refuse_null_and_bad_arguments_without_touching_the_gpu():
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # a 16-byte aligned host address: a refused call never dereferences it
    bn = lambda **kw: L.scl_bn_eval_masked(*[kw.get(k, d) for k, d in (("x", p), ("B", 2), ("H", 3), ("W", 4), ("C", 16), ("gamma", p), ("beta", p),
                                                                     ("rm", p), ("rv", p), ("eps", 1e-5), ("act", 1), ("valid", p), ("mean", p),
                                                                     ("rstd", p), ("y", p), ("stream", None))])
    for kw in (dict(x=None), dict(rm=None), dict(rv=None), dict(valid=None), dict(mean=None), dict(rstd=None), dict(y=None)):
        assert bn(**kw) == -1 and b"bn_eval_masked" in L.scl_last_error(), kw
    for kw in (dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(C=0), dict(C=3), dict(C=4096), dict(act=3), dict(act=-1),
               dict(H=1 << 15, W=1 << 12)):      # H * W * C = 2^31
        assert bn(**kw) == -1 and b"bn_eval_masked" in L.scl_last_error(), kw
    odd = ctypes.c_void_p(p.value + 4)
    assert bn(x=odd) == -1 and b"16-byte" in L.scl_last_error()
    avg = lambda x=p, valid=p, B=2, H=3, W=4, C=256, y=p: L.scl_avgpool_fwd_masked(x, valid, B, H, W, C, y, None)
    for kw in (dict(x=None), dict(valid=None), dict(y=None), dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(H=1 << 16, W=1 << 15)):
        assert avg(**kw) == -1 and b"avgpool_fwd_masked" in L.scl_last_error(), kw
