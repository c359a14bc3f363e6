"""The packed fp32 scoring path at model level (encoder.SCORE_PACK): model.eval() under no_grad with `lengths` runs the transformer
layers of Encoder.forward_f32 on the valid frames only, with the streaming fp32 attention of csrc/attention_f32.hip.  The small encoder
and the oracle set-up of tests/test_varlen_train_gpu.py / tests/test_varlen_pack_gpu.py; PACK_ROWS is set to 64 so that bucket edges are
reachable at this size.  The error measure and the 1e-3 bar are those of tests/test_varlen_gpu.py's fp32 cases (max error over the
tensor's max, against the CPU oracle on each utterance ALONE)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests import test_varlen_train_gpu as VT  # noqa: E402
from tests.test_varlen_gpu import _write_wav  # noqa: E402
from tests.test_varlen_pack_gpu import FULL, LENGTHS, _inputs, _oracle  # noqa: E402
from tests.test_varlen_train_gpu import ARGS, SMALL, maxrel  # noqa: E402

BAR = 1e-3      # the project's scoring bar
LONG = [164240, 400, 30000]      # 513 frames, 1 frame and 93 frames: the padded path chunks, the packed one streams nine key blocks
_LONG_REF = {}


def _model(dev, monkeypatch, pack=True):
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", pack)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    m, cfg = VT._train_model(dev, monkeypatch)      # the oracle's weights
    m.eval()
    return m, cfg


def _score(m, x, lengths, dev):
    with torch.no_grad():
        out, feats, emb = m(x.to(dev), lengths=lengths)
    torch.cuda.synchronize()
    return out, feats, emb


def _check(res, outs, lengths, cfg, what):
    out, feats, emb = res
    worst = 0.0
    for b, n in enumerate(lengths):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = outs[b]
        assert rf.shape[1] == Tb
        errs = (maxrel(out[b], ro[0]), maxrel(emb[b], re[0]), maxrel(feats[b, :Tb], rf[0]))
        print("%s n=%d (%d frames): max-rel logp %.2e emb %.2e feats %.2e" % ((what, n, Tb) + errs))
        assert max(errs) < BAR, (what, n, errs)
        assert (feats[b, Tb:] == 0).all()
        worst = max(worst, max(errs))
    return worst


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------
def test_packed_fp32_scoring_matches_the_oracle_on_each_utterance_alone(dev, monkeypatch):
    ref = _oracle(LENGTHS)
    x, _, T = _inputs(LENGTHS)
    m, cfg = _model(dev, monkeypatch)
    packed = _score(m, x, LENGTHS, dev)
    _check(packed, ref["outs"], LENGTHS, cfg, "packed fp32")
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    padded = _score(m, x, LENGTHS, dev)
    _check(padded, ref["outs"], LENGTHS, cfg, "padded fp32")
    print("packed vs padded fp32 scoring: max-rel logp %.2e feats %.2e emb %.2e"
          % (maxrel(packed[0], padded[0]), maxrel(packed[1], padded[1]), maxrel(packed[2], padded[2])))


# ---- 2. the packed path is really taken ---------------------------------------------------------------------------------------------------
def test_the_switch_selects_the_streaming_kernel_and_its_own_buffer_set(dev, monkeypatch):
    x, _, T = _inputs(LENGTHS)
    m, cfg = _model(dev, monkeypatch)
    B, L = len(LENGTHS), max(LENGTHS)
    calls = {"f32": [], "softmax": 0}
    attn, softmax = ops.attn_fwd_packed_f32, ops.softmax_fwd_f32_varlen

    def count_attn(qkv, ctx, row0, B_, T_, H, D, Mq, scale):
        calls["f32"].append((B_, T_, H, D, Mq, row0.tolist()))
        return attn(qkv, ctx, row0, B_, T_, H, D, Mq, scale)

    def count_softmax(*a, **k):
        calls["softmax"] += 1
        return softmax(*a, **k)
    monkeypatch.setattr(ops, "attn_fwd_packed_f32", count_attn)
    monkeypatch.setattr(ops, "softmax_fwd_f32_varlen", count_softmax)
    _score(m, x, LENGTHS, dev)
    assert calls["f32"] == [(B, T, cfg.heads, 64, 256, [0, 65, 66, 130, 154, 191, 203])] * cfg.layers      # one launch per layer
    assert calls["softmax"] == 0
    assert list(m.encoder._vbufs_f32) == [("f32", B, L, "packed")]
    d = m.encoder._vbufs_f32[("f32", B, L, "packed")]
    assert "S" not in d and "Pm" not in d and d["xa"].numel() == 448 * cfg.embed      # roundup(6 * 65, 64) rows, no score buffers
    assert not m.encoder._vbufs and not m.encoder._bufs      # SCL_VARLEN_PACK's sets are not involved
    # switch off: the same call takes the padded path and its own key
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    _score(m, x, LENGTHS, dev)
    assert len(calls["f32"]) == cfg.layers and calls["softmax"] == cfg.layers
    assert list(m.encoder._vbufs_f32) == [("f32", B, L, "packed"), ("f32", B, L)]


# ---- 3. what the padding holds does not matter ---------------------------------------------------------------------------------------------
def test_padding_content_does_not_change_a_bit(dev, monkeypatch):
    x, _, _ = _inputs(LENGTHS)
    m, _ = _model(dev, monkeypatch)
    base = _score(m, x, LENGTHS, dev)
    noisy = x.clone()
    gen = torch.Generator().manual_seed(3)
    for b, n in enumerate(LENGTHS):
        noisy[b, n:] = torch.randn(x.shape[1] - n, generator=gen)
    again = _score(m, noisy, LENGTHS, dev)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    assert base[1].abs().max() > 0


# ---- 4. every frame valid ---------------------------------------------------------------------------------------------------------------------
def test_every_frame_valid(dev, monkeypatch):
    """Nothing to skip: Mq = roundup(B * T, 64) = 256 rows for 195 frames, the pack and the unpack copy every row."""
    ref = _oracle(FULL)
    x, _, _ = _inputs(FULL)
    m, cfg = _model(dev, monkeypatch)
    _check(_score(m, x, FULL, dev), ref["outs"], FULL, cfg, "packed fp32, every frame valid")


# ---- 5. a clip above 512 frames -----------------------------------------------------------------------------------------------------------------
def test_a_clip_above_512_frames(dev, monkeypatch):
    cfg0 = W2VConfig(**SMALL)
    assert [cfg0.conv_lens(n)[-1] for n in LONG] == [513, 1, 93]
    x, _, T = _inputs(LONG)
    if not _LONG_REF:      # the oracle's forward on each utterance alone (no gradients wanted here)
        base, ocfg = VT._oracle_alone(), W.W2VConfig(**SMALL)
        with torch.no_grad():
            _LONG_REF["outs"] = [tuple(t.clone() for t in OH.full_forward(base["ssl"], base["head"], ocfg, x[b:b + 1, :n].clone()))
                                 for b, n in enumerate(LONG)]
    m, cfg = _model(dev, monkeypatch)
    res = _score(m, x, LONG, dev)
    assert list(m.encoder._vbufs_f32) == [("f32", 3, max(LONG), "packed")]      # no chunk count in the key: no chunks
    _check(res, _LONG_REF["outs"], LONG, cfg, "packed fp32, 513 frames")


# ---- 6. XLS-R width, packed against padded ------------------------------------------------------------------------------------------------------
def test_xlsr_width_packed_and_padded_agree(dev, monkeypatch):
    """No oracle at this width (it would take minutes): the packed and the padded fp32 paths within the scoring bar of each other — an
    addressing error (rows, heads, the 1024-wide pitch) is off by O(1)."""
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    cfg = W2VConfig(layers=2)
    assert cfg.embed == 1024 and cfg.heads == 16 and cfg.ffn == 4096
    m = Model(ARGS, dev, w2v_cfg=cfg, seed=17)
    m.eval()
    lengths = [64600, 400, 30000]      # 201 frames, 1 frame and 93 frames
    gen = torch.Generator().manual_seed(177)
    x = torch.zeros(3, 64600)
    for b, n in enumerate(lengths):
        x[b, :n] = 0.1 * torch.randn(n, generator=gen)
    monkeypatch.setattr(ENC, "SCORE_PACK", True)
    packed = _score(m, x, lengths, dev)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    padded = _score(m, x, lengths, dev)
    assert list(m.encoder._vbufs_f32) == [("f32", 3, 64600, "packed"), ("f32", 3, 64600)]
    errs = [maxrel(a, b) for a, b in zip(packed, padded)]
    print("XLS-R width, 2 layers: packed vs padded fp32 max-rel logp %.2e feats %.2e emb %.2e" % tuple(errs))
    assert max(errs) < BAR, errs
    for b, n in enumerate(lengths):
        assert (packed[1][b, cfg.conv_lens(n)[-1]:] == 0).all()
    assert packed[1].abs().max() > 0 and all(torch.isfinite(t).all() for t in packed)


# ---- 7. 16-wide heads ------------------------------------------------------------------------------------------------------------------------------
def test_other_head_widths_are_refused_loudly(dev, monkeypatch):
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", True)
    m = Model(ARGS, dev, w2v_cfg=W2VConfig.tiny())
    m.eval()
    x = torch.zeros(2, 4000, device=dev)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="SCL_SCORE_PACK"):
        m(x, lengths=[4000, 1000])
    monkeypatch.setattr(ENC, "SCORE_PACK", False)      # and the padded path serves them as before
    with torch.no_grad():
        out, _, _ = m(x, lengths=[4000, 1000])
    assert torch.isfinite(out).all()


# ---- 8. main.py --eval --padding_type none with the switch on -----------------------------------------------------------------------------------
def test_main_eval_padding_type_none_scores_on_the_packed_path(dev, tmp_path, monkeypatch):
    import yaml
    import main as M
    from scl_amd import pack
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    sizes = [3000, 9000, 30000, 70000, 24000]
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(root / u), 0.1 * rs.randn(n))
    (root / "protocol.txt").write_text("".join("%s eval bonafide\n" % u for u in ids))
    cfg = {"model": {"name": "wav2vec2_linear_nll", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    made = []
    reg = dict(M.MODEL_REGISTRY)
    ctor = reg["wav2vec2_linear_nll"]
    # 64-wide heads (the YAML's tiny preset has 16-wide ones, which the packed fp32 path refuses)
    reg["wav2vec2_linear_nll"] = lambda *a, **k: made.append(ctor(*a, w2v_cfg=W2VConfig(**SMALL), **k)) or made[-1]
    monkeypatch.setattr(M, "MODEL_REGISTRY", reg)
    # the reference: each file scored alone on the padded fp32 path (the switch off)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    ref_model = reg["wav2vec2_linear_nll"](cfg["model"], dev, seed=5)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    want_lp = []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            o, _, _ = ref_model(x[None].to(dev), lengths=[n])
            want_lp.append(o[0].cpu().numpy())
    assert all(k[-1] != "packed" for k in ref_model.encoder._vbufs_f32)
    monkeypatch.setattr(ENC, "SCORE_PACK", True)
    out = tmp_path / "scores.txt"
    assert M.main(["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--eval", "--model_path", str(ck),
                   "--padding_type", "none", "--eval_output", str(out)]) == 0
    lines = out.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids      # exactly five lines, protocol order
    relerr = lambda got, ref: np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()
    for l, ref in zip(lines, want_lp):
        err = relerr([float(v) for v in l.split()[1:]], ref)
        print("%s: packed batch vs the file alone %.2e" % (l.split()[0], err))
        assert err < BAR, (l, ref)
    mm = made[-1]
    assert mm is not ref_model and mm.encoder._vbufs_f32 and all(k[-1] == "packed" for k in mm.encoder._vbufs_f32)
    assert not mm.encoder._bufs and not mm.encoder._vbufs
