"""The packed fp32 scoring path (encoder.SCORE_PACK) with 80- and 120-wide attention heads, the XLS-R 1B / 2B head widths:
tests/test_score_pack_gpu.py on the small encoders and the oracle set-up of tests/test_headdim_model_gpu.py.  model.eval() under no_grad
with `lengths` runs the transformer layers of Encoder.forward_f32 on the valid frames only, with the streaming fp32 attention of
csrc/attention_f32_wide.hip.  PACK_ROWS is set to 64 so that bucket edges are reachable at this size.  The error measure and the 1e-3 bar
are the project's scoring bar (max error over the tensor's max, against the CPU oracle on each utterance ALONE)."""
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
from tests.test_headdim_model_gpu import ARGS, SMALL80, SMALLS, _write_wav, maxrel, model_from, oracle_alone, padded_inputs  # noqa: E402

BAR = 1e-3      # the project's scoring bar
LENGTHS = [20880, 400, 20560, 7777, 12000, 4000]      # 65, 1, 64, 24, 37 and 12 frames: T = 65, Mv = 203, Mq = 256
ROW0 = [0, 65, 66, 130, 154, 191, 203]
LONG = [164240, 400, 30000]      # 513 frames, 1 frame and 93 frames: the padded path chunks, the packed one streams 17 key blocks
# The weights are those of tests/test_headdim_model_gpu.py (its WSEED, chosen there from 41, 51, 61, ... for the bf16 bars).  The baseline
# here is the padded fp32 path on the same batch, which test 1 holds to the same bar before the packed path: fp32 scoring sits two orders
# inside the bar, so no search over seeds was needed.
WSEED = 81
SEED = 2024
_LONG_REF = {}


def _ref(width):
    return oracle_alone("score_pack_" + width, SMALLS[width], LENGTHS, SEED, WSEED)      # a cache key of this file's own: other lengths


def _model(dev, monkeypatch, width, pack=True):
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", pack)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    m, cfg = model_from(dev, SMALLS[width], _ref(width))
    m.eval()
    return m, cfg


def _score(m, x, lengths, dev):
    with torch.no_grad():
        out, feats, emb = m(x.to(dev), lengths=lengths)
    torch.cuda.synchronize()
    return out, feats, emb


def _check(res, outs, lengths, cfg, what):
    out, feats, emb = res
    for b, n in enumerate(lengths):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = outs[b]
        assert rf.shape[1] == Tb
        errs = (maxrel(out[b], ro[0]), maxrel(emb[b], re[0]), maxrel(feats[b, :Tb], rf[0]))
        print("%s n=%d (%d frames): max-rel logp %.2e emb %.2e feats %.2e" % ((what, n, Tb) + errs))
        assert max(errs) < BAR, (what, n, errs)
        assert (feats[b, Tb:] == 0).all()


def test_the_frames_of_the_batches():
    cfg = W2VConfig(**SMALL80)
    assert [cfg.conv_lens(n)[-1] for n in LENGTHS] == [65, 1, 64, 24, 37, 12]
    assert [cfg.conv_lens(n)[-1] for n in LONG] == [513, 1, 93]
    assert [W2VConfig().conv_lens(n)[-1] for n in (64600, 400, 30000)] == [201, 1, 93]


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["80", "120"])
def test_packed_fp32_scoring_matches_the_oracle_on_each_utterance_alone(dev, monkeypatch, width):
    ref = _ref(width)
    m, cfg = _model(dev, monkeypatch, width)
    x, _, T = padded_inputs(cfg, LENGTHS, SEED)
    packed = _score(m, x, LENGTHS, dev)
    assert list(m.encoder._vbufs_f32) == [("f32", len(LENGTHS), max(LENGTHS), "packed")]
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    padded = _score(m, x, LENGTHS, dev)
    _check(padded, ref["outs"], LENGTHS, cfg, "padded fp32 (the baseline: see WSEED), %s-wide heads" % width)
    _check(packed, ref["outs"], LENGTHS, cfg, "packed fp32, %s-wide heads" % width)
    print("packed vs padded fp32 scoring: max-rel logp %.2e feats %.2e emb %.2e"
          % (maxrel(packed[0], padded[0]), maxrel(packed[1], padded[1]), maxrel(packed[2], padded[2])))


# ---- 2. the packed path is really taken ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["80", "120"])
def test_the_switch_selects_the_streaming_kernel_and_its_own_buffer_set(dev, monkeypatch, width):
    m, cfg = _model(dev, monkeypatch, width)
    x, _, T = padded_inputs(cfg, LENGTHS, SEED)
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
    assert T == 65 and calls["f32"] == [(B, T, cfg.heads, int(width), 256, ROW0)] * cfg.layers      # one launch per layer
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
    m, cfg = _model(dev, monkeypatch, "80")
    x, _, _ = padded_inputs(cfg, LENGTHS, SEED)
    base = _score(m, x, LENGTHS, dev)
    noisy = x.clone()
    gen = torch.Generator().manual_seed(3)
    for b, n in enumerate(LENGTHS):
        noisy[b, n:] = torch.randn(x.shape[1] - n, generator=gen)
    again = _score(m, noisy, LENGTHS, dev)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    assert base[1].abs().max() > 0


# ---- 4. a clip above 512 frames -----------------------------------------------------------------------------------------------------------------
def test_a_clip_above_512_frames(dev, monkeypatch):
    m, cfg = _model(dev, monkeypatch, "80")
    x, _, T = padded_inputs(cfg, LONG, 77)
    assert T == 513
    if not _LONG_REF:      # the oracle's forward on each utterance alone (no gradients wanted here)
        base, ocfg = _ref("80"), W.W2VConfig(**SMALL80)
        with torch.no_grad():
            _LONG_REF["outs"] = [tuple(t.clone() for t in OH.full_forward(base["ssl"], base["head"], ocfg, x[b:b + 1, :n].clone()))
                                 for b, n in enumerate(LONG)]
    res = _score(m, x, LONG, dev)
    assert list(m.encoder._vbufs_f32) == [("f32", 3, max(LONG), "packed")]      # no chunk count in the key: no chunks
    _check(res, _LONG_REF["outs"], LONG, cfg, "packed fp32, 513 frames, 80-wide heads")


# ---- 5. XLS-R 1B and 2B layer shapes, packed against padded ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("embed,ffn", [(1280, 5120), (1920, 7680)])
def test_xlsr_1b_and_2b_layer_shapes_packed_and_padded_agree(dev, monkeypatch, embed, ffn):
    """No oracle at this width (it would take minutes), as in the 64-wide file: the packed and the padded fp32 paths within the scoring
    bar of each other — an addressing error (rows, heads, the pitch) is off by O(1)."""
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    cfg = W2VConfig(layers=2, embed=embed, heads=16, ffn=ffn)
    assert cfg.embed // cfg.heads in (80, 120)
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
    print("embed %d, 16 heads of %d, 2 layers: packed vs padded fp32 max-rel logp %.2e feats %.2e emb %.2e" % ((embed, embed // 16) + tuple(errs)))
    assert max(errs) < BAR, errs
    for b, n in enumerate(lengths):
        assert (packed[1][b, cfg.conv_lens(n)[-1]:] == 0).all()
    assert packed[1].abs().max() > 0 and all(torch.isfinite(t).all() for t in packed)


# ---- 6. main.py --eval --padding_type none with the switch on -----------------------------------------------------------------------------------
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
    cfg = {"model": {"name": "wav2vec2_linear_nll", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": dict(SMALL80)},
           "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    made = []
    reg = dict(M.MODEL_REGISTRY)
    ctor = reg["wav2vec2_linear_nll"]
    reg["wav2vec2_linear_nll"] = lambda *a, **k: made.append(ctor(*a, **k)) or made[-1]
    monkeypatch.setattr(M, "MODEL_REGISTRY", reg)
    # the reference: each file scored alone on the padded fp32 path (the switch off)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    ref_model = reg["wav2vec2_linear_nll"](cfg["model"], dev, seed=5)
    assert ref_model.cfg.embed == 160 and ref_model.cfg.heads == 2
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
    assert mm is not ref_model and mm.cfg.embed == 160
    assert mm.encoder._vbufs_f32 and all(k[-1] == "packed" for k in mm.encoder._vbufs_f32)
    assert not mm.encoder._bufs and not mm.encoder._vbufs
