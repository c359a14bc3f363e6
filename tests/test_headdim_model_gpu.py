"""Encoders with 80- and 120-wide attention heads (XLS-R 1B / 2B head widths) through the linear plugin: variable-length scoring and
training, the packed layout, a clip beyond 512 frames, one XLS-R 1B sized layer pair, and main.py with the mapping form of `w2v_arch`.
All of it runs the streaming attention of csrc/attention_wide.hip; the oracle is oracle.wav2vec2 with the same config on the CPU.

The bars are those of the 64-wide tests: tests/test_varlen_gpu.py and tests/test_varlen_train_gpu.py (outputs rel-L2 < 1e-2 and max-rel
< 3e-2; gradients cosine > 0.99 and max error < 20 % of the tensor's max, 25 % for the frame-level head, 2e-3 absolute where the
reference is zero), tests/test_long_clip_gpu.py (losses 3e-2, gradient cosines 0.995 / 0.99 for LL.weight) and tests/test_model_gpu.py's
full-size gradient bars (rel-L2 < 6e-2 and cosine > 0.998; frame-level head 1e-1 and 0.995)."""
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd.encoder import VARLEN_SETS, W2VConfig  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests.test_long_clip_gpu import GRADS as LONG_GRADS  # noqa: E402
from tests.test_varlen_train_gpu import LENGTHS, cosine, relerr  # noqa: E402

ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
CONF = {"model": {"contra_mode": "all", "loss_type": 1}}
SMALL80 = dict(conv_dim=32, embed=160, layers=2, heads=2, ffn=320, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)
SMALL120 = dict(SMALL80, embed=240, ffn=480, pos_groups=6)
SMALLS = {"80": SMALL80, "120": SMALL120}
XLSR_1B_LAYERS = dict(embed=1280, layers=2, heads=16, ffn=5120, final_dim=1024)
XLSR_1B_LENGTHS = [16400, 9040]      # 51 and 28 frames
# The oracle weights of tests 1 and 2.  At embed 160 / 240 with 1- to 37-frame utterances the bf16 encoder as a whole sits AT the 64-wide
# tests' bars against the fp32 oracle whatever the attention kernel: the unchanged path — each utterance alone on fixed rows, through the
# materialised-score chain — misses them for about half of the weight draws (seeds 41, 51, .. 131: feats rel-L2 5.8e-3 .. 1.4e-2 against the bar
# of 1e-2; the frame-level head's gradients, which sit behind LeakyReLU slope flips, up to 0.38 of the tensor max against 0.25), 1-frame
# utterances included, where soft-max = 1 and both paths give the same bits.  A test of the streaming kernels needs weights on which that
# baseline meets the bars, or it cannot tell the kernels from the encoder's rounding: 81 is the first seed of 41, 51, 61, ... at which the
# baseline meets them at both widths (feats 6.5e-3 / 8.8e-3).  The tests assert the baseline's bars too; the streaming path is 2e-3 from it.
WSEED = 81
NO_DROP = dict(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, dropout_input=0.0)


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def close_bf16(got, ref):      # test_model_gpu.py's bar for outputs
    return rl2(got, ref) < 1e-2 and maxrel(got, ref) < 3e-2


def test_the_head_dims_of_the_configs():
    assert W2VConfig(**SMALL80).embed // 2 == 80 and W2VConfig(**SMALL120).embed // 2 == 120
    assert [W2VConfig(**SMALL80).conv_lens(n)[-1] for n in (164240, 164239)] == [513, 512]
    assert [W2VConfig().conv_lens(n)[-1] for n in XLSR_1B_LENGTHS] == [51, 28]


def padded_inputs(cfg, lengths, seed):
    """tests/test_varlen_train_gpu.py's _inputs for any config: the zero-padded batch and fixed upstream gradients (d_out, d_feats, d_emb)."""
    gen = torch.Generator().manual_seed(seed)
    B, L = len(lengths), max(lengths)
    T = cfg.conv_lens(L)[-1]
    x = torch.zeros(B, L)
    for b, n in enumerate(lengths):
        x[b, :n] = 0.1 * torch.randn(n, generator=gen)
    ups = (0.3 * torch.randn(B, 2, generator=gen), 0.01 * torch.randn(B, T, 128, generator=gen), 0.05 * torch.randn(B, 128, generator=gen))
    return x, ups, T


_ORACLE = {}


def oracle_alone(name, cfg_kw, lengths, seed, wseed=41):
    """CPU oracle, fp32 autograd (tests/test_varlen_train_gpu.py's _oracle_alone for any config): every utterance alone at its own length;
    the parameter gradients of <upstream, outputs> summed over the utterances, and each utterance's outputs.  Once per config."""
    if name not in _ORACLE:
        ocfg = W.W2VConfig(**cfg_kw)
        ssl, head = W.init_state(ocfg, seed=wseed), OH.init_head(ocfg.embed, seed=wseed + 1)      # 41 / 42: tests/test_varlen_gpu.py's weights
        x, (d_out, d_feats, d_emb), _ = padded_inputs(W2VConfig(**cfg_kw), lengths, seed)
        params = {"ssl_model.model." + n: ssl[n] for n, _, tr in W.param_shapes(ocfg) if tr}
        params.update(head)
        for p in params.values():
            p.requires_grad_(True)
        outs = []
        for b, n in enumerate(lengths):
            o, f, e = OH.full_forward(ssl, head, ocfg, x[b:b + 1, :n].clone())
            Tb = f.shape[1]
            ((o * d_out[b:b + 1]).sum() + (f * d_feats[b:b + 1, :Tb]).sum() + (e * d_emb[b:b + 1]).sum()).backward()
            outs.append((o.detach().clone(), f.detach().clone(), e.detach().clone()))
        grads = {k: p.grad.detach().clone() for k, p in params.items()}
        for p in params.values():
            p.requires_grad_(False)
            p.grad = None
        _ORACLE[name] = dict(grads=grads, outs=outs, ssl=ssl, head=head)
    return _ORACLE[name]


def model_from(dev, cfg_kw, ref):
    cfg = W2VConfig(**cfg_kw, **NO_DROP)
    m = Model(ARGS, dev, w2v_cfg=cfg)
    sd = {"ssl_model.model." + k: v for k, v in ref["ssl"].items()}
    sd.update(ref["head"])
    m.load_state_dict(sd, strict=False)
    return m, cfg


def train_step(m, x, lengths, ups, dev):
    out, feats, emb = m(x.to(dev), lengths=lengths)
    torch.autograd.backward([out, feats, emb], [u.to(dev) for u in ups])
    torch.cuda.synchronize()
    return out.detach().clone(), feats.detach().clone(), emb.detach().clone(), m.P.grad.clone()


def check_outputs(outs, refs, lengths, cfg, what, padded=True):
    """outs: (out, feats, emb) of the padded batch, or with padded=False one such triple per utterance alone."""
    for b, n in enumerate(lengths):
        out, feats, emb = (t[b] for t in outs) if padded else (t[0] for t in outs[b])
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = refs[b]
        errs = [(rl2(g, r), maxrel(g, r)) for g, r in ((out, ro[0]), (emb, re[0]), (feats[:Tb], rf[0]))]
        print("%s n=%d (%d frames): (rel-L2, max-rel) logp %s emb %s feats %s" % ((what, n, Tb) + tuple("(%.2e, %.2e)" % e for e in errs)))
        assert all(e[0] < 1e-2 and e[1] < 3e-2 for e in errs), (what, n, errs)
        assert (feats[Tb:] == 0).all()


def check_grads(got_of, ref_grads, what, exact=None):
    """tests/test_varlen_train_gpu.py's gradient bars over every tensor of ref_grads; got_of(name) -> the tensor under test.  exact: the
    oracle's gradients where ref_grads are another GPU run's — a tensor whose true gradient is zero (the key bias: a soft-max does not
    see a shift of all keys) holds rounding noise in both runs, and gets the absolute bar in both."""
    bad, cnt, worst = [], 0, (1.0, 0.0)
    for name, r in ref_grads.items():
        got = got_of(name).float().cpu()
        cnt += 1
        if (ref_grads if exact is None else exact)[name].abs().max().item() < 1e-6:
            ok = got.abs().max().item() < 2e-3 and r.abs().max().item() < 2e-3
        else:
            lim = 0.25 if name.startswith("backend.m_frame_level") else 0.2
            c, e = cosine(got, r), relerr(got, r)
            worst = (min(worst[0], c), max(worst[1], e))
            ok = c > 0.99 and e < lim
        if not ok:
            bad.append((name, cosine(got, r), relerr(got, r)))
    print("%s: %d tensors, worst cosine %.5f, worst max error %.3f of the tensor max" % (what, cnt, worst[0], worst[1]))
    assert cnt > 60 and not bad, (what, bad)


# ---- 1. the linear plugin with `lengths`: bf16 scoring and one training step -------------------------------------------------------------
@pytest.mark.parametrize("width", ["80", "120"])
def test_lengths_batch_scoring_and_training_match_the_utterances_alone_and_the_oracle(dev, monkeypatch, width):
    monkeypatch.setattr(ML, "SCORE_FP32", False)
    monkeypatch.setattr(ML, "DROP_P", 0.0)
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    ref = oracle_alone(width, SMALLS[width], LENGTHS, 2024, WSEED)
    m, cfg = model_from(dev, SMALLS[width], ref)
    x, ups, T = padded_inputs(cfg, LENGTHS, 2024)
    # bf16 scoring
    m.eval()
    with torch.no_grad():
        score = tuple(t.clone() for t in m(x.to(dev), lengths=LENGTHS))
        alone = [tuple(t.clone() for t in m(x[b:b + 1, :n].to(dev))) for b, n in enumerate(LENGTHS)]      # fixed rows: the materialised chain
    torch.cuda.synchronize()
    d, = m.encoder._vbufs.values()
    assert d["long_attn"] and not d["fused_attn"] and "S" not in d
    check_outputs(alone, ref["outs"], LENGTHS, cfg, "alone vs oracle (the baseline: see WSEED)", padded=False)
    check_outputs(score, ref["outs"], LENGTHS, cfg, "scoring vs oracle")
    check_outputs(score, alone, LENGTHS, cfg, "scoring vs alone")
    # one training step
    m.train()
    step = train_step(m, x, LENGTHS, ups, dev)
    d, = m.encoder._vbufs_train.values()
    assert d["long_attn"] and "attn_ws" in d and "S" not in d and d["dS"] is None      # no T x T buffers
    check_outputs(step[:3], ref["outs"], LENGTHS, cfg, "training vs oracle")
    check_grads(m.P.g, ref["grads"], "training vs oracle")
    batch_grad = step[3]
    alone_outs, alone_grad = [], torch.zeros_like(batch_grad)
    for b, n in enumerate(LENGTHS):
        Tb = cfg.conv_lens(n)[-1]
        o, f, e = m(x[b:b + 1, :n].to(dev))
        torch.autograd.backward([o, f, e], [ups[0][b:b + 1].to(dev), ups[1][b:b + 1, :Tb].to(dev), ups[2][b:b + 1].to(dev)])
        torch.cuda.synchronize()
        alone_outs.append((o.detach().clone(), f.detach().clone(), e.detach().clone()))
        alone_grad += m.P.grad
    check_outputs(step[:3], alone_outs, LENGTHS, cfg, "training vs alone")
    seg = lambda flat, name: flat[m.P.off(name):m.P.off(name) + ref["grads"][name].numel()]
    check_grads(lambda name: seg(batch_grad, name), {k: seg(alone_grad, k).float().cpu() for k in ref["grads"]}, "training vs alone",
                exact=ref["grads"])


# ---- 2. the packed layout against the padded one -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["80", "120"])
def test_packed_path_against_the_padded_path(dev, monkeypatch, width):
    """SCL_VARLEN_PACK=1 and the padded path on the same batch, as tests/test_varlen_pack_gpu.py holds them together: the attention
    kernels carry the same bits in both layouts (tests/test_attention_headdim_gpu.py), so the forward — row-wise kernels around the
    attention, each row computed from its own row — gives every output bit for bit.  The weight gradients are sums over the rows in
    another order (other GEMM plans for another row count): they are held to the oracle at the padded path's bars, as that file does."""
    monkeypatch.setattr(ML, "DROP_P", 0.0)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    ref = oracle_alone(width, SMALLS[width], LENGTHS, 2024, WSEED)
    m, cfg = model_from(dev, SMALLS[width], ref)
    x, ups, T = padded_inputs(cfg, LENGTHS, 2024)
    m.train()
    monkeypatch.setattr(ENC, "VARLEN_PACK", True)
    packed = train_step(m, x, LENGTHS, ups, dev)
    keys = [k for k in m.encoder._vbufs_train if k[-1] == "packed"]
    assert len(keys) == 1 and m.encoder._vbufs_train[keys[0]]["long_attn"]
    check_outputs(packed[:3], ref["outs"], LENGTHS, cfg, "packed vs oracle")
    check_grads(m.P.g, ref["grads"], "packed vs oracle")
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    padded = train_step(m, x, LENGTHS, ups, dev)
    diffs = [maxrel(a, b) for a, b in zip(packed[:3], padded[:3])]
    gdiff = max(relerr(packed[3][m.P.off(n):m.P.off(n) + r.numel()], padded[3][m.P.off(n):m.P.off(n) + r.numel()]) for n, r in ref["grads"].items())
    print("packed vs padded: outputs max-rel %.2e / %.2e / %.2e; gradients worst max error %.3e of the tensor max" % (tuple(diffs) + (gdiff,)))
    assert all(torch.equal(a, b) for a, b in zip(packed[:3], padded[:3])), diffs


# ---- 3. a clip beyond 512 frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["80", "120"])
def test_a_513_frame_clip_takes_the_streaming_attention_and_matches_the_oracle(dev, width):
    """tests/test_long_clip_gpu.py::test_long_clips_take_the_streaming_attention_and_match_oracle at 513 frames, B = 2, both clips of one
    class (the SupCon terms are then 0 in the reference too and L_CE carries the comparison)."""
    ocfg = W.W2VConfig(**SMALLS[width])
    ssl, head = W.init_state(ocfg, seed=41), OH.init_head(ocfg.embed, seed=42)
    m, cfg = model_from(dev, SMALLS[width], dict(ssl=ssl, head=head))
    m.eval()
    B, L = 2, 164240
    x = 0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(3))
    y = torch.tensor([1, 1])
    out, feats, emb = m(x.to(dev))
    bufs = m.encoder.bufs(B, L)
    assert bufs["T"] == 513 and bufs["long_attn"] and not bufs["fused_attn"] and "S" not in bufs and "P" not in bufs
    losses = m.loss(out, feats, emb, y.to(dev), CONF)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    ref_losses, ref_grads, (ro, rf, re), _ = OH.train_step(ssl, head, ocfg, x, y)
    print("513 frames, %s-wide heads: rl2 out %.2e feats %.2e emb %.2e" % (width, rl2(out, ro), rl2(feats, rf), rl2(emb, re)))
    assert close_bf16(out, ro) and close_bf16(feats, rf) and close_bf16(emb, re), (rl2(out, ro), rl2(feats, rf), rl2(emb, re))
    for k, v in ref_losses.items():
        assert abs(losses[k].item() - v) <= 3e-2 * max(abs(v), 1e-3), (k, losses[k].item(), v)
    for name in LONG_GRADS:
        c = cosine(m.P.g(name), ref_grads[name])
        assert c > (0.99 if name == "LL.weight" else 0.995), (name, c)


# ---- 4. two layers of XLS-R 1B's shape -----------------------------------------------------------------------------------------------------
XLSR_1B_GRADS = [
    "ssl_model.model.feature_extractor.conv_layers.0.0.weight", "ssl_model.model.feature_extractor.conv_layers.1.0.weight",
    "ssl_model.model.feature_extractor.conv_layers.6.0.weight", "ssl_model.model.feature_extractor.conv_layers.3.2.1.weight",
    "ssl_model.model.post_extract_proj.weight", "ssl_model.model.encoder.pos_conv.0.weight_v", "ssl_model.model.encoder.pos_conv.0.weight_g",
    "ssl_model.model.encoder.layers.0.self_attn.q_proj.weight", "ssl_model.model.encoder.layers.0.self_attn.k_proj.weight",
    "ssl_model.model.encoder.layers.0.self_attn.v_proj.weight", "ssl_model.model.encoder.layers.0.self_attn.out_proj.weight",
    "ssl_model.model.encoder.layers.0.fc1.weight", "ssl_model.model.encoder.layers.0.fc2.weight", "ssl_model.model.encoder.layers.0.fc1.bias",
    "ssl_model.model.encoder.layers.1.fc1.weight", "ssl_model.model.encoder.layers.1.self_attn.q_proj.bias",
    "ssl_model.model.encoder.layers.1.self_attn.out_proj.weight", "ssl_model.model.encoder.layers.1.fc2.weight",
    "ssl_model.model.encoder.layers.1.final_layer_norm.weight", "ssl_model.model.encoder.layer_norm.bias", "LL.weight", "LL.bias",
    "backend.m_frame_level.0.weight", "backend.m_utt_level.weight",
]      # tests/test_model_gpu.py::FULL_SIZE_GRADS with layers 11 and 23 of the 24 mapped to layer 1 of the 2


def test_xlsr_1b_layer_shape_with_lengths_matches_the_oracle(dev, monkeypatch):
    """embed 1280, 16 heads of 80, ffn 5120, final_dim 1024 on the full conv stack, two layers, B = 2 with lengths: the forward at close_bf16
    and one backward at tests/test_model_gpu.py's full-size gradient bars, against the oracle on each utterance alone."""
    monkeypatch.setattr(ML, "DROP_P", 0.0)
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    ref = oracle_alone("xlsr_1b", XLSR_1B_LAYERS, XLSR_1B_LENGTHS, 77)
    m, cfg = model_from(dev, XLSR_1B_LAYERS, ref)
    assert cfg.embed // cfg.heads == 80
    x, ups, T = padded_inputs(cfg, XLSR_1B_LENGTHS, 77)
    m.train()
    step = train_step(m, x, XLSR_1B_LENGTHS, ups, dev)
    d, = m.encoder._vbufs_train.values()
    assert d["long_attn"] and T == 51
    check_outputs(step[:3], ref["outs"], XLSR_1B_LENGTHS, cfg, "XLS-R 1B layers")
    bad = []
    for name in XLSR_1B_GRADS:
        got, r = m.P.g(name).float().cpu().flatten(), ref["grads"][name].flatten()
        e, c = rl2(got, r), cosine(got, r)
        print("grad %-70s rel-L2 %.2e cos %.6f" % (name, e, c))
        lim_e, lim_c = (1.0e-1, 0.995) if name.startswith("backend.m_frame_level") else (6e-2, 0.998)
        if not (e < lim_e and c > lim_c):
            bad.append((name, e, c))
    assert not bad, bad


# ---- 5. main.py --eval --padding_type none with the mapping form of w2v_arch ---------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_eval_padding_type_none_with_a_mapping_for_w2v_arch(dev, tmp_path, monkeypatch):
    """tests/test_varlen_gpu.py's main.py test with `w2v_arch: {...SMALL80}`: five files of different lengths, each file's score equal to the
    file scored alone (that test's 1e-3 of the largest log-probability)."""
    import yaml
    import main as M
    from scl_amd import pack
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
    ref_model = M.MODEL_REGISTRY["wav2vec2_linear_nll"](cfg["model"], dev, seed=5)
    assert ref_model.cfg.embed == 160 and ref_model.cfg.heads == 2 and ref_model.cfg.layers == 2 and ref_model.cfg.conv_dim == 32
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    want = []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            want.append(ref_model(x[None].to(dev), lengths=[n])[0][0].cpu().numpy())
    made = []
    reg = dict(M.MODEL_REGISTRY)
    ctor = reg["wav2vec2_linear_nll"]
    reg["wav2vec2_linear_nll"] = lambda *a, **k: made.append(ctor(*a, **k)) or made[-1]
    monkeypatch.setattr(M, "MODEL_REGISTRY", reg)
    out = tmp_path / "scores.txt"
    assert M.main(["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--eval", "--model_path", str(ck),
                   "--padding_type", "none", "--eval_output", str(out)]) == 0
    lines = out.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for l, ref in zip(lines, want):
        got = np.asarray([float(v) for v in l.split()[1:]])
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-3, (l, ref)
    mm = made[-1]
    assert mm.cfg.embed == 160 and 1 <= len(mm.encoder._vbufs_f32) + len(mm.encoder._vbufs) <= VARLEN_SETS
