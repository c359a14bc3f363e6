"""Variable-length scoring batches on the `wav2vec2_resnet_nll` plugin: the masked BatchNorm and average kernels bit for bit against
their fixed-length neighbours, the back-end alone and the whole plugin (both scoring precisions, both row layouts) against the CPU
oracle run on each utterance ALONE at its own length, the refusals, the bound on staging memory, and main.py --padding_type none."""
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import hipnn  # noqa: E402
from scl_amd import model_front as MF  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import resnet_head as RH  # noqa: E402
from scl_amd.encoder import VARLEN_SETS, W2VConfig  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from scl_amd.model_resnet import Model  # noqa: E402
from oracle import resnet_head as ORH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402

ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "resnet": RH.DEFAULT_RESNET}
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)   # 64-wide heads
NAN = float("nan")


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


# ---- 1. masked BatchNorm + activation ------------------------------------------------------------------------------------------------
def _bn(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g)); bn.bias.copy_(0.3 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(C, generator=g)); bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.to(dev).eval()


@pytest.mark.parametrize("act", [hipnn.ACT_RELU, hipnn.ACT_SELU], ids=["relu", "selu"])
@pytest.mark.parametrize("C", [1, 16, 64])
def test_masked_batch_norm_selects_valid_rows_bit_for_bit_and_zeros_the_rest(dev, C, act):
    B, H, Wd = 4, 9, 16
    valid = [0, 1, 5, 9]
    clean = torch.randn(B, H, Wd, C, generator=torch.Generator().manual_seed(C + act))
    x = clean.clone()
    for b, v in enumerate(valid):
        x[b, v:] = NAN      # rows at or beyond valid[b] must not be interpreted
    bn = _bn(C, dev, 3 * C + act)
    with torch.no_grad():
        want = hipnn.batch_norm(clean.to(dev), bn, act)      # scl_bn_fwd, eval
        got = hipnn.batch_norm(x.to(dev), bn, act, valid=i32(valid, dev))
        full = hipnn.batch_norm(clean.to(dev), bn, act, valid=i32([H] * B, dev))
        torch.cuda.synchronize()
    assert got.shape == want.shape and torch.isfinite(got).all()
    for b, v in enumerate(valid):
        assert torch.equal(got[b, :v], want[b, :v]), (b, v)
        assert (got[b, v:] == 0).all() and not torch.signbit(got[b, v:]).any(), (b, v)
    assert torch.equal(full, want)
    if act == hipnn.ACT_SELU:
        assert (want < 0).any()      # SELU(bn(x)) is not 0 at x = 0: the mask is not implied by zero inputs


def test_masked_batch_norm_refusals(dev):
    bn = _bn(16, dev, 1)
    x = torch.zeros(2, 3, 4, 16, device=dev)
    v = i32([1, 2], dev)
    with pytest.raises(NotImplementedError, match="scoring mode"):
        hipnn.batch_norm(x, bn, hipnn.ACT_RELU, valid=v)      # autograd on
    bn.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
        hipnn.batch_norm(x, bn, hipnn.ACT_RELU, valid=v)      # batch statistics
    bn.eval()
    with torch.no_grad(), pytest.raises(ValueError):
        hipnn.batch_norm(x.view(6, 4, 16), bn, hipnn.ACT_RELU, valid=v)


# ---- 2. masked average ---------------------------------------------------------------------------------------------------------------
def test_masked_average_equals_the_average_of_each_slice_alone(dev):
    B, H, Wd, C = 4, 7, 16, 256
    valid = [1, 2, 7, 4]
    clean = torch.randn(B, H, Wd, C, generator=torch.Generator().manual_seed(5))
    x = clean.clone()
    for b, v in enumerate(valid):
        x[b, v:] = NAN
    with torch.no_grad():
        got = hipnn.avg_pool_rows_masked(x.to(dev), i32(valid, dev), valid)
        for b, v in enumerate(valid):
            alone = hipnn.avg_pool_rows(clean[b:b + 1, :v].reshape(1, v * Wd, C).to(dev))
            assert torch.equal(got[b:b + 1], alone), (b, v)
        with pytest.raises(SclError):
            hipnn.avg_pool_rows_masked(x.to(dev), i32([1, 0, 7, 4], dev), [1, 0, 7, 4])
        with pytest.raises(SclError):
            hipnn.avg_pool_rows_masked(x.to(dev), i32([1, 8, 7, 4], dev), [1, 8, 7, 4])


# ---- 3. the back-end alone -----------------------------------------------------------------------------------------------------------
class _Head(torch.nn.Module):
    """The product back-end under the reference's state-dict names (as the model plugin grafts it), on the GPU."""

    def __init__(self, cfg):
        super().__init__()
        for n, c in RH.ResNetHead(cfg).named_children():
            self.add_module(n, c)

    def forward(self, feats, frames=None):
        return RH.ResNetHead.forward(self, feats, frames)


def _filled_head(dev, cfg, seed):
    m = _Head(cfg)
    filled = {k: torch.from_numpy(v) for k, v in fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed).items()}
    m.load_state_dict(filled)
    return m.to(dev).eval(), filled


@pytest.mark.parametrize("resnet_type,frames", [("18", [55, 78, 79, 103, 130]), ("50", [55, 79, 103])])
def test_head_on_a_padded_batch_matches_the_oracle_on_each_utterance_alone(dev, monkeypatch, resnet_type, frames):
    """Odd and even row counts into every stride-2 stage and the one-row conv5 output; NaN in the padded feats rows.  The bar is
    tests/test_resnet_gpu.py's for the exact-fp32 convolutions: 2e-4 of the reference tensor's largest magnitude."""
    monkeypatch.setenv("SCL_RESNET_CONV", "f32")
    m, filled = _filled_head(dev, dict(RH.DEFAULT_RESNET, resnet_type=resnet_type), 7)
    B, T = len(frames), max(frames)
    clean = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(13))
    feats = clean.clone()
    for b, n in enumerate(frames):
        feats[b, n:] = NAN
    with torch.no_grad():
        out, emb = m(feats.to(dev), frames)
        torch.cuda.synchronize()
        assert out.shape == (B, 2) and emb.shape == (B, 256) and torch.isfinite(out).all() and torch.isfinite(emb).all()
        for b, n in enumerate(frames):
            ro, re = ORH.forward(filled, clean[b:b + 1, :n], False)
            go, ge = m(clean[b:b + 1, :n].to(dev))      # the GPU head on the utterance alone
            e_o, e_e = maxrel(out[b], ro[0]), maxrel(emb[b], re[0])
            print("resnet %s, %d frames: against the oracle alone logits %.2e emb %.2e | against the GPU head alone logits %.2e emb %.2e"
                  % (resnet_type, n, e_o, e_e, maxrel(out[b], go[0]), maxrel(emb[b], ge[0])))
            assert e_o < 2e-4 and e_e < 2e-4, (n, e_o, e_e)
        # every row full, clean feats: the bits of the fixed-length forward
        full_o, full_e = m(clean.to(dev), [T] * B)
        want_o, want_e = m(clean.to(dev))
        assert torch.equal(full_o, want_o) and torch.equal(full_e, want_e)


def test_head_refusals(dev):
    m, _ = _filled_head(dev, RH.DEFAULT_RESNET, 7)
    feats = torch.zeros(2, 60, 128, device=dev)
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(feats, [60, 55])      # autograd on
    with torch.no_grad():
        with pytest.raises(ValueError, match="at least 55 frames"):
            m(feats, [60, 54])
        with pytest.raises(ValueError):
            m(feats, [60, 61])
        with pytest.raises(ValueError):
            m(feats, [60])


# ---- 4 / 5. the plugin ---------------------------------------------------------------------------------------------------------------
class CpuRef(torch.nn.Module):
    """oracle encoder state + LL + the oracle head (functional forward over the reference's state-dict names) on the CPU."""

    def __init__(self, ssl_sd, cfg, head_sd):
        super().__init__()
        self.cfg = cfg
        self.ssl = {k: v.clone() for k, v in ssl_sd.items()}
        self.LL = torch.nn.Linear(cfg.embed, 128)
        tree = ORH.ParamTree({k: tuple(v.shape) for k, v in head_sd.items() if not k.startswith("LL.")})
        for n, c in tree.named_children():
            self.add_module(n, c)
        self.load_state_dict(head_sd)
        self.eval()

    def alone(self, x):
        """(logits, feats, emb) of one utterance [1, n] at its own length."""
        t = dict(self.named_parameters()); t.update(dict(self.named_buffers()))
        with torch.no_grad():
            rf = self.LL(W.forward(self.ssl, self.cfg, x))
            ro, re = ORH.forward(t, rf, False)
        return ro, rf, re


_CACHE = {}


def _setup(dev, small, counts, seed):
    """The plugin on the tiny preset (or the 64-wide-head SMALL config), the zero-padded batch and the CPU chain's result for every
    utterance alone; built once per (config, batch) and left unchanged."""
    key = (small, tuple(counts))
    if key not in _CACHE:
        ocfg = W.W2VConfig(**SMALL) if small else W.W2VConfig.tiny()
        ssl = W.init_state(ocfg, seed=seed)
        m = Model(ARGS, dev, w2v_cfg=W2VConfig(**SMALL) if small else W2VConfig.tiny())
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("ssl_model.")}
        head_sd = {k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=seed + 1).items()}
        sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
        sd.update(head_sd)
        m.load_state_dict(sd)
        m.eval()
        ref = CpuRef(ssl, ocfg, head_sd)
        gen = torch.Generator().manual_seed(len(counts) + seed)
        L = max(48000, max(counts)) if len(counts) == 5 else max(counts)
        x = torch.zeros(len(counts), L)
        refs = []
        for b, n in enumerate(counts):
            x[b, :n] = 0.1 * torch.randn(n, generator=gen)
            refs.append(ref.alone(x[b:b + 1, :n].clone()))
        _CACHE[key] = (m, x, refs)
    return _CACHE[key]


COUNTS = [17680, 18000, 25500, 33040, 41680]      # 55, 56, 79, 103 and 130 frames in a [5, 48000] batch: every row has padding
LONG = [170000, 17680, 90000]                     # 531 frames (beyond 512), 55 and 281: 175 / 17 / 92 conv1 rows


def _alone_on_gpu(m, x, counts, dev):
    with torch.no_grad():
        return [tuple(t.clone() for t in m(x[b:b + 1, :n].to(dev))) for b, n in enumerate(counts)]


def test_fp32_scoring_of_a_padded_batch(dev, monkeypatch):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    m, x, refs = _setup(dev, False, COUNTS, 91)
    assert x.shape == (5, 48000) and m.min_samples() == 17680
    cfg = m.cfg
    with torch.no_grad():
        out, feats, emb = m(x.to(dev), lengths=COUNTS)
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, COUNTS, dev)
    assert emb.shape == (5, 256) and feats.shape == (5, cfg.conv_lens(48000)[-1], 128)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = refs[b]
        assert rf.shape[1] == Tb and (feats[b, Tb:] == 0).all()
        e = (rl2(feats[b, :Tb], rf[0]), rl2(emb[b], re[0]), rl2(out[b], ro[0]))
        go, gf, ge = alone[b]
        g = (maxrel(out[b], go[0]), maxrel(emb[b], ge[0]), maxrel(feats[b, :Tb], gf[0]))
        print("fp32 n=%d (%d frames): rel-L2 against the CPU chain alone feats %.2e emb %.2e logits %.2e | max-rel against the GPU alone "
              "logits %.2e emb %.2e feats %.2e" % ((n, Tb) + e + g))
        assert e[0] < 1e-2 and e[1] < 3e-2 and e[2] < 3e-2, (n, e)
        assert max(g) < 1e-3, (n, g)


@pytest.mark.parametrize("counts", [COUNTS, LONG], ids=["five", "beyond512"])
def test_fp32_scoring_on_packed_rows_agrees_with_the_padded_layout(dev, monkeypatch, counts):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    m, x, refs = _setup(dev, True, counts, 93)
    cfg = m.cfg
    res = {}
    for pack in (False, True):
        monkeypatch.setattr(ENC, "SCORE_PACK", pack)
        with torch.no_grad():
            res[pack] = tuple(t.clone() for t in m(x.to(dev), lengths=counts))
            torch.cuda.synchronize()
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    alone = _alone_on_gpu(m, x, counts, dev)
    if counts is LONG:
        assert cfg.conv_lens(x.shape[1])[-1] == 531 and RH.batch_rows([cfg.conv_lens(n)[-1] for n in counts])[1] == [175, 17, 92]
    for b, n in enumerate(counts):
        Tb = cfg.conv_lens(n)[-1]
        for pack in (False, True):
            out, feats, emb = res[pack]
            assert (feats[b, Tb:] == 0).all()
            go, gf, ge = alone[b]
            g = (maxrel(out[b], go[0]), maxrel(emb[b], ge[0]), maxrel(feats[b, :Tb], gf[0]))
            print("fp32 %s n=%d (%d frames): max-rel against the GPU alone logits %.2e emb %.2e feats %.2e"
                  % ("packed" if pack else "padded", n, Tb, g[0], g[1], g[2]))
            assert max(g) < 1e-3, (pack, n, g)
        p = tuple(maxrel(res[True][i][b], res[False][i][b]) for i in range(3))
        print("      packed against padded: logits %.2e feats %.2e emb %.2e" % p)
        assert max(p) < 1e-3, (n, p)


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_bf16_scoring_of_a_padded_batch(dev, monkeypatch, pack):
    """SCL_SCORE_FP32=0: the bf16 encoder kernels with the padding mask (and SCL_VARLEN_PACK).  Per tensor the bar is the larger of
    tests/test_resnet_gpu.py's (rel-L2 1e-2 feats, 3e-2 emb and logits) and twice the error the fixed-length bf16 path makes on the same
    utterance alone, both against the CPU chain on that utterance alone."""
    monkeypatch.setattr(MF, "SCORE_FP32", False); monkeypatch.setattr(ML, "SCORE_FP32", False)
    monkeypatch.setattr(ENC, "VARLEN_PACK", pack)
    m, x, refs = _setup(dev, True, COUNTS, 93)
    cfg = m.cfg
    with torch.no_grad():
        out, feats, emb = (t.clone() for t in m(x.to(dev), lengths=COUNTS))
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, COUNTS, dev)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = refs[b]
        assert (feats[b, Tb:] == 0).all()
        go, gf, ge = alone[b]
        for name, got, fixed, ref, floor in (("feats", feats[b, :Tb], gf[0], rf[0], 1e-2), ("emb", emb[b], ge[0], re[0], 3e-2),
                                             ("logits", out[b], go[0], ro[0], 3e-2)):
            err, base = rl2(got, ref), rl2(fixed, ref)
            print("bf16 %s n=%d (%d frames) %s: rel-L2 %.2e, the fixed-length path alone %.2e, bar %.2e"
                  % ("packed" if pack else "padded", n, Tb, name, err, base, max(floor, 2 * base)))
            assert err < max(floor, 2 * base), (name, n, err, base)
    # the recorded plan reads the counts from the state's buffers: a replay with other lengths follows them
    other = [COUNTS[-1 - b] for b in range(len(COUNTS))]
    with torch.no_grad():
        o2, f2, e2 = (t.clone() for t in m(x.to(dev), lengths=other))
        o3, f3, e3 = m(x.to(dev), lengths=COUNTS)
        torch.cuda.synchronize()
    assert torch.equal(o3, out) and torch.equal(e3, emb) and torch.equal(f3, feats)
    assert not torch.equal(e2, emb)
    for b, n in enumerate(other):
        Tb = cfg.conv_lens(n)[-1]
        assert (f2[b, Tb:] == 0).all() and (f2[b, Tb - 1] != 0).any()
    assert ((5, 48000, "packed") if pack else (5, 48000)) in m._vstates and len(m._vstates) <= VARLEN_SETS      # a state per layout of the shape


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, monkeypatch):
    from scl_amd.model_aasist import Model as Aasist
    m, x, _ = _setup(dev, False, COUNTS, 91)
    xs = x[:2].to(dev)
    ok = [20000, 17680]
    m.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(xs, lengths=ok)      # autograd on
    m.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
            m(xs, lengths=ok)
    finally:
        m.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="17680"):
            m(xs, lengths=[20000, 17679])
        for bad in ([20000], [20000, 0], [20000, 48001], [20000, 17680, 17680]):
            with pytest.raises(ValueError, match="lengths"):
                m(xs, lengths=bad)
        m(xs, lengths=ok)
    a = Aasist({"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}, dev, w2v_cfg=W2VConfig.tiny())
    a.eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="wav2vec2_linear_nll"):
        a(xs, lengths=ok)


# ---- 7. staging memory ---------------------------------------------------------------------------------------------------------------
def _staging_bytes(m, B, T):
    """Bytes of the zero-bordered staging maps of one [B, T, 128] batch through the ResNet-18 back-end (f32 operands: channels rounded up
    to 4, 4096 elements of slack per map), from the geometry alone."""
    rows = RH.layer_rows(T, m.resnet.resnet_type, m.resnet.num_nodes)
    maps = [(rows[0], 1, 1)]      # (input rows, input channels, row padding); every convolution but the 1x1 pads the width by 1
    for s in (1, 2, 3, 4):
        for j, blk in enumerate(getattr(m.resnet, "layer%d" % s).children()):
            hin, cin = rows[s if j == 0 else s + 1], blk.conv1.weight.shape[1]
            maps += [(hin, cin, 1), (rows[s + 1], blk.conv2.weight.shape[1], 1)]
            if hasattr(blk, "shortcut"):
                maps.append((hin, cin, 0))
    maps.append((rows[5], m.resnet.conv5.weight.shape[1], 0))
    return sum(4 * (B * (h + 2 * p) * (128 + 2) * ((c + 3) // 4 * 4) + 4096) for h, c, p in maps)


def test_staging_memory_stays_bounded_over_many_padded_lengths(dev, monkeypatch):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    m, _, _ = _setup(dev, False, COUNTS, 91)
    lens = [32000 + 16000 * i for i in range(12)]
    gen = torch.Generator().manual_seed(3)
    mark = None
    pooled = sum(len(v) for v in hipnn._ZERO_POOL.values())
    with torch.no_grad():
        for i, L in enumerate(lens + lens[:4]):
            x = torch.zeros(2, L)
            x[0] = 0.1 * torch.randn(L, generator=gen); x[1, :L - 9000] = 0.1 * torch.randn(L - 9000, generator=gen)
            out = m(x.to(dev), lengths=[L, L - 9000])
            torch.cuda.synchronize()
            assert torch.isfinite(out[0]).all()
            del out, x
            if i == 3:
                mark = torch.cuda.memory_allocated()
            assert len(m._vstates) <= VARLEN_SETS and len(m.ssl._vbufs_f32) <= VARLEN_SETS and len(m.ssl._vbufs) <= VARLEN_SETS
        last = torch.cuda.memory_allocated()
    allowance = _staging_bytes(m, 2, m.cfg.conv_lens(lens[-1])[-1])
    print("allocated after the fourth batch %d, after the last %d, staging of the largest batch %d" % (mark, last, allowance))
    assert last - mark <= allowance
    assert sum(len(v) for v in hipnn._ZERO_POOL.values()) == pooled      # no staging map of these shapes stays in the per-geometry pool


# ---- 8. main.py --eval --padding_type none -------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_eval_padding_type_none_with_the_resnet_plugin(dev, tmp_path, monkeypatch):
    import yaml
    import main as M
    from scl_amd import pack
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    sizes = [3000, 20000, 33333, 64600, 70000]
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(root / u), 0.1 * rs.randn(n))
    (root / "protocol.txt").write_text("".join("%s eval bonafide\n" % u for u in ids))
    cfg = {"model": {"name": "wav2vec2_resnet_nll", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ref_model = M.MODEL_REGISTRY["wav2vec2_resnet_nll"](cfg["model"], dev, seed=5)
    # default BatchNorm buffers make a dull back-end: fill its state as the other tests do
    shapes = {k: tuple(v.shape) for k, v in ref_model.state_dict().items() if not k.startswith("ssl_model.")}
    ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=6).items()}, strict=False)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    assert ref_model.min_samples() == 17680
    want_lp, want_emb = [], []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            if n < 17680:      # the data path zero-pads a shorter file to the model's minimum
                x = torch.cat([x, torch.zeros(17680 - n)])
            o, _, e = ref_model(x[None].to(dev))      # each file alone at its own length
            want_lp.append(o[0].cpu().numpy()); want_emb.append(e[0].cpu().numpy())
    assert want_emb[0].shape == (256,)
    common = ["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--eval", "--model_path", str(ck),
              "--padding_type", "none"]
    relerr = lambda got, ref: np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()
    out = tmp_path / "scores.txt"
    assert M.main(common + ["--eval_output", str(out)]) == 0
    lines = out.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids      # exactly five lines, protocol order, the 3000-sample file included
    for l, ref in zip(lines, want_lp):
        assert relerr([float(v) for v in l.split()[1:]], ref) < 1e-3, (l, ref)
    pred = tmp_path / "pred.txt"
    assert M.main(common + ["--predict", "--eval_output", str(pred)]) == 0
    lines = pred.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for l, ref in zip(lines, want_lp):
        assert abs(float(l.split()[1]) - ref[1]) <= 1e-3 * np.abs(ref).max() and int(l.split()[2]) == int(ref.argmax())
    embd = tmp_path / "emb"
    assert M.main(common + ["--emb", "--eval_output", str(embd)]) == 0
    lines = (embd / "scores.txt").read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for u, ref in zip(ids, want_emb):
        got = np.load(str(embd / (u.split(".")[0] + ".npy")))
        assert got.shape[-1] == 256 and relerr(got, ref) < 1e-3, u
