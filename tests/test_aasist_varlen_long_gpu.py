"""Variable-length scoring beyond 242 frames on the `wav2vec2_aasist` plugin (SCL_AASIST_LENGTHS=long): the back-end
(AasistHead.forward_frames_long) against the product's fixed-length forward and the fp64 oracle on each utterance alone, the whole plugin
(both scoring precisions, packed rows) against itself on each utterance alone, and main.py --eval --padding_type none with files beyond
77,839 samples.  Modelled on tests/test_aasist_varlen_gpu.py, whose bounds these are.

Back-end bars.  Against the fixed-length forward alone: 2e-5 of the largest magnitude (that file's TOL).  Against the fp64 oracle: 2e-5 or
1.5 x the error the fixed-length forward on that utterance has against the same oracle, whichever is larger; the test prints both per
utterance.  Measured on the MI355X:
    frames   against the fixed-length forward   against the fp64 oracle   the fixed-length forward against the oracle
    243      9.1e-7                             5.1e-7                    7.1e-7
    282      1.9e-7                             4.6e-7                    5.3e-7
    283      3.0e-7                             4.9e-7                    6.3e-7
    387      4.7e-7                             4.3e-7                    3.9e-7
    390      5.0e-7                             1.1e-6                    1.6e-6
    773      4.1e-7                             9.4e-7                    6.3e-7
    776      3.9e-7                             7.5e-7                    5.0e-7
    100      7.3e-7                             7.2e-7                    7.6e-7
    3        8.8e-7                             6.2e-7                    7.3e-7
so 1.5 x the fixed-length forward's error is below 2e-5 everywhere and the bar in force is 2e-5; the GraphPool gap of the batch is 1.01e-5.
Plugin: fp32 <= 2.3e-6 padded, <= 4.9e-6 packed (bar 1e-3); bf16 within 1.25 x the fixed-length bf16 path's own error on every tensor."""
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import aasist_head as AH  # noqa: E402
from scl_amd import aasist_long as AL  # noqa: E402
from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_front as MF  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.model_aasist import Model  # noqa: E402
from oracle import aasist_head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402

NAN = float("nan")
TOL = 2e-5
# 243: first beyond the fused graph (81 nodes); 282 / 283: first beyond the fused stack (94 columns, 3 W and 3 W + 1); 387 / 390: first beyond
# the whole-graph pair kernel (129 / 130 nodes); 773 / 776: three j tiles (257 / 258), heterogeneous layers of 149 / 150 nodes with
# n1 = 128 / 129; 100 and 3: short rows riding along
FRAMES = [243, 282, 283, 387, 390, 773, 776, 100, 3]
T_PAD = 800
SEED = 110      # the fp64 GraphPool gap of this batch: 1.0e-5 (seeds 101..112 range from 4.6e-7 to 1.0e-5)
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)   # 64-wide heads
ARGS = {"contra_mode": "all", "loss_type": 1, "aasist": AH.UPSTREAM_AASIST}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


# ---- the back-end -------------------------------------------------------------------------------------------------------------------------
def _pool_gaps(ref, feats):
    """Every GraphPool of the fp64 oracle on one utterance: the gap between the last kept and the first dropped score."""
    gaps, hooks = [], []

    def hook(mod, inp, out):
        s = torch.sigmoid(mod.proj(inp[0]))[0, :, 0].sort(descending=True)[0]
        keep = max(int(s.shape[0] * mod.k), 1)
        if keep < s.shape[0]:
            gaps.append((s[keep - 1] - s[keep]).item())
    for m in ref.modules():
        if isinstance(m, OH.GraphPool):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        out = ref(feats)
    for h in hooks:
        h.remove()
    return out, min(gaps)


@pytest.fixture(scope="module")
def backend_case(dev):
    head = AH.AasistHead()
    sd = fill_state({k: tuple(v.shape) for k, v in head.state_dict().items()}, seed=3)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    head = head.to(dev).eval()
    ref = OH.AasistHead().double().eval()
    ref.load_state_dict({k: torch.from_numpy(v).to(ref.state_dict()[k].dtype) for k, v in sd.items()})
    gen = torch.Generator().manual_seed(SEED)
    feats = torch.zeros(len(FRAMES), T_PAD, 128)
    for b, n in enumerate(FRAMES):
        feats[b, :n] = torch.randn(n, 128, generator=gen)
    refs, gap = [], 1.0
    for b, n in enumerate(FRAMES):
        out, g = _pool_gaps(ref, feats[b:b + 1, :n].double())
        refs.append(out)
        gap = min(gap, g)
    return head, feats, refs, gap


def test_forward_frames_long_against_the_fixed_length_forward_and_the_fp64_oracle(dev, backend_case):
    head, feats, refs, gap = backend_case
    print("smallest gap between a kept and a dropped GraphPool score (fp64): %.2e" % gap)
    assert gap >= 2e-6      # precondition: top-k is discontinuous, a closer gap cannot be compared across precisions (change SEED, not the batch)
    fd = feats.to(dev)
    with torch.no_grad():
        lo, hid = (t.clone() for t in head.forward_frames_long(fd, FRAMES))
        torch.cuda.synchronize()
        assert lo.shape == (len(FRAMES), 2) and hid.shape == (len(FRAMES), 160) and torch.isfinite(lo).all() and torch.isfinite(hid).all()
        fails = []
        for b, n in enumerate(FRAMES):
            fl, fh = head(fd[b:b + 1, :n].contiguous())      # the product's fixed-length forward on the utterance alone
            ef = max(maxrel(lo[b], fl[0]), maxrel(hid[b], fh[0]))
            eo = max(maxrel(lo[b], refs[b][0][0]), maxrel(hid[b], refs[b][1][0]))
            base = max(maxrel(fl[0], refs[b][0][0]), maxrel(fh[0], refs[b][1][0]))      # the fixed-length forward against the same oracle
            bar = max(TOL, 1.5 * base)
            print("%3d frames: against the fixed-length forward %.2e (bar %.0e); against the fp64 oracle %.2e, the fixed-length forward %.2e, bar %.2e"
                  % (n, ef, TOL, eo, base, bar))
            if ef > TOL or eo > bar:
                fails.append((n, ef, eo, bar))
        assert not fails, fails
        # NaN in the padded rows of feats: not a bit changes
        fn = fd.clone()
        for b, n in enumerate(FRAMES):
            fn[b, n:] = NAN
        lo2, hid2 = head.forward_frames_long(fn, FRAMES)
        assert torch.equal(lo2, lo) and torch.equal(hid2, hid)
        # the batch reversed gives the results reversed
        lo4, hid4 = head.forward_frames_long(fd.flip(0).contiguous(), FRAMES[::-1])
        assert torch.equal(lo4, lo.flip(0)) and torch.equal(hid4, hid.flip(0))


def test_a_short_batch_under_long_takes_the_fused_kernels_bit_for_bit(dev, backend_case, monkeypatch):
    head, feats = backend_case[0], backend_case[1]
    frames = [242, 100]
    fd = torch.zeros(2, 320, 128)
    fd[0, :242], fd[1, :100] = feats[5, :242], feats[7, :100]
    fd = fd.to(dev)
    with torch.no_grad():
        monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
        want = tuple(t.clone() for t in Model._head_forward(head, fd, frames))
        monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
        got = tuple(t.clone() for t in Model._head_forward(head, fd, frames))
        fused = tuple(t.clone() for t in head.forward_frames(fd, frames))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[0], fused[0]) and torch.equal(got[1], fused[1])


# ---- the plugin ---------------------------------------------------------------------------------------------------------------------------
class CpuRef(torch.nn.Module):
    """oracle encoder + LL + the oracle head on the CPU, one utterance at its own length (tests/test_aasist_varlen_gpu.py)."""

    def __init__(self, ssl_sd, cfg, head_sd):
        super().__init__()
        self.cfg = cfg
        self.ssl = {k: v.clone() for k, v in ssl_sd.items()}
        self.LL = torch.nn.Linear(cfg.embed, 128)
        head = OH.AasistHead(AH.UPSTREAM_AASIST)
        for n, c in head.named_children():
            self.add_module(n, c)
        for n in ("pos_S", "master1", "master2"):
            self.register_parameter(n, getattr(head, n))
        self.load_state_dict(head_sd)
        self.eval()

    def alone(self, x):
        with torch.no_grad():
            rf = self.LL(W.forward(self.ssl, self.cfg, x))
            ro, rh = OH.AasistHead.forward(self, rf)
        return ro, rf, rh


COUNTS = [77840, 123920, 20000, 1040]      # 243, 387, 62 and 3 frames in a [4, 125000] batch
_CACHE = {}


def _setup(dev, seed=93):
    if "m" not in _CACHE:
        ocfg = W.W2VConfig(**SMALL)
        ssl = W.init_state(ocfg, seed=seed)
        m = Model(ARGS, dev, w2v_cfg=W2VConfig(**SMALL))
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("ssl_model.")}
        head_sd = {k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=seed + 1).items()}
        sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
        sd.update(head_sd)
        m.load_state_dict(sd)
        m.eval()
        gen = torch.Generator().manual_seed(seed)
        x = torch.zeros(len(COUNTS), 125000)
        for b, n in enumerate(COUNTS):
            x[b, :n] = 0.1 * torch.randn(n, generator=gen)
        _CACHE["m"] = (m, x, CpuRef(ssl, ocfg, head_sd))
    return _CACHE["m"]


def _alone_on_gpu(m, x, dev):
    with torch.no_grad():
        return [tuple(t.clone() for t in m(x[b:b + 1, :n].to(dev))) for b, n in enumerate(COUNTS)]


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_fp32_scoring_of_a_batch_with_utterances_beyond_242_frames(dev, monkeypatch, pack):
    """tests/test_aasist_varlen_gpu.py's fp32 plugin bar: 1e-3 of the largest magnitude against the model on each utterance alone."""
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", pack)
    m, x, _ = _setup(dev)
    cfg = m.cfg
    assert [cfg.conv_lens(n)[-1] for n in COUNTS] == [243, 387, 62, 3]
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")
    with torch.no_grad(), pytest.raises(ValueError, match="77839"):      # the parent's limit, still the limit of =1
        m(x.to(dev), lengths=COUNTS)
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
    assert m.head_takes_frames and m.min_samples() == 1040 and m.max_samples() == 960000 and m.head_max_frames() == 3074
    with torch.no_grad():
        out, feats, hid = (t.clone() for t in m(x.to(dev), lengths=COUNTS))
        torch.cuda.synchronize()
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    alone = _alone_on_gpu(m, x, dev)
    assert hid.shape == (4, 160) and feats.shape == (4, cfg.conv_lens(125000)[-1], 128)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        assert (feats[b, Tb:] == 0).all() and (feats[b, Tb - 1] != 0).any()
        go, gf, gh = alone[b]
        g = (maxrel(out[b], go[0]), maxrel(hid[b], gh[0]), maxrel(feats[b, :Tb], gf[0]))
        print("fp32 %s n=%d (%d frames): max-rel against the GPU alone logits %.2e hidden %.2e feats %.2e" % (("packed" if pack else "padded", n, Tb) + g))
        assert max(g) < 1e-3, (n, g)


def test_bf16_scoring_of_a_batch_with_utterances_beyond_242_frames(dev, monkeypatch):
    """tests/test_aasist_varlen_gpu.py's bf16 plugin bar: per tensor the larger of the bf16 floor (rel-L2 1e-2 feats, 3e-2 hidden and logits)
    and twice the error the fixed-length bf16 path makes on the same utterance alone, both against the CPU chain on that utterance alone."""
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
    monkeypatch.setattr(MF, "SCORE_FP32", False); monkeypatch.setattr(ML, "SCORE_FP32", False)
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    m, x, ref = _setup(dev)
    cfg = m.cfg
    with torch.no_grad():
        out, feats, hid = (t.clone() for t in m(x.to(dev), lengths=COUNTS))
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, dev)
    for b, n in enumerate(COUNTS):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, rh = ref.alone(x[b:b + 1, :n].clone())
        assert (feats[b, Tb:] == 0).all()
        go, gf, gh = alone[b]
        for name, got, fixed, want, floor in (("feats", feats[b, :Tb], gf[0], rf[0], 1e-2), ("hidden", hid[b], gh[0], rh[0], 3e-2),
                                              ("logits", out[b], go[0], ro[0], 3e-2)):
            err, base = rl2(got, want), rl2(fixed, want)
            print("bf16 n=%d (%d frames) %s: rel-L2 %.2e, the fixed-length path alone %.2e, bar %.2e" % (n, Tb, name, err, base, max(floor, 2 * base)))
            assert err < max(floor, 2 * base), (name, n, err, base)


def test_plugin_refusals_under_long(dev, monkeypatch):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
    m, x, _ = _setup(dev)
    xs = x[:2].to(dev)
    ok = COUNTS[:2]
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(xs, lengths=ok)      # autograd on
    m.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
            m(xs, lengths=ok)
    finally:
        m.eval()
    with torch.no_grad():
        monkeypatch.setattr(AH, "FUSED_STACK", False)      # SCL_AASIST_FUSED=0: the long path does not depend on it ...
        assert torch.isfinite(m(xs, lengths=ok)[0]).all()
        with pytest.raises(NotImplementedError, match="SCL_AASIST_FUSED=0"):      # ... a short batch still runs on the fused kernels only
            m(xs, lengths=[20000, 64000])
        monkeypatch.setattr(AH, "FUSED_STACK", True)


# ---- main.py --eval --padding_type none ---------------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_eval_padding_type_none_scores_whole_files_beyond_77839_samples(dev, tmp_path, monkeypatch, capsys):
    import yaml
    import main as M
    from scl_amd import pack
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    sizes = [700, 20000, 90000, 130000]      # one below min_samples() = 1040, two beyond the 77,839 samples of SCL_AASIST_LENGTHS=1
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(root / u), 0.1 * rs.randn(n))
    (root / "protocol.txt").write_text("".join("%s eval bonafide\n" % u for u in ids))
    cfg = {"model": {"name": "wav2vec2_aasist", "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"}, "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ref_model = M.MODEL_REGISTRY["wav2vec2_aasist"](cfg["model"], dev, seed=5)
    shapes = {k: tuple(v.shape) for k, v in ref_model.state_dict().items() if not k.startswith("ssl_model.")}
    ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=6).items()}, strict=False)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "long")
    lo, hi = ref_model.min_samples(), ref_model.max_samples()
    assert (lo, hi) == (1040, 960000)
    want = []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            x = torch.cat([x, torch.zeros(lo - n)]) if n < lo else x      # the data path pads to the minimum; nothing is cut
            want.append(ref_model(x[None].to(dev))[0][0].cpu().numpy())      # each file alone, whole
    common = ["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "4", "--eval", "--model_path", str(ck), "--padding_type", "none"]
    relerr = lambda got, ref: np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()
    out = tmp_path / "scores.txt"
    capsys.readouterr()
    assert M.main(common + ["--eval_output", str(out)]) == 0
    assert "4 utterances, 0 cut" in capsys.readouterr().out
    lines = out.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for l, ref in zip(lines, want):
        assert relerr([float(v) for v in l.split()[1:]], ref) < 1e-3, (l, ref)
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")      # the same files under =1: two are cut, as before
    capsys.readouterr()
    assert M.main(common + ["--eval_output", str(tmp_path / "cut.txt")]) == 0
    assert "4 utterances, 2 cut to 77839 samples" in capsys.readouterr().out
