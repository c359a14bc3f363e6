"""The AASIST back-end and the three non-linear plugins on clips beyond 512 frames.

Back-end: AasistHead against oracle.aasist_head.AasistHead in float64 on the CPU at 513 frames (171 temporal nodes; heterogeneous layers of
106 and 52 nodes) and 780 frames (260 temporal nodes; 151 and 75), train mode (dropout p = 0) and eval mode, two steps, with the machinery and
the bars (BARS_AASIST) of tests/test_backends_train_gpu.py.  At these sizes the head runs the per-layer composition (graph_unfused over
Residual_block.run, hipnn and gat_score): graph.supported and resstack.supported are asserted false, and no fused plan may appear.  The pair
scores of the 171-, 260- and 151-node layers are the tiled kernels of csrc/gat.hip.

Where a tensor misses its BARS_AASIST bar, the same oracle run in fp32 on the CPU is compared with float64 on the same inputs, and that
tensor's bar is 3 x the oracle's own fp32 error; every such case is printed with both values.  Measured on the MI355X, worst over the four
cases and both steps (bar): out 1.9e-6 (3e-6), out-max 2.0e-6 (5e-6), grad_x 2.1e-4 (3e-4), grad 6.5e-4 (1e-3; first_bn1.bias, T = 513 train
step 1), grad-scalar 2.8e-4 (5e-2), buffer 2.1e-7 (2e-6), zero-grad 9.3e-8 (2e-6): every tensor holds its BARS_AASIST bar, none is on the
fp32-oracle bar.

Preconditions, asserted: every GraphPool top-k margin above TOPK_MARGIN in float64 (the seeds below were checked on the CPU).

Plugins: wav2vec2_aasist and wav2vec2_resnet_nll at 2 x 164,240 samples (513 frames), with the comparisons and bars their own test files use
at short clips (tests/test_aasist_gpu.py, test_resnet_gpu.py; the train steps on 4 clips, see TRAIN_LABELS); the encoder is the two-layer one with 64-wide
heads (W2VConfig.tiny() where its 16-wide heads can run 513 frames: fp32 scoring; see SMALL below)."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402
from oracle.aasist_head import AasistHead as OracleAasist  # noqa: E402
from scl_amd import graph, resstack  # noqa: E402
from scl_amd import model_front as MF  # noqa: E402
from scl_amd.aasist_head import UPSTREAM_AASIST, AasistHead, node_counts  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.optim import FusedAdamW  # noqa: E402
from test_aasist_cpu import analytically_zero  # noqa: E402
from test_backends_train_gpu import (BARS_AASIST, TOPK_MARGIN, Report, calibrate, compare_buffers, compare_params, fill, labels, set_mode,  # noqa: E402
                                     topk_margins, upstream, batch_counts, maxrel, rl2 as rl2_64)
import test_aasist_gpu as TA  # noqa: E402
import test_resnet_gpu as TR  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLES = 164240      # 513 frames
FP32_FACTOR = 3.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the back-end against float64 ---------------------------------------------------------------------------------------------------------
# (B, T, training) -> seed of the weights; inputs are seeded from (step, B, T).  Chosen so that every top-k margin holds in float64.
HEAD_CASES = [(2, 513, True), (2, 513, False), (2, 780, True), (2, 780, False)]
HEAD_SEEDS = {(2, 513, True): 1003, (2, 513, False): 1002, (2, 780, True): 1002, (2, 780, False): 1003}      # float64 margins 2.0e-4 .. 2.5e-3


def head_input(step, B, T):
    return torch.randn(B, T, 128, generator=torch.Generator().manual_seed(7919 * step + B + T))


def make_reference(B, T, training):
    ref = OracleAasist(UPSTREAM_AASIST).double()
    ref.load_state_dict(fill(ref, seed=HEAD_SEEDS[(B, T, training)]))
    if not training:
        calibrate(ref, torch.randn(B, T, 128, generator=torch.Generator().manual_seed(31 + B + T)).double())
    set_mode((ref,), training)
    return ref


def reference_step(ref, x, y, dtype=torch.float64, grads=None):
    """One forward + backward of the oracle in `dtype`; the upstream gradient is the float64 loss's (`grads`), or computed here."""
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    margins = []
    hooks = topk_margins(ref, margins)
    ro, rh = ref(xr)
    for h in hooks:
        h.remove()
    if grads is None:
        grads = upstream(ro, rh, xr, y, 1.0)
    torch.autograd.backward([ro, rh], [g.to(dtype) for g in grads])
    return xr, ro, rh, grads, margins


class Fp32Floor(Report):
    """Report whose bar for a tensor that misses its BARS_AASIST bar is FP32_FACTOR x what the oracle itself loses on that tensor in fp32 on
    the CPU.  record=True: the pass that stores the oracle's fp32 errors under the same (step, kind, name) keys."""

    def __init__(self, tag, bars):
        super().__init__(tag, bars)
        self.floor, self.record, self.widened = {}, False, []

    def check(self, kind, name, value):
        key = (self.step, kind, name)
        if self.record:
            self.floor[key] = value
            return
        f = self.floor.get(key)
        if value == value and value >= self.bars[kind] and f is not None and value < FP32_FACTOR * f:
            self.widened.append("%s step %d %s: %.3e >= %.0e, oracle fp32 %.3e, bar %.3e" % (kind, self.step, name, value, self.bars[kind], f, FP32_FACTOR * f))
            return
        super().check(kind, name, value)

    def done(self):
        if self.widened:
            print("\n[%s] on the fp32-oracle bar:\n  %s" % (self.tag, "\n  ".join(self.widened)))
        super().done()


def compare_all(rep, out, hid, xin, params, module, ro, rh, xr, rparams, ref, training, nbt0, steps):
    for name, g, r in (("logits", out, ro), ("hidden", hid, rh)):
        rep.check("out", name, rl2_64(g, r))
        rep.check("out-max", name, maxrel(g, r))
    rep.check("grad_x", "input", rl2_64(xin.grad, xr.grad))
    n = compare_params(rep, params, rparams, training, analytically_zero)
    compare_buffers(rep, module, ref, nbt0, steps)
    return n


@pytest.mark.parametrize("B,T,training", HEAD_CASES, ids=["%d-%d-%s" % (B, T, "train" if t else "eval") for B, T, t in HEAD_CASES])
def test_aasist_backend_long_clips_match_float64_oracle(dev, B, T, training):
    ref = make_reference(B, T, training)
    gpu = AasistHead(UPSTREAM_AASIST).to(dev)
    ref32 = OracleAasist(UPSTREAM_AASIST)
    for m in (gpu, ref32):
        m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    set_mode((gpu, ref32), training)
    nT = T // 3
    counts = node_counts([T])
    assert counts["W"][0] == nT and nT > 128 and (counts["N1"][0] > 128) == (T == 780)
    # the per-layer composition is what these sizes select
    assert not graph.supported(gpu, 42, nT) and not resstack.supported([blk[0] for blk in gpu.encoder], nT)
    y = labels(B)
    nbt0 = batch_counts(ref)
    gparams, rparams, params32 = dict(gpu.named_parameters()), dict(ref.named_parameters()), dict(ref32.named_parameters())
    rep = Fp32Floor("aasist long B=%d T=%d %s" % (B, T, "train" if training else "eval"), BARS_AASIST)
    plans = lambda mod: {(id(pl), getattr(pl, "gen", 0)) for pl in mod._PLANS}
    for step in range(2):
        rep.step = step
        x = head_input(step, B, T)
        xr, ro, rh, grads, margins = reference_step(ref, x, y)
        assert len(margins) == 6 and min(margins) > TOPK_MARGIN, \
            "step %d: a GraphPool top-k margin of %.2e in float64 (floor %.0e); pick another seed" % (step, min(margins), TOPK_MARGIN)
        # the oracle's own fp32 error on the same inputs and upstream gradient
        x32, o32, h32, _, _ = reference_step(ref32, x, y, torch.float32, grads)
        rep.record = True
        compare_all(rep, o32, h32, x32, params32, ref32, ro, rh, xr, rparams, ref, training, nbt0, step + 1 if training else 0)
        rep.record = False
        # the product back-end
        xg = x.to(dev).requires_grad_(True)
        rs_before, gr_before = plans(resstack), plans(graph)
        out, hid = gpu(xg)
        assert plans(resstack) == rs_before and plans(graph) == gr_before, "a fused plan ran: not the per-layer composition"
        torch.autograd.backward([out, hid], [grads[0].float().to(dev), grads[1].float().to(dev)])
        torch.cuda.synchronize()
        print("\n[aasist long B=%d T=%d %s step %d] min top-k margin %.2e" % (B, T, "train" if training else "eval", step, min(margins)))
        n = compare_all(rep, out, hid, xg, gparams, gpu, ro, rh, xr, rparams, ref, training, nbt0, step + 1 if training else 0)
        assert n == sum(1 for p in rparams.values() if p.grad is not None) == len(rparams) - 10, n
        assert not training or all(v == nbt0[k] + step + 1 for k, v in batch_counts(gpu).items()), batch_counts(gpu)
        for p in list(gparams.values()) + list(rparams.values()) + list(params32.values()):
            if p.grad is not None:
                p.grad.zero_()
    rep.done()


# ---- the plugins at 2 x 164,240 samples -----------------------------------------------------------------------------------------------------
# W2VConfig.tiny() has 16-wide heads, and the bf16 encoder path (training, SCL_SCORE_FP32=0) takes 513 frames only on the streaming attention
# (64-wide heads, or 72..128): tiny is refused there by the encoder, loudly.  So tiny runs where it can, the fp32 scoring path, and the
# train steps and the bf16 scoring run on the smallest encoder with 64-wide heads, the one the other long-clip tests use.
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)


# Scoring runs 2 clips.  The train steps run 4, two per class: with 2 clips the SupCon terms of the plugins' loss have no positive pair beside
# a negative one (mixed labels: NaN in the reference's own formula; equal labels: exactly 0), so a 2-clip step would leave them unchecked.
TRAIN_LABELS = [1, 1, 0, 0]


def long_clips(seed, B=2):
    return 0.1 * torch.randn(B, SAMPLES, generator=torch.Generator().manual_seed(seed))


def make_plugin(Model, args, dev, seed, tiny=False, prefix="ssl_model."):
    """A plugin and its oracle pieces on the same seeded weights, as the `make` of the plugin's own test file builds them."""
    ocfg, cfg = (W.W2VConfig.tiny(), W2VConfig.tiny()) if tiny else (W.W2VConfig(**SMALL), W2VConfig(**SMALL))
    ssl = W.init_state(ocfg, seed=seed)
    m = Model(args, dev, w2v_cfg=cfg)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith(prefix)}
    head_sd = {k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=seed + 1).items()}
    sd = {prefix + "model." + k: v for k, v in ssl.items()}
    sd.update(head_sd)
    m.load_state_dict(sd)
    return m, ssl, head_sd, ocfg


def make_aasist(dev, seed, tiny=False):
    m, ssl, head_sd, ocfg = make_plugin(TA.Model, TA.ARGS, dev, seed, tiny)
    ref = TA.CpuRef(ssl, ocfg, head_sd)
    for mod in list(m.modules()) + list(ref.modules()):
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m, ref, ocfg


def test_aasist_plugin_train_step_at_513_frames(dev):
    """tests/test_aasist_gpu.py::test_train_step_gradients_and_update at 4 x 164,240 samples."""
    m, ref, cfg = make_aasist(dev, 51)
    m.train(); ref.train()
    x, y = long_clips(3, 4), torch.tensor(TRAIN_LABELS)
    for n in [n for n, _, tr in W.param_shapes(cfg) if tr]:
        ref.ssl[n].requires_grad_(True)
    opt = FusedAdamW(m, lr=1e-4, weight_decay=1e-4, overlap=False)
    out, feats, hid = m(x.to(dev))
    assert feats.shape == (4, 513, 128) and out.shape == (4, 2) and hid.shape == (4, 160)
    losses = m.loss(out, feats, hid, y.to(dev), TA.CONF)
    opt.zero_grad()
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    # (1) back-end + losses on the SAME features: fp32 torch on both sides, 2e-3
    f_leaf = feats.detach().cpu().requires_grad_(True)
    ro, rh = OracleAasist.forward(ref, f_leaf)
    rl = OH.model_loss(ro, f_leaf, rh, y, 1)
    sum(rl.values()).backward()
    for k in rl:
        assert abs(float(losses[k].detach()) - float(rl[k].detach())) < 2e-3 * abs(float(rl[k].detach())) + 1e-5, (k, float(losses[k].detach()), float(rl[k].detach()))
    refp = dict(ref.named_parameters())
    errs = {k: TA.rl2(m.P.g(k), refp[k].grad) for k in ("out_layer.weight", "HtrgGAT_layer_ST11.att_weight12", "GAT_layer_T.proj_with_att.weight",
                                                       "GAT_layer_T.att_proj.weight", "GAT_layer_T.att_weight", "encoder.0.0.conv1.weight",
                                                       "attention.0.weight", "pos_S", "master1", "pool_hT2.proj.weight")}
    print("aasist plugin 513 frames, head gradients vs the fp32 oracle:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(v < 2e-3 for v in errs.values()), errs
    # (2) encoder + LL: the reference d(feats) through the fp32 oracle encoder; bf16 bar on the HIP side
    rf = ref.LL(W.forward(ref.ssl, cfg, x))
    assert TA.rl2(feats, rf) < 1e-2
    rf.backward(f_leaf.grad)
    for k in ("LL.weight", "LL.bias"):
        assert TA.rl2(m.P.g(k), refp[k].grad) < 3e-2, (k, TA.rl2(m.P.g(k), refp[k].grad))
    for n in ("post_extract_proj.weight", "encoder.layers.1.fc1.weight", "encoder.layers.0.self_attn.q_proj.weight", "feature_extractor.conv_layers.0.0.weight"):
        got, want = m.P.g("ssl_model.model." + n), ref.ssl[n].grad
        assert TA.rl2(got, want) < 8e-2, (n, TA.rl2(got, want))
    before = m.P.flat[: m.P.n_train].clone()
    opt.step()
    torch.cuda.synchronize()
    delta = (m.P.flat[: m.P.n_train] - before).abs()
    assert delta[m._head_lo:].max() > 0 and delta[: m._head_lo].max() > 0 and delta.max() <= 2.2e-4


@pytest.mark.parametrize("fp32,tiny", [(True, True), (True, False), (False, False)], ids=["fp32-tiny", "fp32", "bf16"])
def test_aasist_plugin_scores_at_513_frames(dev, monkeypatch, fp32, tiny):
    """tests/test_aasist_gpu.py::test_eval_forward_matches_cpu_reference at 2 x 164,240 samples, on both scoring precisions."""
    monkeypatch.setattr(MF, "SCORE_FP32", fp32)
    m, ref, cfg = make_aasist(dev, 41, tiny=tiny)
    m.eval(); ref.eval()
    x = long_clips(2)
    with torch.no_grad():
        ro, rf, rh = ref(x)
        out, feats, hid = m(x.to(dev))
    assert out.shape == (2, 2) and hid.shape == (2, 160) and feats.shape == rf.shape == (2, 513, 128)
    print("aasist plugin 513 frames eval %s: feats %.2e hidden %.2e logits %.2e" % ("fp32" if fp32 else "bf16", TA.rl2(feats, rf), TA.rl2(hid, rh), TA.rl2(out, ro)))
    assert TA.rl2(feats, rf) < 1e-2, TA.rl2(feats, rf)
    assert TA.rl2(hid, rh) < 5e-2 and TA.rl2(out, ro) < 5e-2, (TA.rl2(hid, rh), TA.rl2(out, ro))
    m.is_train = False
    with torch.no_grad():
        lone = m(x.to(dev))
    assert torch.equal(lone, out)


def test_resnet_plugin_at_513_frames(dev):
    """tests/test_resnet_gpu.py::test_eval_forward_and_train_step at 4 x 164,240 samples."""
    m, ssl, head_sd, cfg = make_plugin(TR.Model, TR.ARGS, dev, 91)
    ref = TR.CpuRef(ssl, cfg, head_sd)
    x, y = long_clips(2, 4), torch.tensor(TRAIN_LABELS)
    m.eval(); ref.eval()
    with torch.no_grad():
        rf = ref.LL(W.forward(ref.ssl, cfg, x))
        ro, re = ref.head(rf)
        out, feats, emb = m(x.to(dev))
    assert out.shape == (4, 2) and emb.shape == (4, 256) and feats.shape == (4, 513, 128)
    print("resnet plugin 513 frames eval: feats %.2e emb %.2e logits %.2e" % (TR.rl2(feats, rf), TR.rl2(emb, re), TR.rl2(out, ro)))
    assert TR.rl2(feats, rf) < 1e-2 and TR.rl2(emb, re) < 3e-2 and TR.rl2(out, ro) < 3e-2, (TR.rl2(feats, rf), TR.rl2(emb, re), TR.rl2(out, ro))
    m.train(); ref.train()
    opt = FusedAdamW(m, lr=1e-4, weight_decay=1e-4)
    out, feats, emb = m(x.to(dev))
    losses = m.loss(out, feats, emb, y.to(dev), TR.CONF)
    opt.zero_grad()
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    head2 = TR.CpuRef(ref.ssl, cfg, {k: v.cpu() for k, v in m.state_dict().items() if not k.startswith("ssl_model.")})
    head2.train()
    f_leaf = feats.detach().cpu().requires_grad_(True)
    o2, e2 = head2.head(f_leaf)
    rl = {k: v * 4 for k, v in OH.model_loss(o2, f_leaf, e2, y, 1).items()}      # this plugin's Model.loss has no 1/bz
    sum(rl.values()).backward()
    for k in rl:
        assert abs(float(losses[k].detach()) - float(rl[k].detach())) < 2e-3 * abs(float(rl[k].detach())) + 1e-5, k
    refp = dict(head2.named_parameters())
    errs = {k: TR.rl2(m.P.g(k), refp[k].grad) for k in ("resnet.fc.weight", "resnet.conv5.weight", "resnet.layer2.0.shortcut.0.weight", "resnet.conv1.weight", "first_bn.weight")}
    print("resnet plugin 513 frames, head gradients vs the fp32 oracle:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(v < 2e-2 for v in errs.values()), errs
    for n in [n for n, _, tr in W.param_shapes(cfg) if tr]:
        ref.ssl[n].requires_grad_(True)
        ref.ssl[n].grad = None
    head2.LL(W.forward(ref.ssl, cfg, x)).backward(f_leaf.grad)
    for n in ("post_extract_proj.weight", "encoder.layers.1.fc1.weight", "feature_extractor.conv_layers.0.0.weight"):
        assert TR.rl2(m.P.g("ssl_model.model." + n), ref.ssl[n].grad) < 8e-2, n
    assert TR.rl2(m.P.g("LL.weight"), refp["LL.weight"].grad) < 3e-2
    before = m.P.flat[: m.P.n_train].clone()
    opt.step()
    torch.cuda.synchronize()
    delta = (m.P.flat[: m.P.n_train] - before).abs()
    assert delta[m._head_lo:].max() > 0 and delta[: m._head_lo].max() > 0 and delta.max() <= 2.2e-4


# ---- main.py end to end ---------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_trains_and_scores_aasist_at_trim_length_164240(dev, tmp_path, monkeypatch):
    """One training epoch with its validation pass (packs of 164,240-sample views: 513 frames, 171 temporal nodes, on the default XLS-R-300M
    encoder, random init) and --eval, as tests/test_long_clip_gpu.py runs the linear plugin at 200,000."""
    import yaml
    import main as M
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    ids = ["u%d.wav" % i for i in range(4)]      # two per list: a pack draws num_additional_real other utterances of its list
    os.makedirs(root / "scp", exist_ok=True)
    for sub, names in (("scp/train_bonafide.lst", ids[:2]), ("scp/dev_bonafide.lst", ids[2:]), ("scp/test.lst", ids)):
        (root / sub).write_text("\n".join(names) + "\n")
    (root / "protocol.txt").write_text("")
    for u in ids:
        _write_wav(str(root / "bonafide" / u), 0.1 * rs.randn(30000 + 3000 * int(u[1])))
        _write_wav(str(root / "eval" / u), 0.1 * rs.randn(20000 + 9000 * int(u[1])))
        for v in ("hifigan", "waveglow"):
            _write_wav(str(root / "vocoded" / (v + "_" + u)), 0.1 * rs.randn(28000))
    cfg = {"model": {"name": "wav2vec2_aasist", "contra_mode": "all", "loss_type": 1},
           "data": {"name": "asvspoof_2019_augall_3", "kwargs": {"vocoders": ["hifigan", "waveglow"], "augmentation_methods": ["RawBoost12"],
                    "num_additional_real": 1, "trim_length": SAMPLES, "wav_samp_rate": 16000, "online_aug": True,
                    "aug_dir": str(tmp_path / "aug")}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("RANK", raising=False)
    seen, shapes = [], []
    run_orig, fwd_orig = M.run_epoch, AasistHead.forward

    def run_rec(loader, model, optimizer, device, config, train):
        r = run_orig(loader, model, optimizer, device, config, train)
        seen.append((train, float(r[0])))
        return r

    def fwd_rec(self, feats):
        shapes.append((self.training, feats.shape[1]))
        return fwd_orig(self, feats)
    monkeypatch.setattr(M, "run_epoch", run_rec)
    monkeypatch.setattr(AasistHead, "forward", fwd_rec)
    np.random.seed(0)
    rc = M.main(["--seed", "1", "--config", str(cfg_path), "--database_path", str(root), "--batch_size", "1", "--num_epochs", "1",
                 "--padding_type", "repeat", "--comment", "long"])
    assert rc == 0
    assert seen and all(np.isfinite(l) for _, l in seen), seen
    assert any(t for t, _ in seen) and any(not t for t, _ in seen)
    assert (True, 513) in shapes and (False, 513) in shapes, shapes      # the back-end trained and validated on 513-frame features
    m = M.MODEL_REGISTRY["wav2vec2_aasist"](cfg["model"], dev)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in m.state_dict().items()}, ck)
    out = tmp_path / "scores.txt"
    M.main(["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--eval", "--model_path", str(ck),
            "--eval_output", str(out)])
    lines = out.read_text().strip().split("\n")
    assert len(lines) == 4 and all(len(l.split()) == 3 for l in lines)
    assert np.isfinite(np.array([[float(v) for v in l.split()[1:]] for l in lines])).all()
