"""AasistHead.forward_frames_train (aasist_long.py): the AASIST back-end in train mode on zero-padded batches, head level, on the GPU, with the
machinery and bars (BARS_AASIST, the fp32-oracle fallback Fp32Floor) of tests/test_aasist_long_gpu.py.

  equal    equal frames 121 on a batch padded to 199 (NaN in the padding) against oracle.aasist_head.AasistHead in float64, train mode, on
           the compact batch feats[:, :121]: outputs, d(feats), every parameter gradient and every buffer, two steps
  alone    B = 1 at its own length (199 frames, no padding) against the oracle on the utterance alone, the same bars
  ragged   [30, 199, 121, 202, 64] and [780, 513, 45] (260 / 171 / 15 temporal nodes, heterogeneous layers of 151 / 106 / 28: the tiled var
           backward beside an utterance below 128 nodes) against the float64 DEFINITION, tests/aasist_train_cases.py::masked_train_forward,
           two steps with buffers; NaN and zeros in the padding give the same bits; rows of d(feats) at and beyond 3 * W_b are exact zeros
Dropout p = 0 (set_mode), weights from fill.  No fused plan may appear; the scoring forms still refuse train mode and autograd.
Preconditions, asserted: every GraphPool top-k margin above TOPK_MARGIN in float64 at both steps."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.aasist_head import AasistHead as OracleAasist  # noqa: E402
from scl_amd import graph, resstack  # noqa: E402
from scl_amd.aasist_head import UPSTREAM_AASIST, AasistHead  # noqa: E402
from test_aasist_long_gpu import Fp32Floor, compare_all, reference_step  # noqa: E402
from tests import aasist_train_cases as AC  # noqa: E402
from test_backends_train_gpu import BARS_AASIST, TOPK_MARGIN, batch_counts, fill, labels, set_mode  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")

# name -> (B, frames t0, padded T, seed of the weights)
ORACLE_CASES = {"equal": (2, 121, 199, 1004), "alone": (1, 199, 199, 1004)}      # float64 margins 2.3e-3 .. 9.2e-3 at both steps


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _input(step, B, T):
    return torch.randn(B, T, 128, generator=torch.Generator().manual_seed(7919 * step + B + T))


def _padded(x, T, fill_value, dev):
    out = torch.full((x.shape[0], T, 128), fill_value)
    out[:, : x.shape[1]] = x
    return out.to(dev).requires_grad_(True)


def _plans(mod):
    return {(id(pl), getattr(pl, "gen", 0)) for pl in mod._PLANS}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_equal_frames_match_the_float64_oracle_on_the_compact_batch(dev, case):
    B, t0, T, seed = ORACLE_CASES[case]
    ref = OracleAasist(UPSTREAM_AASIST).double()
    ref.load_state_dict(fill(ref, seed=seed))
    gpu, ref32 = AasistHead(UPSTREAM_AASIST).to(dev), OracleAasist(UPSTREAM_AASIST)
    for m in (gpu, ref32):
        m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    set_mode((ref, gpu, ref32), True)
    nbt0 = batch_counts(ref)
    gparams, rparams, params32 = dict(gpu.named_parameters()), dict(ref.named_parameters()), dict(ref32.named_parameters())
    rep = Fp32Floor("aasist varlen train %s" % case, BARS_AASIST)
    g = torch.Generator().manual_seed(17)
    for step in range(2):
        rep.step = step
        x = _input(step, B, t0)
        # one utterance has no contrastive pair: fixed cotangents instead of the plugin loss's
        grads = None if B > 1 else (torch.randn(B, 2, generator=g, dtype=torch.float64), torch.randn(B, 160, generator=g, dtype=torch.float64) / 16)
        xr, ro, rh, grads, margins = reference_step(ref, x, labels(B), torch.float64, grads)
        assert len(margins) == 6 and min(margins) > TOPK_MARGIN, \
            "step %d: a GraphPool top-k margin of %.2e in float64 (floor %.0e); pick another seed" % (step, min(margins), TOPK_MARGIN)
        x32, o32, h32, _, _ = reference_step(ref32, x, labels(B), torch.float32, grads)
        rep.record = True
        compare_all(rep, o32, h32, x32, params32, ref32, ro, rh, xr, rparams, ref, True, nbt0, step + 1)
        rep.record = False
        xg = _padded(x, T, NAN, dev)
        rs_before, gr_before = _plans(resstack), _plans(graph)
        out, hid = gpu.forward_frames_train(xg, [t0] * B)
        assert _plans(resstack) == rs_before and _plans(graph) == gr_before, "a fused plan ran"
        torch.autograd.backward([out, hid], [grads[0].float().to(dev), grads[1].float().to(dev)])
        torch.cuda.synchronize()
        own = 3 * (t0 // 3)
        assert bool((xg.grad[:, own:] == 0).all()), "d(feats) at and beyond 3 * W_b"
        n = compare_all(rep, out, hid, types.SimpleNamespace(grad=xg.grad[:, :t0]), gparams, gpu, ro, rh, xr, rparams, ref, True, nbt0, step + 1)
        assert n == sum(1 for p in rparams.values() if p.grad is not None)
        assert all(v == nbt0[k] + step + 1 for k, v in batch_counts(gpu).items()), batch_counts(gpu)
        for p in list(gparams.values()) + list(rparams.values()) + list(params32.values()):
            if p.grad is not None:
                p.grad.zero_()
    rep.done()


class _Named:
    """The definition's state dict behind the two accessors compare_buffers / compare_params read."""

    def __init__(self, t, buffers):
        self.t, self.buffers = t, buffers

    def named_buffers(self):
        return [(k, self.t[k]) for k in self.buffers]


@pytest.mark.parametrize("case", sorted(AC.HEAD_RAGGED))
def test_ragged_batch_matches_the_float64_definition(dev, case):
    """Ragged frames against tests/aasist_train_cases.py::masked_train_forward in float64 (pinned by tests/test_aasist_varlen_train_cpu.py) at
    BARS_AASIST, or 3 x what the same definition loses in fp32 on the CPU; two steps, buffers compared; top-k margins asserted per utterance.
    A second head gets zeros in place of the NaN padding: the same bits."""
    frames, seed = AC.HEAD_RAGGED[case]
    B, T = len(frames), max(frames)
    ref, t = AC.oracle_state(seed)
    _, t32 = AC.oracle_state(seed, torch.float32)
    buffers = [k for k, _ in ref.named_buffers()]
    heads = [AasistHead(UPSTREAM_AASIST).to(dev) for _ in range(2)]
    for h in heads:
        h.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    set_mode(heads, True)
    gpu = heads[0]
    nbt0 = batch_counts(ref)
    gparams = dict(gpu.named_parameters())
    rparams, params32 = {k: t[k] for k in gparams}, {k: t32[k] for k in gparams}
    rep = Fp32Floor("aasist varlen train ragged %s" % case, BARS_AASIST)
    own = [3 * (n // 3) for n in frames]

    def masked(x):      # what compare_all reads of d(feats): the rows an utterance owns, zeros elsewhere on both sides
        y = x.clone()
        for b, n in enumerate(own):
            y[b, n:] = 0
        return y

    for step in range(2):
        rep.step = step
        x = AC.head_input(step, B, T)
        grads = AC.head_cotangents(step, B)
        rec = {}
        xr = x.double().requires_grad_(True)
        ro, rh = AC.masked_train_forward(t, xr, frames, rec)
        torch.autograd.backward([ro, rh], list(grads))
        assert min(rec["margins"]) > TOPK_MARGIN, "step %d: a GraphPool top-k margin of %.2e in float64; pick another seed" % (step, min(rec["margins"]))
        x32 = x.clone().requires_grad_(True)
        o32, h32 = AC.masked_train_forward(t32, x32, frames)
        torch.autograd.backward([o32, h32], [g.float() for g in grads])
        rep.record = True
        compare_all(rep, o32, h32, x32, params32, _Named(t32, buffers), ro, rh, xr, rparams, _Named(t, buffers), True, nbt0, step + 1)
        rep.record = False
        got = []
        for h, fill_value in zip(heads, (NAN, 0.0)):
            xp = x.clone()
            for b, n in enumerate(frames):
                xp[b, n:] = fill_value
            xg = xp.to(dev).requires_grad_(True)
            rs_before, gr_before = _plans(resstack), _plans(graph)
            out, hid = h.forward_frames_train(xg, frames)
            assert _plans(resstack) == rs_before and _plans(graph) == gr_before, "a fused plan ran"
            torch.autograd.backward([out, hid], [grads[0].float().to(dev), grads[1].float().to(dev)])
            torch.cuda.synchronize()
            for b, n in enumerate(own):
                assert bool((xg.grad[b, n:] == 0).all()), ("d(feats) beyond the utterance", b)
            tensors = {"out": out.detach(), "hid": hid.detach(), "d_feats": xg.grad}
            tensors.update({"grad " + k: p.grad.clone() for k, p in h.named_parameters() if p.grad is not None})
            tensors.update({"buffer " + k: v.clone() for k, v in h.named_buffers()})
            got.append((tensors, out, hid, xg))
        diff = [k for k in got[0][0] if not torch.equal(got[0][0][k], got[1][0][k])]
        assert not diff, ("NaN and zero padding differ, step %d" % step, diff)
        _, out, hid, xg = got[0]
        assert (xr.grad - masked(xr.grad)).abs().max() == 0
        n = compare_all(rep, out, hid, xg, gparams, gpu, ro, rh, xr, rparams, _Named(t, buffers), True, nbt0, step + 1)
        assert n == sum(1 for p in rparams.values() if p.grad is not None)
        assert all(v == nbt0[k] + step + 1 for k, v in batch_counts(gpu).items()), batch_counts(gpu)
        for h in heads:
            for p in h.parameters():
                p.grad = None
        for d in (t, t32):
            for v in d.values():
                v.grad = None
    rep.done()


def test_modes_are_refused_loudly_and_the_scoring_refusals_stay(dev):
    head = AasistHead(UPSTREAM_AASIST).to(dev)
    x = torch.zeros(2, 64, 128, device=dev)
    head.train()
    for fn in (head.forward_frames, head.forward_frames_long):
        with pytest.raises(NotImplementedError, match="scoring mode"):
            fn(x, [64, 30])
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training mode"):
        head.forward_frames_train(x, [64, 30])
    with pytest.raises(ValueError, match="frames"):
        head.forward_frames_train(x, [64, 65])
    with pytest.raises(ValueError, match="frames"):
        head.forward_frames_train(x, [64, 2])
    head.eval()
    with pytest.raises(NotImplementedError, match="training mode"):
        head.forward_frames_train(x, [64, 30])


# ---- the plugin: SCL_AASIST_TRAIN_LENGTHS=1 ---------------------------------------------------------------------------------------------
# The two-layer encoder with 64-wide heads (SMALL of tests/test_aasist_long_gpu.py), 4 clips of 24000 samples, dropout p = 0.
CLIP, LENGTHS = 24000, [24000, 1040, 20000, 22001]
# attention.2.bias is not in the list: it shifts every score of the map by a constant and both poolings are soft-maxes, so its gradient is
# analytically zero (measured: noise on both sides), as tests/test_aasist_cpu.py::analytically_zero has it
HEAD_GRADS = ("out_layer.weight", "HtrgGAT_layer_ST11.att_weight12", "GAT_layer_T.proj_with_att.weight", "GAT_layer_T.att_proj.weight",
              "encoder.0.0.conv1.weight", "encoder.3.0.bn2.weight", "attention.0.weight", "attention.2.weight", "pos_S", "master1", "LL.weight")
SSL_GRADS = ("ssl_model.model.post_extract_proj.weight", "ssl_model.model.encoder.layers.1.fc1.weight")


def _plugin_step(dev, x, lengths):
    """A freshly built plugin (same seed every time), one forward + loss + backward -> (out, feats, hid, {name: gradient})."""
    import test_aasist_gpu as TA
    from test_aasist_long_gpu import TRAIN_LABELS, make_aasist
    m, _, _ = make_aasist(dev, 51)
    m.train()
    out, feats, hid = m(x.to(dev)) if lengths is None else m(x.to(dev), lengths=lengths)
    losses = m.loss(out, feats, hid, torch.tensor(TRAIN_LABELS).to(dev), TA.CONF)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return out.detach(), feats.detach(), hid.detach(), {k: m.P.g(k).detach().clone() for k in HEAD_GRADS + SSL_GRADS}


def _clips(seed):
    return 0.1 * torch.randn(4, CLIP, generator=torch.Generator().manual_seed(seed))


def test_plugin_trains_with_lengths_behind_the_switch(dev, monkeypatch):
    import test_aasist_gpu as TA
    x = _clips(5)
    monkeypatch.delenv("SCL_AASIST_TRAIN_LENGTHS", raising=False)
    monkeypatch.delenv("SCL_AASIST_LENGTHS", raising=False)
    with pytest.raises(NotImplementedError, match="SCL_AASIST_LENGTHS=1"):      # the switch off: the refusal as before
        _plugin_step(dev, x, LENGTHS)
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    # every sample valid, against the CPU chain oracle as tests/test_aasist_long_gpu.py::test_aasist_plugin_train_step_at_513_frames compares the
    # fixed-length step, with its bars: (1) back-end + losses on the SAME features, fp32 torch on both sides, 2e-3; (2) encoder + LL, bf16 bars
    from oracle import head as OH
    from oracle import wav2vec2 as W
    from test_aasist_long_gpu import TRAIN_LABELS, make_aasist
    m, ref, cfg = make_aasist(dev, 51)
    m.train(); ref.train()
    y = torch.tensor(TRAIN_LABELS)
    for n in [n for n, _, tr in W.param_shapes(cfg) if tr]:
        ref.ssl[n].requires_grad_(True)
    out, feats, hid = m(x.to(dev), lengths=[CLIP] * 4)
    losses = m.loss(out, feats, hid, y.to(dev), TA.CONF)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    f_leaf = feats.detach().cpu().requires_grad_(True)
    ro, rh = OracleAasist.forward(ref, f_leaf)
    rl = OH.model_loss(ro, f_leaf, rh, y, 1)
    sum(rl.values()).backward()
    for k in rl:
        assert abs(float(losses[k].detach()) - float(rl[k].detach())) < 2e-3 * abs(float(rl[k].detach())) + 1e-5, (k, float(losses[k].detach()), float(rl[k].detach()))
    refp = dict(ref.named_parameters())
    errs = {k: TA.rl2(m.P.g(k), refp[k].grad) for k in HEAD_GRADS if k != "LL.weight"}
    print("aasist plugin, lengths = full, head gradients vs the fp32 oracle on the same features:", {k: "%.2e" % v for k, v in errs.items()})
    assert all(v < 2e-3 for v in errs.values()), errs
    rf = ref.LL(W.forward(ref.ssl, cfg, x))
    assert TA.rl2(feats, rf) < 1e-2
    rf.backward(f_leaf.grad)
    for k in ("LL.weight", "LL.bias"):
        assert TA.rl2(m.P.g(k), refp[k].grad) < 3e-2, (k, TA.rl2(m.P.g(k), refp[k].grad))
    for n in ("post_extract_proj.weight", "encoder.layers.1.fc1.weight", "encoder.layers.0.self_attn.q_proj.weight"):
        got, want = m.P.g("ssl_model.model." + n), ref.ssl[n].grad
        assert TA.rl2(got, want) < 8e-2, (n, TA.rl2(got, want))
    # ragged lengths: what lies beyond an utterance's samples reaches no bit; feats rows beyond its frames are zero
    junk = x.clone()
    for b, n in enumerate(LENGTHS):
        junk[b, n:] = 3.0 * torch.randn(CLIP - n, generator=torch.Generator().manual_seed(b))
        x[b, n:] = 0.0
    a, b_ = _plugin_step(dev, x, LENGTHS), _plugin_step(dev, junk, LENGTHS)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]) and torch.equal(a[2], b_[2])
    diff = [k for k in a[3] if not torch.equal(a[3][k], b_[3][k])]
    assert not diff, diff
    assert all(bool(torch.isfinite(t).all()) for t in a[:3]) and all(bool(torch.isfinite(t).all()) for t in a[3].values())
    # scoring with lengths stays behind its own switch
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    from test_aasist_long_gpu import make_aasist
    m, _, _ = make_aasist(dev, 51)
    m.eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="SCL_AASIST_LENGTHS=1"):
        m(x.to(dev), lengths=LENGTHS)


def _step_on(m, x, lengths, dev):
    """One forward + loss + backward on an existing plugin -> (out, feats, hid, {trainable name: gradient copy})."""
    import test_aasist_gpu as TA
    from test_aasist_long_gpu import TRAIN_LABELS
    out, feats, hid = m(x.to(dev), lengths=lengths)
    losses = m.loss(out, feats, hid, torch.tensor(TRAIN_LABELS).to(dev), TA.CONF)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return out.detach(), feats.detach(), hid.detach(), {k: m.P.g(k).detach().clone() for k, (_, _, _, tr) in m.P.index.items() if tr}


def test_plugin_second_step_replays_the_first_steps_plans(dev, monkeypatch):
    from scl_amd.optim import FusedAdamW
    from test_aasist_long_gpu import make_aasist
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    m, _, _ = make_aasist(dev, 51)
    m.train()
    opt = FusedAdamW(m, lr=1e-4, weight_decay=1e-4, overlap=False)
    x = _clips(5)
    nbt = []
    for step in range(2):
        opt.zero_grad()
        out, _, hid, grads = _step_on(m, x, LENGTHS, dev)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(hid).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        opt.step()
        nbt.append(int(m.first_bn.num_batches_tracked))
        assert len(m._vstates_train) == 1 and len(m.ssl._vbufs_train) == 1, "the second step records nothing new"
    assert nbt == [1, 2]


# No frozen-encoder case: this plugin, like model/wav2vec2_aasist.py, does not read `flag_fix_ssl` (model_aasist.py: the SSL model follows
# the parent's train / eval mode), with or without lengths; the front's flag_fix_ssl branch is the ResNet plugin's and is tested there.
def test_feats_rows_beyond_an_utterances_frames_are_zero(dev, monkeypatch):
    from test_aasist_long_gpu import make_aasist
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    m, _, _ = make_aasist(dev, 51)
    m.train()
    _, feats, _, grads = _step_on(m, _clips(5), LENGTHS, dev)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for b, n in enumerate(LENGTHS):
        t = m.cfg.conv_lens(n)[-1]
        assert bool((feats[b, t:] == 0).all()) and bool(feats[b, :t].any())


def test_plugin_packed_encoder_rows_agree_with_the_padded_path(dev, monkeypatch):
    """SCL_VARLEN_PACK=1 packs the encoder rows, the back-end stays padded: the comparison and bars of
    tests/test_resnet_varlen_train_gpu.py's packed-against-padded test."""
    import test_aasist_gpu as TA
    from scl_amd import encoder as ENC
    from test_aasist_long_gpu import make_aasist
    from tests import nn_cases as NC
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    x = _clips(5)
    runs = []
    for pack in (False, True):
        monkeypatch.setattr(ENC, "VARLEN_PACK", pack)
        m, _, _ = make_aasist(dev, 51)
        m.train()
        runs.append(_step_on(m, x, LENGTHS, dev))
    padded, packed = runs
    st, = m._vstates_train.values()
    assert st["row0"] is not None, "the packed layout did not run"
    for name, a, b in zip(("logits", "feats", "hidden"), packed[:3], padded[:3]):
        print("packed vs padded %s: rel-L2 %.2e max-rel %.2e" % (name, TA.rl2(a, b), NC.maxrel(a, b)))
        assert TA.rl2(a, b) < 1e-2 and NC.maxrel(a, b) < 3e-2, name
    bad, worst = [], (1.0, 0.0)
    for name in padded[3]:
        a, b = packed[3][name].double().cpu().flatten(), padded[3][name].double().cpu().flatten()
        if b.abs().max().item() < 1e-6:
            ok = a.abs().max().item() < 2e-3
        else:
            c, e = (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item(), NC.maxrel(a, b)
            worst = (min(worst[0], c), max(worst[1], e))
            ok = c > 0.99 and e < 0.2
        if not ok:
            bad.append(name)
    print("packed vs padded gradients: worst cosine %.5f, worst max error %.3f of the tensor max" % worst)
    assert not bad, bad


def test_main_trains_the_aasist_plugin_on_two_zero_padded_packs_per_step(dev, tmp_path, monkeypatch):
    """tests/test_resnet_varlen_train_gpu.py::test_main_trains_the_resnet_plugin_on_two_zero_padded_packs_per_step with both switches set."""
    import wave
    import numpy as np
    import yaml
    import main as M
    from scl_amd.encoder import W2VConfig
    from test_aasist_long_gpu import SMALL
    monkeypatch.setenv("SCL_AASIST_TRAIN_LENGTHS", "1")
    monkeypatch.setenv("SCL_AASIST_LENGTHS", "1")

    def write_wav(path, x):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with wave.open(path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    ids = ["u%d.wav" % i for i in range(6)]
    sizes = [19000, 26000, 9000, 21000, 18500, 23000]      # shorter and longer than trim_length
    os.makedirs(root / "scp", exist_ok=True)
    for sub, names in (("scp/train_bonafide.lst", ids[:4]), ("scp/dev_bonafide.lst", ids[4:]), ("scp/test.lst", ids)):
        (root / sub).write_text("\n".join(names) + "\n")
    (root / "protocol.txt").write_text("")
    for u, n in zip(ids, sizes):
        write_wav(str(root / "bonafide" / u), 0.1 * rs.randn(n))
        for j, v in enumerate(("hifigan", "waveglow")):
            write_wav(str(root / "vocoded" / (v + "_" + u)), 0.1 * rs.randn(n - 700 + 1500 * j))
    trim = 24000
    cfg = {"model": {"name": "wav2vec2_aasist", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "asvspoof_2019_augall_3", "kwargs": {"vocoders": ["hifigan", "waveglow"], "augmentation_methods": ["RawBoost12"],
                    "num_additional_real": 1, "trim_length": trim, "wav_samp_rate": 16000, "online_aug": True,
                    "aug_dir": str(tmp_path / "aug")}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    calls, made = [], []
    reg = dict(M.MODEL_REGISTRY)
    ctor = reg["wav2vec2_aasist"]

    def spy(*a, **k):
        m = ctor(*a, w2v_cfg=W2VConfig(**SMALL), **k)      # 64-wide heads (the YAML's tiny preset has 16-wide ones)
        inner = m.forward

        def forward(x, lengths=None):
            calls.append((bool(m.training), torch.is_grad_enabled(), tuple(x.shape), None if lengths is None else list(lengths)))
            return inner(x, lengths)
        m.forward = forward
        made.append(m)
        return m
    reg["wav2vec2_aasist"] = spy
    monkeypatch.setattr(M, "MODEL_REGISTRY", reg)
    seen = []
    run_orig = M.run_epoch

    def run_rec(loader, model, optimizer, device, config, train):
        r = run_orig(loader, model, optimizer, device, config, train)
        seen.append((train, float(r[0])))
        return r
    monkeypatch.setattr(M, "run_epoch", run_rec)
    early = M.EarlyStop
    monkeypatch.setattr(M, "EarlyStop", lambda **kw: early(**dict(kw, init_best=-1.0)))      # an untrained toy model still writes its checkpoint
    np.random.seed(0)
    rc = M.main(["--seed", "1", "--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--num_epochs", "1",
                 "--padding_type", "zero", "--comment", "zp"])
    assert rc == 0
    assert [t for t, _ in seen] == [True, False] and all(np.isfinite(l) for _, l in seen), seen
    lo = made[-1].min_samples()
    train_calls = [c for c in calls if c[0]]
    assert len(train_calls) == 2 and len(calls) >= 3
    for training, grad, shape, lengths in calls:
        assert grad == training and lengths is not None and shape[1] == trim and len(lengths) == shape[0]
        assert all(lo <= n <= trim for n in lengths)
    assert all(min(c[3]) < trim for c in train_calls)
    saved = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "out") for f in fs if f.endswith(".pth")]
    assert saved, "no checkpoint written"
    sd = torch.load(saved[0], map_location="cpu")
    assert int(sd["first_bn.num_batches_tracked"]) == 2 and int(sd["encoder.1.0.bn1.num_batches_tracked"]) == 2      # two masked training steps
