"""The layer mix (YAML `ssl_layer_mix`) at model level: switched off nothing changes; with a one-hot soft-max on the last state the
mix-on model IS the mix-off model, bit for bit, through dropout, LayerDrop, padded and packed layouts and recorded plans; with random
logits it follows the fp64 definition of tests/layer_mix_cases.py; the fp32 scoring path, a frozen encoder, another plugin and two
data-parallel ranks carry it."""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd.encoder import MIX_WEIGHT, W2VConfig  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from scl_amd.optim import FusedAdamW  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests import layer_mix_cases as LM  # noqa: E402

ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
CONF = {"model": {"contra_mode": "all", "loss_type": 1}}
TINY = dict(conv_dim=32, embed=64, layers=2, heads=4, ffn=128, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)      # W2VConfig.tiny()
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)   # 64-wide heads
Y6 = torch.tensor([1, 1, 1, 0, 0, 0])
LENGTHS6 = [12000, 9000, 7000, 12000, 5000, 10000]


def clips(seed, B=6, L=12000):
    return 0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def build(dev, ssl, head, fields, mix, logits=None, args=ARGS, **cfg_kw):
    m = Model(args, dev, w2v_cfg=W2VConfig(layer_mix=mix, **fields, **cfg_kw))
    sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
    sd.update(head)
    if logits is not None:
        sd[MIX_WEIGHT] = logits
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("first_bn" in k or (k == MIX_WEIGHT and logits is None) for k in missing), (missing, unexpected)
    return m


def step(m, x, y, dev, lengths=None):
    out, feats, emb = m(x.to(dev)) if lengths is None else m(x.to(dev), lengths=lengths)
    sum(m.loss(out, feats, emb, y.to(dev), CONF).values()).backward()
    torch.cuda.synchronize()
    return out.clone(), feats.clone(), emb.clone()


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()


def relerr(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def cosine(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()


# ---- 1. switched off ----------------------------------------------------------------------------------------------------------------------
def test_switch_off_is_the_model_without_the_key(dev):
    """`ssl_layer_mix: false` against a dict that does not know the key: same layout, same outputs, same gradient bits, over a recorded
    step and its replay, in train mode (head dropout on)."""
    runs = []
    for extra in ({}, {"ssl_layer_mix": False}):
        m = Model(dict(ARGS, w2v_arch="tiny", **extra), dev, seed=3)
        assert m.cfg.layer_mix is False and MIX_WEIGHT not in m.state_dict() and m.layer_mix_weights() is None
        m.train()
        res = [step(m, clips(11, 4, 4000), torch.tensor([1, 1, 0, 0]), dev) + (m.P.grad.clone(),) for _ in range(2)]
        runs.append((dict(m.P.index), res))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---- 2. bit identity ------------------------------------------------------------------------------------------------------------------------
def one_hot_logits(layers):
    a = torch.full((layers + 1,), -1e4)
    a[-1] = 0.0
    return a


DROPS = {"p0": {}, "drop_layerdrop": dict(dropout=0.1, encoder_layerdrop=0.35), "drop_replay": dict(dropout=0.1)}
# CPU seed of the LayerDrop draws (two layers, two steps): torch.manual_seed(11) gives skip = [True, False], [False, True] at p = 0.35 — the
# bottom layer skipped in the first step, the top one in the second
LAYERDROP_SEED = 11


@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("layout", ["fixed", "padded", "packed"])
def test_one_hot_mix_on_the_last_state_equals_the_model_without_the_mix_bit_for_bit(dev, monkeypatch, layout, drop):
    """Logits of -1e4 everywhere but index L: the soft-max is exactly (0, .., 0, 1) in f32, so in train mode outputs and every encoder
    and head gradient must carry the bits of the mix-off model — the injection points, the mask of the rewritten bf16 pair, LayerDrop
    and the seeds of a replayed plan, without a tolerance.  fixed: the tiny config; padded and packed: 2 layers with 64-wide heads
    (tiny's 16-wide heads take no lengths on the bf16 path)."""
    fields = TINY if layout == "fixed" else SMALL
    monkeypatch.setattr(ENC, "VARLEN_PACK", layout == "packed")
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    ocfg = W.W2VConfig(**fields)
    ssl, head = W.init_state(ocfg, seed=31), OH.init_head(ocfg.embed, seed=32)
    x, lengths = clips(12), (None if layout == "fixed" else LENGTHS6)
    torch.manual_seed(LAYERDROP_SEED)
    assert [[float(torch.rand(())) < 0.35 for _ in range(2)] for _ in range(2)] == [[True, False], [False, True]]
    res = {}
    for mix in (False, True):
        m = build(dev, ssl, head, fields, mix, one_hot_logits(2) if mix else None, **DROPS[drop])
        m.train()
        if mix:
            w = m.layer_mix_weights()
            assert w.tolist() == [0.0, 0.0, 1.0]
        torch.manual_seed(LAYERDROP_SEED)
        steps = []
        for _ in range(2):      # the second step replays the recorded plans where there are any (no LayerDrop) under new seeds
            outs = step(m, x, Y6, dev, lengths)
            steps.append((outs, {n: m.P.g(n).clone() for n, (_, _, _, tr) in m.P.index.items() if tr}))
        res[mix] = steps
    for s, ((outs_off, g_off), (outs_on, g_on)) in enumerate(zip(res[False], res[True])):
        for a, b in zip(outs_off, outs_on):
            assert torch.equal(a, b), (s, "outputs")
        assert set(g_on) == set(g_off) | {MIX_WEIGHT}
        bad = [n for n in g_off if not torch.equal(g_off[n], g_on[n])]
        assert not bad, (s, bad[:5], len(bad))
        assert max(v.abs().max().item() for v in g_off.values()) > 0
    if drop == "drop_layerdrop":      # the skips did happen: a skipped layer's gradients are exactly zero
        z = lambda g, n: g["ssl_model.model.encoder.layers.%d.fc1.weight" % n].abs().max().item() == 0
        assert z(res[True][0][1], 0) and not z(res[True][0][1], 1) and z(res[True][1][1], 1) and not z(res[True][1][1], 0)
    if drop != "p0":      # and the two steps drew different masks
        assert not torch.equal(res[True][0][0][1], res[True][1][0][1])


# ---- 3. against the definition --------------------------------------------------------------------------------------------------------------
def gradient_failures(m, grads):
    """tests/test_model_gpu.py::test_every_parameter_gradient_matches_oracle_autograd's criterion over every tensor of `grads`; the mix's
    logits are held like the encoder's LayerNorm weights (a full reduction over the same tensors)."""
    bad, n = [], 0
    for name, ref in grads.items():
        got = m.P.g(name).cpu()
        n += 1
        if ref.abs().max().item() < 1e-6:
            ok = got.abs().max().item() < 2e-3
        else:
            lim = 0.25 if name.startswith("backend.m_frame_level") else 0.2
            ok = cosine(got, ref) > 0.99 and relerr(got, ref) < lim
        if not ok:
            bad.append((name, cosine(got, ref), relerr(got, ref)))
    assert n > 60 and MIX_WEIGHT in grads
    return bad


@pytest.mark.parametrize("skip_last", [False, True], ids=["all_layers", "last_layer_skipped"])
def test_random_logits_follow_the_fp64_definition(dev, monkeypatch, skip_last):
    """Eval mode (no dropout on either side), tiny config, 6 x 12000 samples: outputs at the bf16 bars of tests/test_model_gpu.py (relative
    L2 < 1e-2, no element off by more than 3e-2 of the tensor's maximum), every parameter gradient, layer_mix.weight's among them, at
    the criterion of its gradient test.  Once with the last layer skipped by LayerDrop: h_L is then the final LayerNorm of h_{L-1}.
    Weights and batch are those of test_every_parameter_gradient_matches_oracle_autograd (seeds 91 / 92 / 8), whose criterion this is: how
    many LeakyReLU slopes of the head flip under the bf16 encoder's perturbation is a property of the batch, with the mix or without it
    (measured on another batch, seeds 41 / 42 / 13, WITHOUT the mix and with every layer run: cosine 0.9892 and 0.9881 for
    backend.m_frame_level.0.bias / .3.bias against this criterion's 0.99)."""
    ocfg = W.W2VConfig.tiny()
    ssl, head = W.init_state(ocfg, seed=91), OH.init_head(ocfg.embed, seed=92)
    logits = torch.tensor([0.7, -0.4, 0.2])
    m = build(dev, ssl, head, TINY, True, logits)
    m.eval()
    x = clips(8)
    if skip_last:
        # the encoder alone in training mode (its dropouts are 0), the head in eval mode; the draws scripted: layer 0 kept, layer 1 skipped
        m.cfg.encoder_layerdrop = 0.5
        fwd = m.ssl.forward
        monkeypatch.setattr(m.ssl, "forward", lambda x_, training=True, **kw: fwd(x_, **dict(kw, training=True)))
        draws = iter([torch.tensor(0.9), torch.tensor(0.1)])
        with monkeypatch.context() as mp_:
            mp_.setattr(torch, "rand", lambda *a, **k: next(draws))
            out, feats, emb = m(x.to(dev))
        assert next(draws, None) is None
    else:
        out, feats, emb = m(x.to(dev))
    sum(m.loss(out, feats, emb, Y6.to(dev), CONF).values()).backward()
    torch.cuda.synchronize()
    (ro, rf, re), grads = LM.reference_grads(ssl, head, ocfg, x, Y6, logits, skip_last)
    for name, got, ref in (("out", out, ro), ("feats", feats, rf), ("emb", emb, re)):
        print("%s: rl2 %.3e relerr %.3e" % (name, rl2(got, ref), relerr(got, ref)))
        assert rl2(got, ref) < 1e-2 and relerr(got, ref) < 3e-2, name
    print("d(logits): got %s want %s" % (m.P.g(MIX_WEIGHT).tolist(), grads[MIX_WEIGHT].tolist()))
    if skip_last:
        assert grads["ssl_model.model.encoder.layers.1.fc1.weight"].abs().max().item() == 0
    bad = gradient_failures(m, grads)
    assert not bad, bad


# ---- 4. fp32 scoring -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["fixed", "padded", "packed"])
def test_fp32_scoring_follows_the_definition_to_1e3(dev, monkeypatch, layout):
    """Encoder.forward_f32 with random logits at the bar of test_fp32_scoring_path_matches_oracle_to_1e3_at_xlsr_shape (1e-3 of each
    tensor's largest value): tiny fixed-length and zero-padded, and SCL_SCORE_PACK=1 on the encoder with 64-wide heads.  A padded
    utterance is held to what the definition gives it alone at its own length; feats beyond its frames are 0."""
    fields = SMALL if layout == "packed" else TINY
    monkeypatch.setattr(ENC, "SCORE_PACK", layout == "packed")
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    ocfg = W.W2VConfig(**fields)
    ssl, head = W.init_state(ocfg, seed=51), OH.init_head(ocfg.embed, seed=52)
    logits = torch.tensor([-0.3, 0.9, 0.1])
    m = build(dev, ssl, head, fields, True, logits)
    m.eval()
    x = clips(14, 4, 9000)
    lengths = None if layout == "fixed" else [9000, 4000, 6500, 2000]
    with torch.no_grad():
        out, feats, emb = m(x.to(dev)) if lengths is None else m(x.to(dev), lengths=lengths)
        if lengths is None:
            ro, rf, re = LM.full_forward(LM.to64(ssl), LM.to64(head), ocfg, x.double(), logits.double())
        else:
            ro, rf, re = torch.zeros(4, 2, dtype=torch.float64), torch.zeros(feats.shape, dtype=torch.float64), torch.zeros(4, 128, dtype=torch.float64)
            for b, n in enumerate(lengths):
                o, f, e = LM.full_forward(LM.to64(ssl), LM.to64(head), ocfg, x[b:b + 1, :n].double(), logits.double())
                ro[b], re[b], rf[b, : f.shape[1]] = o[0], e[0], f[0]
                if f.shape[1] < feats.shape[1]:
                    assert feats[b, f.shape[1]:].abs().max().item() == 0
    mx = lambda a, b: ((a.double().cpu() - b).abs().max() / b.abs().max()).item()
    print("fp32 scoring with the mix (%s): max-rel logp %.2e emb %.2e feats %.2e" % (layout, mx(out, ro), mx(emb, re), mx(feats, rf)))
    assert mx(out, ro) < 1e-3 and mx(emb, re) < 1e-3 and mx(feats, rf) < 1e-3


# ---- 5. frozen encoder -----------------------------------------------------------------------------------------------------------------------
def test_frozen_encoder_trains_the_mix_and_the_head_only(dev):
    """flag_fix_ssl with the mix: d(mix) is formed for the logits alone.  The frozen model's forward is the unfrozen model's eval-mode
    forward (the same kernels on the same buffers), so g = d(mix) has the same bits and scl_layer_mix_bwd_w, a fixed-order reduction,
    gives the logits' gradient the same BITS as the unfrozen run — equality, not a bar.  The encoder's gradients stay untouched (zero),
    and one AdamW step moves the logits and the head and nothing of the encoder."""
    ocfg = W.W2VConfig.tiny()
    ssl, head = W.init_state(ocfg, seed=61), OH.init_head(ocfg.embed, seed=62)
    logits = torch.tensor([0.5, -0.2, 0.1])
    x, y = clips(15, 4, 4000), torch.tensor([1, 1, 0, 0])
    res = {}
    for frozen in (False, True):
        m = build(dev, ssl, head, TINY, True, logits, args=dict(ARGS, flag_fix_ssl=frozen))
        m.eval()
        opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-2)
        before = m.P.flat[: m.P.n_train].clone()
        opt.zero_grad()
        outs = step(m, x, y, dev)
        grad = m.P.grad[: m.P.n_train].clone()
        opt.step()
        torch.cuda.synchronize()
        lo, hi = m.trainable_range()
        res[frozen] = (outs, grad, m.P.flat[: m.P.n_train] - before, lo, m.P.off(MIX_WEIGHT))
        assert (lo if frozen else m.P.off("LL.weight")) <= m.P.off(MIX_WEIGHT) < hi
    lo, om = res[True][3], res[True][4]
    assert 0 < lo <= om
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    assert res[True][1][:lo].abs().max().item() == 0.0 and res[False][1][:lo].abs().max().item() > 0
    assert torch.equal(res[True][1][lo:], res[False][1][lo:])                      # head and mix gradients: the same bits
    assert res[True][1][om:om + 3].abs().max().item() > 0
    assert res[True][2][:lo].abs().max().item() == 0.0                               # the encoder did not move
    assert res[True][2][om:om + 3].abs().min().item() > 0                            # the logits did, every one of them
    assert torch.equal(res[True][2][lo:], res[False][2][lo:])


# ---- 6. another plugin ------------------------------------------------------------------------------------------------------------------------
def test_resnet_plugin_trains_a_step_with_the_mix_and_round_trips_its_state(dev):
    from scl_amd.model_resnet import Model as RModel
    from scl_amd.resnet_head import DEFAULT_RESNET
    args = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "resnet": DEFAULT_RESNET}
    m = RModel(args, dev, w2v_cfg=W2VConfig.tiny().with_layer_mix(), seed=5)
    assert MIX_WEIGHT in m.state_dict() and m.P.off(MIX_WEIGHT) == m.P.off("LL.bias") + 128
    assert torch.equal(m.layer_mix_weights(), torch.full((3,), 1.0 / 3))      # zeros at initialisation: a uniform average
    m.train()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4)
    x, y = clips(16, 4, 24000), torch.tensor([1, 1, 0, 0])
    out, feats, emb = m(x.to(dev))
    losses = m.loss(out, feats, emb, y.to(dev), CONF)
    opt.zero_grad()
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in (out, feats, emb)) and torch.isfinite(m.P.grad).all()
    g = m.P.g(MIX_WEIGHT).clone()
    assert g.abs().max().item() > 0 and abs(g.sum().item()) <= 1e-5 * g.abs().max().item() + 1e-12      # a soft-max gradient sums to zero
    a0 = m.P.f32(MIX_WEIGHT).clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(m.P.f32(MIX_WEIGHT), a0) and torch.isfinite(m.P.flat).all()
    sd = copy.deepcopy(m.state_dict())
    m2 = RModel(args, dev, w2v_cfg=W2VConfig.tiny().with_layer_mix(), seed=6)
    m2.load_state_dict(sd)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    del sd[MIX_WEIGHT]
    with pytest.raises(RuntimeError, match="layer_mix.weight"):
        m2.load_state_dict(sd, strict=True)
    # and a mix-off model refuses the key it does not have
    m3 = RModel(args, dev, w2v_cfg=W2VConfig.tiny(), seed=6)
    with pytest.raises(RuntimeError, match="layer_mix.weight"):
        m3.load_state_dict(m.state_dict(), strict=True)


# ---- 7. data parallel -------------------------------------------------------------------------------------------------------------------------
DP_ARGS = dict(ARGS, w2v_arch="tiny", ssl_layer_mix=True)


def _dp_data(rank):
    g = torch.Generator().manual_seed(300 + rank)
    return 0.1 * torch.randn(4, 4000, generator=g), torch.tensor([1, 1, 0, 0])


def _dp_model(dev):
    m = Model(DP_ARGS, dev, seed=0)
    m.P.f32(MIX_WEIGHT).copy_(torch.tensor([0.4, -0.3, 0.2]))
    m.P.mark_dirty()
    m.eval()
    return m


def _worker_mix(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from scl_amd.parallel import GradSync
    dev = torch.device("cuda:0")
    m = _dp_model(dev)
    sync = GradSync(m.P.grad[: m.P.n_train], bucket_elems=40000)
    o = m.P.off(MIX_WEIGHT)
    handed = []      # the logits' gradient as it stands when its bucket is handed to the collective
    sync.final_check = lambda a, b: handed.append(m.P.grad[o:o + 3].clone()) if a <= o < b else None
    opt = FusedAdamW(m, lr=0.0, weight_decay=0.0, grad_sync=sync)      # the weights stay: both steps have the gradient of the first
    x, y = _dp_data(rank)
    early = []
    for _ in range(2):      # the second step replays the recorded plan with its callbacks
        m.P.grad.zero_()
        out, feats, emb = m(x.to(dev))
        total = sum(m.loss(out, feats, emb, y.to(dev), CONF).values())
        opt.zero_grad()
        sync.begin()
        total.backward()
        early.append(sync.launched)      # buckets the backward itself announced (the tail, the logits' among them)
        opt.step()
        torch.cuda.synchronize()
    reduced = m.P.grad[o:o + 3].clone() / world
    q.put((rank, reduced.cpu().numpy(), [h.cpu().numpy() for h in handed], early, len(sync.bounds)))
    dist.destroy_process_group()


def test_two_ranks_all_reduce_the_logits_gradient_to_the_mean(dev):
    """Modelled on tests/test_dp_gpu.py: two processes on cuda:0 over gloo.  The logits sit in the tail of the flat buffer, which is
    reduced first, from a callback inside the backward: what is handed over there must already be the rank's final gradient, and what comes
    back the mean of the two ranks' single-process gradients (that file's bar, 2e-6)."""
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_mix, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=300) for _ in range(world))}
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    m = _dp_model(dev)
    own = []
    for r in range(world):
        x, y = _dp_data(r)
        step(m, x, y, dev)
        own.append(m.P.g(MIX_WEIGHT).clone().cpu())
    mean = (own[0] + own[1]) / world
    assert mean.abs().max().item() > 0
    for r in range(world):
        reduced, handed, early, nbuckets = res[r]
        assert nbuckets > 3 and len(handed) == 2 and all(e >= 1 for e in early)      # bucketed, and announced from inside the backward
        for h in handed:
            assert torch.equal(torch.from_numpy(h), own[r])      # final at hand-over, recorded step and replay
        assert (torch.from_numpy(reduced) - mean).abs().max().item() < 2e-6
