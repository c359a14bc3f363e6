"""The packed variable-length path at model level (encoder.VARLEN_PACK): the transformer layers of the linear model on the valid frames
only, packed back to back.  The small encoder and the oracle set-up of tests/test_varlen_train_gpu.py; PACK_ROWS is set to 64 so that
bucket edges are reachable at this size.  Outputs and every parameter gradient against the CPU oracle's autograd on each utterance ALONE
with the padded path's bars; exact zeros wherever no frame is valid; padding content; launch plans per (direction, row count); dropout;
a replayed step against a fresh recording at its seed, bit for bit, on every row layout; every frame valid; bf16 scoring;
main.py --padding_type zero --batch_size 2 with the switch on."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests import test_varlen_train_gpu as VT  # noqa: E402
from tests.test_varlen_train_gpu import SMALL, cosine, maxrel, relerr, rl2  # noqa: E402

LENGTHS = [20880, 400, 20560, 7777, 12000, 4000]      # 65, 1, 64, 24, 37 and 12 frames: T = 65, Mv = 203, Mq = 256
FRAMES = [65, 1, 64, 24, 37, 12]
FULL = [20880, 20880, 20880]                          # every frame valid: 3 x 65 = 195 rows, Mq = roundup(195, 64) = 256
_REF = {}


def test_the_frames_of_the_batch():
    """The layout the other tests rely on, from the conv stack's own arithmetic (no GPU work)."""
    cfg = W2VConfig(**SMALL)
    assert [cfg.conv_lens(n)[-1] for n in LENGTHS] == FRAMES and cfg.conv_lens(max(LENGTHS))[-1] == 65
    row0, Mq = ops.packed_rows(FRAMES, 65, 64)
    assert row0 == [0, 65, 66, 130, 154, 191, 203] and Mq == 256
    assert ops.packed_rows([65] * 3, 65, 64)[1] == 256 == (3 * 65 + 63) // 64 * 64


def _inputs(lengths):
    """tests/test_varlen_train_gpu.py's _inputs for other lengths: the zero-padded batch and fixed upstream gradients (d_feats is
    non-zero in the padded rows too)."""
    cfg = W2VConfig(**SMALL)
    gen = torch.Generator().manual_seed(4048 + len(lengths))
    B, L = len(lengths), max(lengths)
    T = cfg.conv_lens(L)[-1]
    x = torch.zeros(B, L)
    for b, n in enumerate(lengths):
        x[b, :n] = 0.1 * torch.randn(n, generator=gen)
    ups = (0.3 * torch.randn(B, 2, generator=gen), 0.01 * torch.randn(B, T, 128, generator=gen), 0.05 * torch.randn(B, 128, generator=gen))
    return x, ups, T


def _oracle(lengths):
    """CPU oracle, fp32 autograd, with the weights of tests/test_varlen_train_gpu.py's oracle: every utterance alone at its own length;
    the parameter gradients of <upstream, outputs> summed over the utterances, and each utterance's outputs.  Once per set of lengths."""
    key = tuple(lengths)
    if key not in _REF:
        base = VT._oracle_alone()
        ocfg = W.W2VConfig(**SMALL)
        ssl, head = base["ssl"], base["head"]
        x, (d_out, d_feats, d_emb), _ = _inputs(lengths)
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
        _REF[key] = dict(grads=grads, outs=outs)
    return _REF[key]


def _packed_model(dev, monkeypatch, **kw):
    monkeypatch.setattr(ENC, "VARLEN_PACK", True)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    return VT._train_model(dev, monkeypatch, **kw)


def _check_outputs(out, feats, emb, ref, lengths, cfg, what):
    for b, n in enumerate(lengths):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = ref["outs"][b]
        errs = [(rl2(g, r), maxrel(g, r)) for g, r in ((out[b], ro[0]), (emb[b], re[0]), (feats[b, :Tb], rf[0]))]
        print("%s n=%d (%d frames): (rel-L2, max-rel) logp %s emb %s feats %s" % ((what, n, Tb) + tuple("(%.2e, %.2e)" % e for e in errs)))
        assert all(e[0] < 1e-2 and e[1] < 3e-2 for e in errs), (what, n, errs)      # the padded path's bar for outputs
        assert (feats[b, Tb:] == 0).all()


def _check_against_the_oracle(m, cfg, step, ref, lengths):
    out, feats, emb, _ = step
    _check_outputs(out, feats, emb, ref, lengths, cfg, "packed")
    bad, cnt, worst = [], 0, (1.0, 0.0)
    for name, r in ref["grads"].items():
        got = m.P.g(name).cpu()
        cnt += 1
        if r.abs().max().item() < 1e-6:
            ok = got.abs().max().item() < 2e-3
        else:
            lim = 0.25 if name.startswith("backend.m_frame_level") else 0.2
            c, e = cosine(got, r), relerr(got, r)
            worst = (min(worst[0], c), max(worst[1], e))
            ok = c > 0.99 and e < lim
        if not ok:
            bad.append((name, cosine(got, r), relerr(got, r)))
    print("%d tensors: worst cosine %.5f, worst max error %.3f of the tensor max" % (cnt, worst[0], worst[1]))
    assert cnt > 60 and not bad, bad


def _packed_set(m):
    keys = [k for k in m.encoder._vbufs_train if k[-1] == "packed"]
    assert len(keys) == 1      # one buffer set per padded shape, whatever the lengths
    return m.encoder._vbufs_train[keys[0]]


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------
def test_packed_training_batch_gives_the_sum_of_each_utterance_alone(dev, monkeypatch):
    """Bars of test_padded_training_batch_gives_the_sum_of_each_utterance_alone: outputs rel-L2 < 1e-2 and max-rel < 3e-2; gradients
    cosine > 0.99 and max error < 20 % of the tensor's max (25 % for the frame-level head), 2e-3 absolute where the reference is zero."""
    ref = _oracle(LENGTHS)
    x, ups, T = _inputs(LENGTHS)
    m, cfg = _packed_model(dev, monkeypatch)
    step = VT._step(m, x, LENGTHS, ups, dev)
    d = _packed_set(m)
    assert d["long_attn"] and "attn_ws" in d and "S" not in d and d["dS"] is None and not m.encoder._vbufs and not m.encoder._bufs
    assert d["xin"][0].numel() == d["Mp"] * cfg.embed and d["Mp"] == 448      # sized for roundup(B * T, 64) rows
    st, = m._vstates_train.values()
    assert sorted(k[-1] for k in st["plans"]) == [256, 256] and st["row0"].tolist() == [0, 65, 66, 130, 154, 191, 203]
    _check_against_the_oracle(m, cfg, step, ref, LENGTHS)
    # the padded path on the same batch (figures only: the GEMM plans may differ with the row count)
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    padded = VT._step(m, x, LENGTHS, ups, dev)
    diffs = [(relerr(step[3][m.P.off(n):m.P.off(n) + r.numel()], padded[3][m.P.off(n):m.P.off(n) + r.numel()]), n) for n, r in ref["grads"].items()]
    print("packed vs padded path: outputs max-rel %.2e / %.2e / %.2e; gradients worst max error %.3e of the tensor max (%s)"
          % (maxrel(step[0], padded[0]), maxrel(step[1], padded[1]), maxrel(step[2], padded[2]), max(diffs)[0], max(diffs)[1]))


def test_every_frame_valid(dev, monkeypatch):
    """Nothing to skip: Mq = roundup(B * T, 64) = 256 rows for 195 frames, the pack and the unpack copy every row."""
    ref = _oracle(FULL)
    x, ups, T = _inputs(FULL)
    m, cfg = _packed_model(dev, monkeypatch)
    step = VT._step(m, x, FULL, ups, dev)
    st, = m._vstates_train.values()
    assert sorted(k[-1] for k in st["plans"]) == [256, 256] and st["row0"].tolist() == [0, 65, 130, 195]
    _check_against_the_oracle(m, cfg, step, ref, FULL)


# ---- 2. zeros where nothing is valid -------------------------------------------------------------------------------------------------------
def test_zeros_where_no_frame_is_valid(dev, monkeypatch):
    x, ups, T = _inputs(LENGTHS)
    m, cfg = _packed_model(dev, monkeypatch)
    out, feats, emb, _ = VT._step(m, x, LENGTHS, ups, dev)
    d = _packed_set(m)
    B, E, C = len(LENGTHS), cfg.embed, cfg.conv_dim
    hb = next(iter(m._vstates_train.values()))["hb"]
    Mv, Mq = 203, 256
    for b, n in enumerate(LENGTHS):
        fr = cfg.conv_lens(n)
        Tb = fr[-1]
        assert (feats[b, Tb:] == 0).all() and feats[b, :Tb].abs().max() > 0
        assert (d["out_pad"].view(B, T, E)[b, Tb:] == 0).all()
        assert (hb["denc"][:B * T * E].view(B, T, E)[b, Tb:] == 0).all() and hb["denc"][:B * T * E].view(B, T, E)[b, :Tb].float().abs().max() > 0
        dxin = d["dxin_pad"].view(B, T, E)      # the unpacked d(xin[0])
        assert (dxin[b, Tb:] == 0).all() and dxin[b, :Tb].abs().max() > 0
        for buf in d["dx0_pad"]:      # d(x0) behind the positional convolution and zero_tail_rows
            assert (buf[:B * T * E].view(B, T, E)[b, Tb:] == 0).all()
        for i, t in enumerate(d["Ts"]):
            assert (d["dz"][i][:B * t * C].view(B, t, C)[b, fr[i]:] == 0).all(), (b, i)
            assert d["dz"][i][:B * t * C].view(B, t, C)[b, :fr[i]].float().abs().max() > 0
    # the rows of the packed stretch that belong to no utterance
    for dq in d["dqkv"]:
        assert (dq[Mv * 3 * E:Mq * 3 * E] == 0).all() and dq[:Mv * 3 * E].float().abs().max() > 0
    for f32buf, bfbuf in d["dx_rot"]:
        assert (f32buf[Mv * E:Mq * E] == 0).all() and (bfbuf[Mv * E:Mq * E] == 0).all()
        assert f32buf[:Mv * E].abs().max() > 0 and bfbuf[:Mv * E].float().abs().max() > 0
    for buf, w in ((d["d_ctx"], E), (d["d_out_pk"], E), (d["d_f"][0], cfg.ffn), (d["d_f"][1], cfg.ffn)):
        assert (buf[Mv * w:Mq * w] == 0).all() and buf[:Mv * w].float().abs().max() > 0
    for n in range(cfg.layers):      # forward: the attention writes zeros there, everything else stays finite
        assert (d["ctx"][n][Mv * E:Mq * E] == 0).all()
        assert all(torch.isfinite(d[k][n][:Mq * E].float()).all() for k in ("xin", "x1", "h1", "h2"))


# ---- 3. what the padding holds does not matter ---------------------------------------------------------------------------------------------
def test_padding_content_does_not_change_a_bit(dev, monkeypatch):
    x, ups, _ = _inputs(LENGTHS)
    m, _ = _packed_model(dev, monkeypatch)
    base = VT._step(m, x, LENGTHS, ups, dev)
    noisy = x.clone()
    gen = torch.Generator().manual_seed(3)
    for b, n in enumerate(LENGTHS):
        noisy[b, n:] = torch.randn(x.shape[1] - n, generator=gen)
    again = VT._step(m, noisy, LENGTHS, ups, dev)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    assert base[3].abs().max() > 0


# ---- 4. plans follow the lengths ------------------------------------------------------------------------------------------------------------
def test_recorded_plans_follow_the_lengths_and_the_row_count(dev, monkeypatch):
    x, ups, T = _inputs(LENGTHS)
    m, cfg = _packed_model(dev, monkeypatch)
    first = VT._step(m, x, LENGTHS, ups, dev)                 # 203 rows: records the plans of Mq = 256
    narrow = [4000] * 5 + [20880]                            # 5 x 12 + 65 = 125 rows: another bucket, Mq = 128
    second = VT._step(m, x, narrow, ups, dev)
    same_bucket = [20880, 20880, 20880, 400, 400, 400]       # 3 x 65 + 3 = 198 rows: other lengths, the plans of Mq = 256 replayed
    third = VT._step(m, x, same_bucket, ups, dev)
    fourth = VT._step(m, x, LENGTHS, ups, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, fourth))
    assert not torch.equal(first[3], second[3]) and not torch.equal(first[3], third[3])
    for lengths, r in ((narrow, second), (same_bucket, third)):
        for b, n in enumerate(lengths):
            assert (r[1][b, cfg.conv_lens(n)[-1]:] == 0).all()
    st, = m._vstates_train.values()
    assert sorted((k[0], k[-1]) for k in st["plans"]) == [("bwd", 128), ("bwd", 256), ("fwd", 128), ("fwd", 256)]      # one per (direction, Mq)
    _packed_set(m)
    # the other lengths of the same bucket against the padded path's bar on the oracle: a replayed plan computes the right thing
    x3, ups3, _ = _inputs(same_bucket)
    _check_against_the_oracle(m, cfg, VT._step(m, x3, same_bucket, ups3, dev), _oracle(same_bucket), same_bucket)
    assert len(st["plans"]) == 4
    # a padded-path step of the same shape in between keeps its own state and buffers, and the packed one is untouched by it
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    VT._step(m, x, LENGTHS, ups, dev)
    assert len(m._vstates_train) == 2 and len(m.encoder._vbufs_train) == 2
    pst = m._vstates_train[(len(LENGTHS), max(LENGTHS))]
    assert len(pst["plans"]) == 2 and pst["row0"] is None
    monkeypatch.setattr(ENC, "VARLEN_PACK", True)
    fifth = VT._step(m, x, LENGTHS, ups, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, fifth))
    assert len(st["plans"]) == 4 and len(m._vstates_train) == 2 and len(m.encoder._vbufs_train) == 2


# ---- 5. every dropout on ---------------------------------------------------------------------------------------------------------------------
def test_packed_training_step_with_every_dropout_on(dev, monkeypatch):
    x, ups, T = _inputs(LENGTHS)
    m, cfg = _packed_model(dev, monkeypatch, head_drop=0.5, dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, dropout_input=0.1)
    runs = []
    for seed in (1234, 99, 1234):      # the first records, the others replay with their own seeds
        m._step_seed = seed
        runs.append(VT._step(m, x, LENGTHS, ups, dev))
    for r in runs:
        assert all(torch.isfinite(t).all() for t in r)
        for b, n in enumerate(LENGTHS):
            assert (r[1][b, cfg.conv_lens(n)[-1]:] == 0).all()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))      # repeatable for a fixed seed
    assert not torch.equal(runs[0][3], runs[1][3]) and not torch.equal(runs[0][0], runs[1][0])      # and the masks are drawn
    d = _packed_set(m)
    for dq in d["dqkv"]:
        assert (dq[203 * 3 * cfg.embed:256 * 3 * cfg.embed] == 0).all()


@pytest.mark.parametrize("case", ["fixed", "padded", "packed", "tiny"])
def test_a_replayed_step_is_bit_for_bit_the_recorded_step_of_its_seed(dev, monkeypatch, case):
    """The per-step values of a launch plan (the encoder's site seeds, the head's three seeds) are patched into every recorded call that
    carries one: model A records a train step at one step seed and replays it at another; model B, same weights and fresh states, records
    its first step at that other seed.  A's second step and B's first issue the same launches with the same seeds, so the outputs and the
    whole flat gradient buffer are equal bit for bit.  Every dropout on (the encoder's four at 0.1, the head's at its 0.5).  The six
    utterances as a fixed batch (65 frames: the fused attention kernel), padded and packed (the streaming kernels); `tiny`: the 5 x 9000
    fixed batch of tools/launch_log.py, 16-wide heads, so the materialised scores and scl_dropout_rows."""
    monkeypatch.setattr(ENC, "VARLEN_PACK", case == "packed")
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    drops = dict(dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, dropout_input=0.1)
    if case == "tiny":
        cfg, lengths = W2VConfig.tiny(), None
        vars(cfg).update(drops)
        gen = torch.Generator().manual_seed(5)
        B, T = 5, cfg.conv_lens(9000)[-1]
        x = 0.1 * torch.randn(B, 9000, generator=gen)
        ups = (0.3 * torch.randn(B, 2, generator=gen), 0.01 * torch.randn(B, T, 128, generator=gen), 0.05 * torch.randn(B, 128, generator=gen))
    else:
        cfg, lengths = W2VConfig(**SMALL, **drops), (None if case == "fixed" else LENGTHS)
        x, ups, T = _inputs(LENGTHS)

    def step(m, seed):
        m._step_seed = seed
        return VT._step(m, x, lengths, ups, dev)

    def plans(m):
        st, = (m._states if lengths is None else m._vstates_train).values()
        return st["plans"]
    a, b = (ML.Model(VT.ARGS, dev, w2v_cfg=cfg).train() for _ in range(2))
    assert torch.equal(a.P.flat, b.P.flat)
    first = step(a, 1234)
    recorded = {k: len(v["calls"]) for k, v in plans(a).items()}
    second = step(a, 99)
    fresh = step(b, 99)
    assert len(recorded) == 2 and {k: len(v["calls"]) for k, v in plans(a).items()} == recorded      # A's second step was a replay
    d, = (a.encoder._bufs if lengths is None else a.encoder._vbufs_train).values()
    assert (d["fused_attn"], d["long_attn"]) == {"fixed": (True, False), "tiny": (False, False)}.get(case, (False, True))
    for name, got, want in zip(("logp", "feats", "emb", "flat gradient"), second, fresh):
        assert torch.isfinite(got).all() and torch.equal(got, want), (case, name, (got != want).sum().item())
    assert second[3].abs().max() > 0 and not torch.equal(first[3], second[3]) and not torch.equal(first[0], second[0])      # masks are drawn anew


# ---- 6. bf16 scoring -------------------------------------------------------------------------------------------------------------------------
def test_packed_bf16_scoring(dev, monkeypatch):
    """Eval + no_grad + SCORE_FP32 off: the packed path against the oracle on each utterance alone, with the output bar; the padded
    path on the same batch for comparison (figures only)."""
    ref = _oracle(LENGTHS)
    x, _, T = _inputs(LENGTHS)
    m, cfg = _packed_model(dev, monkeypatch)
    monkeypatch.setattr(ML, "SCORE_FP32", False)
    m.eval()
    with torch.no_grad():
        out, feats, emb = m(x.to(dev), lengths=LENGTHS)
        again = m(x.to(dev), lengths=LENGTHS)      # the replay
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((out, feats, emb), again))
    keys = list(m.encoder._vbufs)
    assert keys == [(len(LENGTHS), max(LENGTHS), "packed")] and set(m._vstates) == set(keys) and not m.encoder._vbufs_train
    st, = m._vstates.values()
    assert [k[-1] for k in st["plans"]] == [256]
    _check_outputs(out, feats, emb, ref, LENGTHS, cfg, "packed scoring")
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    with torch.no_grad():
        pout, pfeats, pemb = m(x.to(dev), lengths=LENGTHS)
    torch.cuda.synchronize()
    _check_outputs(pout, pfeats, pemb, ref, LENGTHS, cfg, "padded scoring")
    print("packed vs padded scoring: max-rel logp %.2e feats %.2e emb %.2e" % (maxrel(out, pout), maxrel(feats, pfeats), maxrel(emb, pemb)))
    # the fp32 scoring path ignores the switch
    monkeypatch.setattr(ENC, "VARLEN_PACK", True)
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    with torch.no_grad():
        m(x.to(dev), lengths=LENGTHS)
    assert len(m.encoder._vbufs_f32) == 1 and len(m.encoder._vbufs) == 2


# ---- 7. main.py --padding_type zero --batch_size 2 with the switch on ---------------------------------------------------------------------------
def test_main_trains_zero_padded_packs_on_the_packed_path(dev, tmp_path, monkeypatch):
    import yaml
    import main as M
    monkeypatch.setattr(ENC, "VARLEN_PACK", True)
    monkeypatch.setattr(ENC, "PACK_ROWS", 64)
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    ids = ["u%d.wav" % i for i in range(3)]
    sizes = [2500, 9000, 4100]      # shorter and longer than trim_length
    os.makedirs(root / "scp", exist_ok=True)
    for sub, names in (("scp/train_bonafide.lst", ids[:2]), ("scp/dev_bonafide.lst", ids[1:]), ("scp/test.lst", ids)):      # a pack needs a second bona fide clip
        (root / sub).write_text("\n".join(names) + "\n")
    (root / "protocol.txt").write_text("")
    for u, n in zip(ids, sizes):
        VT._write_wav(str(root / "bonafide" / u), 0.1 * rs.randn(n))
        for j, v in enumerate(("hifigan", "waveglow")):
            VT._write_wav(str(root / "vocoded" / (v + "_" + u)), 0.1 * rs.randn(n - 700 + 1500 * j))
    trim = 6000
    cfg = {"model": {"name": "wav2vec2_linear_nll", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
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
    ctor = reg["wav2vec2_linear_nll"]

    def spy(*a, **k):
        m = ctor(*a, w2v_cfg=W2VConfig(**SMALL), **k)      # 64-wide heads (the YAML's tiny preset has 16-wide ones)
        inner = m.forward

        def forward(x, lengths=None):
            calls.append((bool(m.training), tuple(x.shape), None if lengths is None else list(lengths)))
            return inner(x, lengths)
        m.forward = forward
        made.append(m)
        return m
    reg["wav2vec2_linear_nll"] = spy
    monkeypatch.setattr(M, "MODEL_REGISTRY", reg)
    seen = []
    run_orig = M.run_epoch

    def run_rec(loader, model, optimizer, device, config, train):
        r = run_orig(loader, model, optimizer, device, config, train)
        seen.append((train, float(r[0])))
        return r
    monkeypatch.setattr(M, "run_epoch", run_rec)
    np.random.seed(0)
    rc = M.main(["--seed", "1", "--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--num_epochs", "1",
                 "--padding_type", "zero", "--comment", "zpk"])
    assert rc == 0
    assert [t for t, _ in seen] == [True, False] and all(np.isfinite(l) for _, l in seen), seen
    train_calls = [c for c in calls if c[0]]
    assert len(train_calls) == 1 and train_calls[0][1] == (14, trim) and min(train_calls[0][2]) < trim      # two packs of 7 views in one step
    mm = made[-1]
    assert list(mm.encoder._vbufs_train) == [(14, trim, "packed")] and list(mm._vstates_train) == [(14, trim, "packed")]
    st, = mm._vstates_train.values()
    assert sorted(k[0] for k in st["plans"]) == ["bwd", "fwd"] and all(k[-1] % 64 == 0 for k in st["plans"])
