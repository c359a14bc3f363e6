"""Variable-length scoring batches: zero-padded [B, L] plus per-utterance lengths (the counterpart of fairseq's padding_mask).
Kernels of csrc/attention_varlen.hip against fp64 and, bit for bit, against the fixed-length streaming kernel; the linear model on
both scoring paths against the CPU oracle run on each utterance ALONE at its own length; the refusals; main.py --padding_type none."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import lib as LIB  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.encoder import VARLEN_SETS, W2VConfig  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402

ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def close_bf16(got, ref):      # test_model_gpu.py's bar for outputs
    return rl2(got, ref) < 1e-2 and maxrel(got, ref) < 3e-2


def i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


# ---- 1. the streaming kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,T,klen", [(4, 2, 130, [1, 63, 64, 130]), (3, 4, 577, [577, 65, 512]), (2, 16, 224, [224, 17])])
def test_varlen_attention_against_fp64_and_bitwise_against_the_fixed_length_kernel(dev, B, H, T, klen):
    D, E = 64, H * 64
    scale = D ** -0.5
    gen = torch.Generator().manual_seed(T * 7 + H)
    clean = (0.7 * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16)
    qkv = clean.clone()
    for b, n in enumerate(klen):
        qkv[b, n:] = float("nan")      # Q, K and V rows at or beyond klen[b] must never be read
    qkv = qkv.to(dev)
    ctx = torch.full((B, T, E), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), float("nan"), device=dev)
    ops.attn_fwd_varlen(qkv, ctx, lse, i32(klen, dev), B, T, H, D, scale)
    torch.cuda.synchronize()
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(lse).all()
    for b, n in enumerate(klen):
        q, k, v = (clean[b, :n, i].double().permute(1, 0, 2) for i in range(3))      # [H, n, D]
        s = (q @ k.transpose(-1, -2)) * scale
        ref = (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(n, E)
        e_ctx, e_lse = rl2(ctx[b, :n], ref), rl2(lse[b, :, :n], torch.logsumexp(s, -1))
        print("T=%d klen=%d: ctx rel-L2 %.2e, lse rel-L2 %.2e" % (T, n, e_ctx, e_lse))
        assert e_ctx < 1.2e-2 and e_lse < 1e-5, (b, n, e_ctx, e_lse)
        blk = (n + 63) // 64 * 64      # first query block wholly beyond klen[b]
        assert (ctx[b, blk:] == 0).all() and (lse[b, :, blk:] == 0).all()
        # the utterance alone at T = klen[b] through the fixed-length kernel: the same key blocks in the same order per query
        alone = clean[b:b + 1, :n].contiguous().to(dev)
        c1 = torch.full((1, n, E), float("nan"), dtype=torch.bfloat16, device=dev)
        l1 = torch.full((1, H, n), float("nan"), device=dev)
        ops.attn_fwd_long(alone, c1, l1, 1, n, H, D, scale)
        torch.cuda.synchronize()
        assert torch.equal(ctx[b, :n], c1[0]) and torch.equal(lse[b, :, :n], l1[0])
    # every utterance full: the whole output is attn_fwd_long's
    full = clean.to(dev)
    c0, l0 = torch.full_like(ctx, float("nan")), torch.full_like(lse, float("nan"))
    c2, l2 = torch.full_like(ctx, float("nan")), torch.full_like(lse, float("nan"))
    ops.attn_fwd_long(full, c0, l0, B, T, H, D, scale)
    ops.attn_fwd_varlen(full, c2, l2, i32([T] * B, dev), B, T, H, D, scale)
    torch.cuda.synchronize()
    assert torch.equal(c0, c2) and torch.equal(l0, l2)


# ---- 2. the fp32 soft-max and the two small kernels -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,T,Tp,klen", [(3, 2, 70, 72, [1, 64, 70]), (3, 1, 600, 600, [600, 513, 3])])
def test_varlen_f32_softmax_against_fp64(dev, B, H, T, Tp, klen):
    gen = torch.Generator().manual_seed(T)
    S = 4.0 * torch.randn(B, H * T, Tp, generator=gen)
    junk = 1e3 * (2.0 * torch.randint(0, 2, (B, H * T, Tp), generator=gen) - 1.0)
    for b, n in enumerate(klen):
        S[b, :, n:] = junk[b, :, n:]      # columns at or beyond klen (pad columns included) hold +-1e3
    Sd = S.to(dev)
    P = torch.full((B, H * T, Tp), float("nan"), device=dev)
    ops.softmax_fwd_f32_varlen(Sd, P, i32(klen, dev), B * H * T, H * T, T, Tp, Tp)
    torch.cuda.synchronize()
    for b, n in enumerate(klen):
        ref = torch.softmax(S[b, :, :n].double(), -1)
        e = maxrel(P[b, :, :n], ref)
        print("T=%d klen=%d: soft-max max-rel %.2e" % (T, n, e))
        assert e < 1e-5, (b, n, e)
        assert (P[b, :, n:] == 0).all()
    # a chunk of the batch: utterances 1.. with the counts read from klen + 1 (what the encoder's chunk loop passes)
    P2 = torch.full((B - 1, H * T, Tp), float("nan"), device=dev)
    ops.softmax_fwd_f32_varlen(Sd[1:].contiguous(), P2, i32(klen, dev), (B - 1) * H * T, H * T, T, Tp, Tp, klen_offset=1)
    torch.cuda.synchronize()
    assert torch.equal(P2, P[1:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_tail_rows_and_varlen_mean_pool(dev, dtype):
    B, T, C, lens = 4, 37, 128, [1, 2, 36, 37]
    x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(9)).to(dtype)
    poisoned = x.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:] = float("nan")      # the mean must not read beyond the utterance's frames
    emb = torch.full((B, C), float("nan"), device=dev)
    ops.meanpool_fwd_varlen(poisoned.to(dev), emb, i32(lens, dev), B, T, C)
    xd = x.to(dev)
    ops.zero_tail_rows(xd, i32(lens, dev), B, T, C)
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        assert torch.equal(xd[b, :n].cpu(), x[b, :n]) and (xd[b, n:] == 0).all()
        # fp32 summation of n exactly loaded terms, u = 2^-24: |error of the sum| <= (n - 1) u sum|x|, the division adds u |mean|;
        # together at most u sum|x| (first order; 1 % on top for the higher-order terms)
        ref = x[b, :n].double().mean(0)
        bound = 1.01 * 2.0 ** -24 * x[b, :n].double().abs().sum(0) + 1e-30
        assert ((emb[b].double().cpu() - ref).abs() <= bound).all()


# ---- 3. the model against the oracle run on each utterance alone ---------------------------------------------------------------------
def _small_model(dev, cfg_kw=None):
    ocfg = W.W2VConfig(**SMALL)
    cfg = W2VConfig(**SMALL, **(cfg_kw or {}))
    ssl, head = W.init_state(ocfg, seed=41), OH.init_head(ocfg.embed, seed=42)
    m = Model(ARGS, dev, w2v_cfg=cfg)
    sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
    sd.update(head)
    m.load_state_dict(sd, strict=False)
    return m, ssl, head, ocfg, cfg


BATCHES = {"A": [400, 720, 20799, 41000, 64600],      # 1, 2, 64, 127 and 201 frames
           "B": [170000, 64600, 200000]}              # 531, 201 and 624 frames: looped soft-max, chunks above 512 frames, streaming kernel
_REFS = {}


def _batch_and_refs(name):
    """The zero-padded batch and the oracle's (log-probs, feats, emb) of every utterance alone; computed once, never modified."""
    if name not in _REFS:
        lengths = BATCHES[name]
        ocfg = W.W2VConfig(**SMALL)
        ssl, head = W.init_state(ocfg, seed=41), OH.init_head(ocfg.embed, seed=42)
        gen = torch.Generator().manual_seed(len(lengths))
        x = torch.zeros(len(lengths), max(lengths))
        refs = []
        for b, n in enumerate(lengths):
            x[b, :n] = 0.1 * torch.randn(n, generator=gen)
            with torch.no_grad():
                refs.append(tuple(t.clone() for t in OH.full_forward(ssl, head, ocfg, x[b:b + 1, :n].clone())))
        _REFS[name] = (x, refs)
    return _REFS[name]


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_padded_batch_with_lengths_matches_the_oracle_on_each_utterance_alone(dev, monkeypatch, name, fp32):
    monkeypatch.setattr(ML, "SCORE_FP32", fp32)
    x, refs = _batch_and_refs(name)
    lengths = BATCHES[name]
    m, _, _, _, cfg = _small_model(dev)
    if name == "B":      # fp32 path: two utterances per attention chunk, so the second chunk reads its counts at an offset
        T, H = cfg.conv_lens(x.shape[1])[-1], cfg.heads
        monkeypatch.setattr(ENC, "F32_ATTN_CHUNK_BYTES", 2 * 4 * H * T * ((T + 7) // 8 * 8))
    m.eval()
    with torch.no_grad():
        out, feats, emb = m(x.to(dev), lengths=lengths)
        torch.cuda.synchronize()
    T = cfg.conv_lens(x.shape[1])[-1]
    assert feats.shape == (len(lengths), T, 128)
    if name == "B":
        assert T > 512
    for b, n in enumerate(lengths):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = refs[b]
        assert rf.shape[1] == Tb
        assert (feats[b, Tb:] == 0).all()
        if fp32:      # the project's scoring bar
            errs = (maxrel(out[b], ro[0]), maxrel(emb[b], re[0]), maxrel(feats[b, :Tb], rf[0]))
            print("fp32 %s n=%d (%d frames): max-rel logp %.2e emb %.2e feats %.2e" % ((name, n, Tb) + errs))
            assert max(errs) < 1e-3, (n, errs)
        else:
            errs = [(rl2(g, r), maxrel(g, r)) for g, r in ((out[b], ro[0]), (emb[b], re[0]), (feats[b, :Tb], rf[0]))]
            print("bf16 %s n=%d (%d frames): (rel-L2, max-rel) logp %s emb %s feats %s" % ((name, n, Tb) + tuple("(%.2e, %.2e)" % e for e in errs)))
            assert close_bf16(out[b], ro[0]) and close_bf16(emb[b], re[0]) and close_bf16(feats[b, :Tb], rf[0]), (n, errs)
    if not fp32:      # the recorded plan reads the counts from the state's buffer: a replay with other lengths follows them
        other = [max(400, n // 2) for n in lengths]
        with torch.no_grad():
            o2, f2, e2 = m(x.to(dev), lengths=other)
            o3, f3, e3 = m(x.to(dev), lengths=lengths)
            torch.cuda.synchronize()
        assert torch.equal(o3, out) and torch.equal(e3, emb) and torch.equal(f3, feats)
        assert not torch.equal(e2, emb) and (f2[0, cfg.conv_lens(other[0])[-1]:] == 0).all()


# ---- 4. XLS-R-300M shape ---------------------------------------------------------------------------------------------------------
def test_xlsr_shape_two_clips_of_different_length_fp32_scoring(dev, monkeypatch):
    monkeypatch.setattr(ML, "SCORE_FP32", True)
    ocfg = W.W2VConfig()
    ssl, head = W.init_state(ocfg, seed=81), OH.init_head(ocfg.embed, seed=82)
    m = Model(ARGS, dev, w2v_cfg=W2VConfig())
    sd = {"ssl_model.model." + k: v for k, v in ssl.items()}
    sd.update(head)
    m.load_state_dict(sd, strict=False)
    m.eval()
    lengths = [48000, 16000]      # 149 and 49 frames
    x = torch.zeros(2, 48000)
    gen = torch.Generator().manual_seed(77)
    for b, n in enumerate(lengths):
        x[b, :n] = 0.1 * torch.randn(n, generator=gen)
    with torch.no_grad():
        out, feats, emb = m(x.to(dev), lengths=lengths)
        torch.cuda.synchronize()
        for b, n in enumerate(lengths):
            Tb = W2VConfig().conv_lens(n)[-1]
            ro, rf, re = OH.full_forward(ssl, head, ocfg, x[b:b + 1, :n].clone())
            errs = (maxrel(out[b], ro[0]), maxrel(emb[b], re[0]), maxrel(feats[b, :Tb], rf[0]))
            print("XLS-R n=%d (%d frames): max-rel logp %.2e emb %.2e feats %.2e" % ((n, Tb) + errs))
            assert max(errs) < 1e-3, (n, errs)
            assert (feats[b, Tb:] == 0).all()


# ---- 5. refusals, and the bound on live buffer sets ---------------------------------------------------------------------------------
def test_lengths_are_refused_under_autograd_in_train_mode_and_by_the_other_plugins(dev):
    from scl_amd.model_aasist import Model as Aasist
    m, _, _, _, _ = _small_model(dev)
    x = torch.zeros(2, 4000, device=dev)
    m.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(x, lengths=[4000, 1000])
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
        m(x, lengths=[4000, 1000])
    m.eval()
    with torch.no_grad():
        for bad in ([4000], [4000, 0], [4000, 4001]):
            with pytest.raises(ValueError, match="lengths"):
                m(x, lengths=bad)
    a = Aasist(ARGS, dev, w2v_cfg=W2VConfig.tiny())
    a.eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="wav2vec2_linear_nll"):
        a(x, lengths=[4000, 1000])


def test_frame_counts_outside_1_to_T_are_an_error_code_from_the_library():
    L = LIB.load()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert L.scl_varlen_check_lengths(arr(1, 12, 5), 3, 12) == 0
    assert L.scl_varlen_check_lengths(arr(3, 0), 2, 12) == -1 and b"outside 1..12" in L.scl_last_error()
    assert L.scl_varlen_check_lengths(arr(13), 1, 12) == -1
    with pytest.raises(SclError, match="outside 1..12"):
        ops.check_lengths([5, 13], 12)
    assert ops.check_lengths([5, 12], 12) == [5, 12]


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "bf16"])
def test_variable_length_buffer_sets_are_bounded_and_survive_eviction(dev, monkeypatch, fp32):
    monkeypatch.setattr(ML, "SCORE_FP32", fp32)
    m, _, _, _, _ = _small_model(dev)
    m.eval()
    shapes = [(2, 1600 * k) for k in range(1, VARLEN_SETS + 3)]
    first = {}
    with torch.no_grad():
        for rnd in range(2):      # the second round re-creates the evicted sets (and re-records their plans)
            for B, L in shapes:
                x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(L))).to(dev)
                x[1, L // 2:] = 0
                res = [t.clone() for t in m(x, lengths=[L, L // 2])]
                if rnd == 0:
                    first[(B, L)] = res
                else:
                    assert all(torch.equal(a, b) for a, b in zip(res, first[(B, L)]))
                assert len(m.encoder._vbufs) <= VARLEN_SETS and len(m.encoder._vbufs_f32) <= VARLEN_SETS and len(m._vstates) <= VARLEN_SETS
    live = m.encoder._vbufs_f32 if fp32 else m.encoder._vbufs
    assert len(live) == VARLEN_SETS and (fp32 or set(m._vstates) == set(live))
    assert not m.encoder._bufs and not m._states and not m._hbufs      # nothing in the keep-forever tables


# ---- 6. main.py --eval --padding_type none -------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_eval_padding_type_none_scores_whole_utterances_in_protocol_order(dev, tmp_path, monkeypatch):
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
    cfg = {"model": {"name": "wav2vec2_linear_nll", "flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1, "w2v_arch": "tiny"},
           "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ref_model = M.MODEL_REGISTRY["wav2vec2_linear_nll"](cfg["model"], dev, seed=5)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    want_lp, want_emb = [], []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            o, _, e = ref_model(x[None].to(dev), lengths=[n])
            want_lp.append(o[0].cpu().numpy()); want_emb.append(e[0].cpu().numpy())
    made = []
    reg = dict(M.MODEL_REGISTRY)
    ctor = reg["wav2vec2_linear_nll"]
    reg["wav2vec2_linear_nll"] = lambda *a, **k: made.append(ctor(*a, **k)) or made[-1]
    monkeypatch.setattr(M, "MODEL_REGISTRY", reg)
    common = ["--config", str(cfg_path), "--database_path", str(root), "--batch_size", "2", "--eval", "--model_path", str(ck),
              "--padding_type", "none"]
    relerr = lambda got, ref: np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()
    # scores
    out = tmp_path / "scores.txt"
    assert M.main(common + ["--eval_output", str(out)]) == 0
    lines = out.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids      # exactly five lines, protocol order, the 3000-sample file included
    for l, ref in zip(lines, want_lp):
        assert relerr([float(v) for v in l.split()[1:]], ref) < 1e-3, (l, ref)
    mm = made[-1]
    assert 1 <= len(mm.encoder._vbufs_f32) + len(mm.encoder._vbufs) <= VARLEN_SETS and not mm.encoder._bufs      # 70000 samples included
    # --predict
    pred = tmp_path / "pred.txt"
    assert M.main(common + ["--predict", "--eval_output", str(pred)]) == 0
    lines = pred.read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for l, ref in zip(lines, want_lp):
        assert abs(float(l.split()[1]) - ref[1]) <= 1e-3 * np.abs(ref).max() and int(l.split()[2]) == int(ref.argmax())
    # --emb
    embd = tmp_path / "emb"
    assert M.main(common + ["--emb", "--eval_output", str(embd)]) == 0
    lines = (embd / "scores.txt").read_text().strip().split("\n")
    assert [l.split()[0] for l in lines] == ids
    for u, ref in zip(ids, want_emb):
        assert relerr(np.load(str(embd / (u.split(".")[0] + ".npy"))), ref) < 1e-3, u
    # the other plugins are refused at start-up
    cfg["model"]["name"] = "wav2vec2_aasist"
    cfg_path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit) as e:
        M.main(common + ["--eval_output", str(tmp_path / "x.txt")])
    assert "wav2vec2_linear_nll only" in str(e.value)
