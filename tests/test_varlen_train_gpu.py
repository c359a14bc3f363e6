"""Training on zero-padded batches: the padding mask through the backward.
Kernels of csrc/attention_varlen.hip (scl_attn_bwd_varlen, the dropout forward, scl_meanpool_bwd_varlen) against fp64 with a key mask
and, bit for bit, against the fixed-length streaming kernels on each utterance alone; the linear model in train mode with `lengths`
against the CPU oracle's autograd on each utterance alone; padding content, plan replay with other lengths, dropout; main.py with
--padding_type zero --batch_size 2."""
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from scl_amd.model_linear import Model  # noqa: E402
from oracle import head as OH  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from tests.attention_cases import keep_scale  # noqa: E402

ARGS = {"flag_fix_ssl": False, "contra_mode": "all", "loss_type": 1}
# the tiny encoder with 64-wide heads (the tiny preset's are 16 wide, and variable-length batches run the streaming attention, which
# takes head dim 64): tests/test_varlen_gpu.py's configuration
SMALL = dict(conv_dim=32, embed=128, layers=2, heads=2, ffn=256, pos_k=16, pos_groups=4, final_dim=16, latent_vars=8, latent_groups=2)


def rl2(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def maxrel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


SHAPES = [(4, 2, 130, [1, 63, 64, 130]), (3, 4, 577, [577, 65, 512]), (2, 16, 224, [224, 17]),
          (4, 2, 300, [33, 128, 129, 300])]      # the last one straddles the 32-row query tile and the 128-key dK / dV block


def _nan_tail(t, klen, dim=1):
    t = t.clone()
    for b, n in enumerate(klen):
        t[b].narrow(dim - 1, n, t.shape[dim] - n).fill_(float("nan"))
    return t


# ---- 1. the kernels against fp64 attention with a key mask --------------------------------------------------------------------------
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,T,klen", SHAPES)
def test_varlen_attention_backward_against_fp64_with_a_key_mask(dev, B, H, T, klen, drop_p):
    D, E = 64, H * 64
    seed, scale = 0x2468ACE, D ** -0.5
    gen = torch.Generator().manual_seed(T * 7 + H)
    clean = (0.7 * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16)
    dclean = torch.randn(B, T, E, generator=gen).to(torch.bfloat16)
    qkv, dctx, kl = clean.to(dev), dclean.to(dev), i32(klen, dev)
    ctx = torch.full((B, T, E), float("nan"), dtype=torch.bfloat16, device=dev)
    lse = torch.full((B, H, T), float("nan"), device=dev)
    ops.attn_fwd_varlen_drop(qkv, ctx, lse, kl, B, T, H, D, scale, drop_p=drop_p, drop_seed=seed)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    dqkv = torch.full((B, T, 3, H, D), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.attn_bwd_varlen(qkv, ctx, dctx, lse, kl, dqkv, ws, B, T, H, D, scale, drop_p=drop_p, drop_seed=seed)
    dq2 = torch.full_like(dqkv, float("nan"))
    ops.attn_bwd_varlen(qkv, ctx, dctx, lse, kl, dq2, ws, B, T, H, D, scale, drop_p=drop_p, drop_seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(dq2, dqkv)      # deterministic: two runs, the same bits
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(ctx.float()).all()
    # the mask index of the fixed-length kernels with the padded T: ((b*H + h)*T + q)*T + k
    keep = keep_scale(seed, B * H * T * T, drop_p).view(B, H, T, T).double() if drop_p > 0 else None
    for b, n in enumerate(klen):
        q, k, v = (clean[b, :n, i].double().permute(1, 0, 2).clone().requires_grad_(True) for i in range(3))      # [H, n, D]
        s = (q @ k.transpose(-1, -2)) * scale
        pr = torch.softmax(s, -1)
        if keep is not None:
            pr = pr * keep[b, :, :n, :n]
        ref = (pr @ v).permute(1, 0, 2).reshape(n, E)
        ref.backward(dclean[b, :n].double())
        e_ctx = rl2(ctx[b, :n], ref)
        errs = []
        for i, gr in enumerate((q.grad, k.grad, v.grad)):
            got = dqkv[b, :n, i].permute(1, 0, 2)
            if n == 1 and i < 2:      # one key: dq and dk are exactly 0; the kernel leaves bf16 round-off of dP - delta (as at T = 1)
                assert got.double().abs().max().item() <= 1e-2 * v.grad.abs().max().item()
                errs.append(float("nan"))
                continue
            errs.append(rl2(got, gr))
        print("T=%d klen=%d p=%.1f: ctx rel-L2 %.2e, dq %.2e dk %.2e dv %.2e" % (T, n, drop_p, e_ctx, errs[0], errs[1], errs[2]))
        assert e_ctx < 1.2e-2, (b, n, e_ctx)
        assert all(not (e >= 2.5e-2) for e in errs), (b, n, errs)
        assert (dqkv[b, n:] == 0).all() and (ctx[b, n:] == 0).all() and (lse[b, :, n:] == 0).all()


# ---- 2. bit identity with the fixed-length kernel on the utterance alone; rows beyond klen are never loaded ---------------------------
@pytest.mark.parametrize("B,H,T,klen", SHAPES)
def test_varlen_attention_backward_carries_the_bits_of_the_fixed_length_kernel(dev, B, H, T, klen):
    D, E = 64, H * 64
    scale = D ** -0.5
    gen = torch.Generator().manual_seed(T * 11 + H)
    clean = (0.7 * torch.randn(B, T, 3, H, D, generator=gen)).to(torch.bfloat16)
    dclean = torch.randn(B, T, E, generator=gen).to(torch.bfloat16)
    kl = i32(klen, dev)
    qkv, dctx = clean.to(dev), dclean.to(dev)
    ctx = torch.zeros(B, T, E, dtype=torch.bfloat16, device=dev)
    lse = torch.zeros(B, H, T, device=dev)
    ops.attn_fwd_varlen(qkv, ctx, lse, kl, B, T, H, D, scale)
    ws = torch.empty(ops.attn_long_ws_bytes(B, T, H), dtype=torch.uint8, device=dev)
    dqkv = torch.full((B, T, 3, H, D), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.attn_bwd_varlen(qkv, ctx, dctx, lse, kl, dqkv, ws, B, T, H, D, scale)
    # the same inputs with NaN in every row at or beyond klen[b] (qkv, ctx, dctx, lse): the same bits, so none of them is loaded
    lse_nan = lse.clone()
    for b, n in enumerate(klen):
        lse_nan[b, :, n:] = float("nan")
    dq_nan = torch.full_like(dqkv, float("nan"))
    ops.attn_bwd_varlen(_nan_tail(qkv, klen), _nan_tail(ctx, klen), _nan_tail(dctx, klen), lse_nan, kl, dq_nan, ws, B, T, H, D, scale)
    torch.cuda.synchronize()
    assert torch.equal(dq_nan, dqkv)
    for b, n in enumerate(klen):
        alone = clean[b:b + 1, :n].contiguous().to(dev)
        c1 = torch.empty(1, n, E, dtype=torch.bfloat16, device=dev)
        l1 = torch.empty(1, H, n, device=dev)
        ops.attn_fwd_long(alone, c1, l1, 1, n, H, D, scale)
        d1 = torch.full((1, n, 3, H, D), float("nan"), dtype=torch.bfloat16, device=dev)
        w1 = torch.empty(ops.attn_long_ws_bytes(1, n, H), dtype=torch.uint8, device=dev)
        ops.attn_bwd_long(alone, c1, dclean[b:b + 1, :n].contiguous().to(dev), l1, d1, w1, 1, n, H, D, scale)
        torch.cuda.synchronize()
        assert torch.equal(dqkv[b, :n], d1[0]), (b, n)
        assert (dqkv[b, n:] == 0).all()
    # every utterance full: the whole gradient is scl_attn_bwd_long's
    full = i32([T] * B, dev)
    c0, l0 = torch.empty_like(ctx), torch.empty_like(lse)
    ops.attn_fwd_long(qkv, c0, l0, B, T, H, D, scale)
    d0, d2 = torch.full_like(dqkv, float("nan")), torch.full_like(dqkv, float("nan"))
    ops.attn_bwd_long(qkv, c0, dctx, l0, d0, ws, B, T, H, D, scale)
    ops.attn_bwd_varlen(qkv, c0, dctx, l0, full, d2, ws, B, T, H, D, scale)
    torch.cuda.synchronize()
    assert torch.equal(d0, d2)


def test_varlen_attention_backward_refuses_other_head_dims(dev):
    z = torch.zeros(4096, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(4096, device=dev)
    ws = torch.empty(4096, dtype=torch.uint8, device=dev)
    with pytest.raises(SclError, match="head dim 64"):
        ops.attn_bwd_varlen(z, z, z, f, i32([4], dev), z, ws, 1, 4, 2, 32, 0.1)
    with pytest.raises(SclError, match="head dim 64"):
        ops.attn_fwd_varlen_drop(z, z, f, i32([4], dev), 1, 4, 2, 32, 0.1, drop_p=0.1, drop_seed=1)


# ---- 3. the mean pool's backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("drop_p", [0.0, 0.5])
def test_varlen_mean_pool_backward(dev, dtype, drop_p):
    B, T, C, lens, seed = 4, 37, 128, [1, 2, 36, 37], 77
    gen = torch.Generator().manual_seed(5)
    pre = torch.randn(B, T, C, generator=gen).to(dtype)
    demb = torch.randn(B, C, generator=gen)
    dpre = torch.full((B, T, C), float("nan"), dtype=dtype, device=dev)
    ops.meanpool_bwd_varlen(demb.to(dev), _nan_tail(pre, lens).to(dev), dpre, i32(lens, dev), B, T, C, 3, drop_p=drop_p, seed=seed)
    torch.cuda.synchronize()
    keep = keep_scale(seed, B * T * C, drop_p).view(B, T, C).double() if drop_p > 0 else torch.ones(B, T, C, dtype=torch.float64)
    slope = torch.where(pre.double() > 0, 1.0, 0.01)      # LeakyReLU's derivative (activation id 3)
    for b, n in enumerate(lens):
        ref = (demb[b].double() / n)[None, :] * keep[b, :n] * slope[b, :n]
        # f32: the division and two products, 3 roundings of 2^-24 each; bf16: one more rounding of the output, 2^-8
        tol = 2.0 ** -22 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
        assert ((dpre[b, :n].double().cpu() - ref).abs() <= tol * ref.abs() + 1e-30).all(), (b, n)
        assert (dpre[b, n:] == 0).all()
    if drop_p == 0:      # every utterance full: scl_meanpool_bwd's bits
        a = torch.empty(B, T, C, dtype=dtype, device=dev)
        c = torch.empty(B, T, C, dtype=dtype, device=dev)
        ops.meanpool_bwd(demb.to(dev), pre.to(dev), a, B, T, C, 3)
        ops.meanpool_bwd_varlen(demb.to(dev), pre.to(dev), c, i32([T] * B, dev), B, T, C, 3)
        torch.cuda.synchronize()
        assert torch.equal(a, c)


# ---- 4. the model in train mode: a padded batch against the oracle's autograd on each utterance alone ----------------------------------
LENGTHS = [12000, 4000, 7777, 400]      # 37, 12, 24 and 1 frames
_ORACLE = {}


def _inputs():
    """The zero-padded batch and fixed upstream gradients (d_out, d_feats, d_emb); d_feats is non-zero in the padded rows too.  Their
    sizes are those the loss hands back on such a batch (d_out O(1/B), the SupCon terms one to two orders below)."""
    cfg = W2VConfig(**SMALL)
    gen = torch.Generator().manual_seed(2024)
    B, L = len(LENGTHS), max(LENGTHS)
    T = cfg.conv_lens(L)[-1]
    x = torch.zeros(B, L)
    for b, n in enumerate(LENGTHS):
        x[b, :n] = 0.1 * torch.randn(n, generator=gen)
    ups = (0.3 * torch.randn(B, 2, generator=gen), 0.01 * torch.randn(B, T, 128, generator=gen), 0.05 * torch.randn(B, 128, generator=gen))
    return x, ups, T


def _oracle_alone():
    """CPU oracle, fp32 autograd: every utterance alone at its own length; the parameter gradients of <upstream, outputs> summed over
    the utterances, and each utterance's outputs.  Computed once, never modified."""
    if not _ORACLE:
        ocfg = W.W2VConfig(**SMALL)
        ssl, head = W.init_state(ocfg, seed=91), OH.init_head(ocfg.embed, seed=92)
        x, (d_out, d_feats, d_emb), _ = _inputs()
        params = {"ssl_model.model." + n: ssl[n] for n, _, tr in W.param_shapes(ocfg) if tr}
        params.update(head)
        for p in params.values():
            p.requires_grad_(True)
        outs = []
        for b, n in enumerate(LENGTHS):
            o, f, e = OH.full_forward(ssl, head, ocfg, x[b:b + 1, :n].clone())
            Tb = f.shape[1]
            ((o * d_out[b:b + 1]).sum() + (f * d_feats[b:b + 1, :Tb]).sum() + (e * d_emb[b:b + 1]).sum()).backward()
            outs.append((o.detach().clone(), f.detach().clone(), e.detach().clone()))
        grads = {k: p.grad.detach().clone() for k, p in params.items()}
        for p in params.values():
            p.requires_grad_(False)
            p.grad = None
        _ORACLE.update(grads=grads, outs=outs, ssl=ssl, head=head)
    return _ORACLE


def _train_model(dev, monkeypatch, head_drop=0.0, **enc_drop):
    monkeypatch.setattr(ML, "DROP_P", head_drop)
    rates = dict(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, dropout_input=0.0)
    rates.update(enc_drop)
    cfg = W2VConfig(**SMALL, **rates)
    ref = _oracle_alone()
    m = Model(ARGS, dev, w2v_cfg=cfg)
    sd = {"ssl_model.model." + k: v for k, v in ref["ssl"].items()}
    sd.update(ref["head"])
    m.load_state_dict(sd, strict=False)
    m.train()
    return m, cfg


def _step(m, x, lengths, ups, dev):
    out, feats, emb = m(x.to(dev), lengths=lengths)
    torch.autograd.backward([out, feats, emb], [u.to(dev) for u in ups])
    torch.cuda.synchronize()
    return out.detach().clone(), feats.detach().clone(), emb.detach().clone(), m.P.grad.clone()


def cosine(a, b):
    a = torch.as_tensor(a).float().cpu().flatten(); b = torch.as_tensor(b).float().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()


def relerr(got, ref):
    got, ref = torch.as_tensor(got).float().cpu(), torch.as_tensor(ref).float().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def test_padded_training_batch_gives_the_sum_of_each_utterance_alone(dev, monkeypatch):
    """Outputs and every parameter gradient of the padded batch in train mode against the CPU oracle's autograd on each utterance ALONE
    at its own length (gradients summed over the utterances), with the bars of test_every_parameter_gradient_matches_oracle_autograd:
    cosine > 0.99 and max error < 20 % of the tensor's max (25 % for the frame-level head), 2e-3 absolute where the reference is zero."""
    ref = _oracle_alone()
    x, ups, T = _inputs()
    m, cfg = _train_model(dev, monkeypatch)
    out, feats, emb, _ = _step(m, x, LENGTHS, ups, dev)
    assert m.encoder._vbufs_train and not m.encoder._vbufs and not m.encoder._bufs      # the training set: streaming attention, kept
    d = next(iter(m.encoder._vbufs_train.values()))
    assert d["long_attn"] and "attn_ws" in d and "S" not in d and "P" not in d and d["dS"] is None      # no T x T buffers
    for b, n in enumerate(LENGTHS):
        Tb = cfg.conv_lens(n)[-1]
        ro, rf, re = ref["outs"][b]
        errs = [(rl2(g, r), maxrel(g, r)) for g, r in ((out[b], ro[0]), (emb[b], re[0]), (feats[b, :Tb], rf[0]))]
        print("n=%d (%d frames): (rel-L2, max-rel) logp %s emb %s feats %s" % ((n, Tb) + tuple("(%.2e, %.2e)" % e for e in errs)))
        assert all(e[0] < 1e-2 and e[1] < 3e-2 for e in errs), (n, errs)      # test_model_gpu.py's bar for outputs
        assert (feats[b, Tb:] == 0).all()
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


def test_padded_rows_carry_exactly_zero_gradient_down_to_the_conv_stack(dev, monkeypatch):
    """The two masks (attention backward, d(x0) behind the positional convolution) make every padded row's gradient exactly 0: checked on
    the buffers of the backward itself, at every level that keeps its own buffer."""
    x, ups, T = _inputs()
    m, cfg = _train_model(dev, monkeypatch)
    _step(m, x, LENGTHS, ups, dev)
    d = next(iter(m.encoder._vbufs_train.values()))
    B, E, C = len(LENGTHS), cfg.embed, cfg.conv_dim
    hb = next(iter(m._vstates_train.values()))["hb"]
    for b, n in enumerate(LENGTHS):
        fr = cfg.conv_lens(n)
        Tb = fr[-1]
        assert (hb["denc"][:B * T * E].view(B, T, E)[b, Tb:] == 0).all()
        for dq in d["dqkv"]:
            assert (dq[:B * T * 3 * E].view(B, T, 3 * E)[b, Tb:] == 0).all()
        for f32buf, bfbuf in d["dx_rot"]:
            assert (f32buf.view(B, T, E)[b, Tb:] == 0).all() and (bfbuf[:B * T * E].view(B, T, E)[b, Tb:] == 0).all()
        for i, t in enumerate(d["Ts"]):      # the conv stack: frames of layer i that lie wholly inside the utterance's samples
            assert (d["dz"][i][:B * t * C].view(B, t, C)[b, fr[i]:] == 0).all(), (b, i)
            assert d["dz"][i][:B * t * C].view(B, t, C)[b, :fr[i]].float().abs().max() > 0


# ---- 5. what the padding holds does not matter ----------------------------------------------------------------------------------------
def test_padding_content_does_not_change_a_bit(dev, monkeypatch):
    x, ups, _ = _inputs()
    m, _ = _train_model(dev, monkeypatch)
    base = _step(m, x, LENGTHS, ups, dev)
    noisy = x.clone()
    gen = torch.Generator().manual_seed(3)
    for b, n in enumerate(LENGTHS):
        noisy[b, n:] = torch.randn(x.shape[1] - n, generator=gen)
    again = _step(m, noisy, LENGTHS, ups, dev)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    assert base[3].abs().max() > 0


# ---- 6. replay with other lengths; dropout --------------------------------------------------------------------------------------------
def test_recorded_plans_follow_the_lengths_of_each_step(dev, monkeypatch):
    x, ups, T = _inputs()
    m, cfg = _train_model(dev, monkeypatch)
    first = _step(m, x, LENGTHS, ups, dev)      # records the forward's and the backward's plan
    other = [4000, 12000, 400, 9000]
    second = _step(m, x, other, ups, dev)       # replays them with other frame counts
    third = _step(m, x, LENGTHS, ups, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, third))
    assert not torch.equal(first[3], second[3])
    for b, n in enumerate(other):
        assert (second[1][b, cfg.conv_lens(n)[-1]:] == 0).all()
    st, = m._vstates_train.values()
    assert len(st["plans"]) == 2 and len(m.encoder._vbufs_train) == 1      # one buffer set, one plan per direction
    # a fixed-length step of the same shape keeps its own state and buffers, and the padded one is untouched by it
    out, feats, emb = m(x.to(dev))
    torch.autograd.backward([out, feats, emb], [u.to(dev) for u in ups])
    fourth = _step(m, x, LENGTHS, ups, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, fourth))


def test_padded_training_step_with_every_dropout_on(dev, monkeypatch):
    x, ups, T = _inputs()
    m, cfg = _train_model(dev, monkeypatch, head_drop=0.5, dropout=0.1, attention_dropout=0.1, activation_dropout=0.1, dropout_input=0.1)
    runs = []
    for seed in (1234, 99, 1234):      # the first records, the others replay with their own seeds
        m._step_seed = seed
        runs.append(_step(m, x, LENGTHS, ups, dev))
    for r in runs:
        assert all(torch.isfinite(t).all() for t in r)
        for b, n in enumerate(LENGTHS):
            assert (r[1][b, cfg.conv_lens(n)[-1]:] == 0).all()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))      # repeatable for a fixed seed
    assert not torch.equal(runs[0][3], runs[1][3]) and not torch.equal(runs[0][0], runs[1][0])      # and the masks are drawn


def test_the_refusals_stay(dev, monkeypatch):
    m, _ = _train_model(dev, monkeypatch)
    x = torch.zeros(2, 4000, device=dev)
    m.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(x, lengths=[4000, 1000])
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
        m(x, lengths=[4000, 1000])
    with pytest.raises(ValueError, match="lengths"):
        m(x, lengths=[4000, 4001])
    with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
        m.encoder.forward(x, training=True, frames=i32([12, 3], dev))


# ---- 7. main.py --padding_type zero --batch_size 2 --------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_trains_and_validates_two_zero_padded_packs_per_step(dev, tmp_path, monkeypatch):
    import yaml
    import main as M
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    ids = ["u%d.wav" % i for i in range(7)]
    sizes = [2500, 9000, 4100, 6000, 3300, 7000, 5000]      # shorter and longer than trim_length
    os.makedirs(root / "scp", exist_ok=True)
    for sub, names in (("scp/train_bonafide.lst", ids[:4]), ("scp/dev_bonafide.lst", ids[4:]), ("scp/test.lst", ids)):
        (root / sub).write_text("\n".join(names) + "\n")
    (root / "protocol.txt").write_text("")
    for u, n in zip(ids, sizes):
        _write_wav(str(root / "bonafide" / u), 0.1 * rs.randn(n))
        for j, v in enumerate(("hifigan", "waveglow")):
            _write_wav(str(root / "vocoded" / (v + "_" + u)), 0.1 * rs.randn(n - 700 + 1500 * j))
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
            calls.append((bool(m.training), torch.is_grad_enabled(), tuple(x.shape), None if lengths is None else list(lengths)))
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
                 "--padding_type", "zero", "--comment", "zp"])
    assert rc == 0
    assert [t for t, _ in seen] == [True, False] and all(np.isfinite(l) for _, l in seen), seen
    V = 1 + 1 + 1 + 2 + 2      # the anchor, its RawBoost view, one more bona fide, two vocoded and their RawBoost views
    lo = made[-1].cfg.min_samples()
    train_calls = [c for c in calls if c[0]]
    val_calls = [c for c in calls if not c[0]]
    assert len(train_calls) == 2 and len(val_calls) == 2
    for training, grad, shape, lengths in calls:
        assert grad == training and lengths is not None and shape[1] == trim and len(lengths) == shape[0]
        assert all(lo <= n <= trim for n in lengths)
    assert all(min(c[3]) < trim for c in train_calls)      # 2500 and 4100 samples: each training step holds a clip shorter than the padding
    assert [c[2][0] for c in train_calls] == [2 * V, 2 * V] and sorted(c[2][0] for c in val_calls) == [V, 2 * V]
    mm = made[-1]
    assert len(mm._vstates_train) == 1 and len(mm.encoder._vbufs_train) == 1      # one shape: one buffer set, one recorded plan
