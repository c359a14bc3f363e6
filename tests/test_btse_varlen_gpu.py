"""Variable-length batches on the `wav2vec2_btse` plugin: whole utterances of different frame AND token counts in one zero-padded batch.

Row b gets what the plugin computes for that utterance ALONE at its own length with its own tokens (tests/test_btse_varlen_cpu.py pins that
definition on the CPU): the mean over time over its own frames, the bio score read at its OWN last token (scl_btse_bio_fwd_own /
_bwd_own — the reference's read-out at the last padded position, which the fixed-length entries keep, gives every shorter row a zero).
The float64 oracle (oracle/btse.py, identity LL as tests/test_btse_train_gpu.py sets it up) is always run PER UTTERANCE ALONE at its own
frames and tokens; gradients are summed over the utterances.

 1. the bio kernels through the C ABI (the plan's descriptor, ops.btse_bio_*_own): scores and every slab row against the oracle alone at
    token counts around the 64-row blocks of the rows and attention kernels, the window of 4 and the thirds of the relative-embedding
    sums; all counts full: bit-identical to the fixed-length entries; a count of 0: zeros; token ids beyond the counts, scratch last used
    by a launch of another token count or filled with NaN, NaN in slab / gbio: not one bit moves;
 2. the back-end (BtseHead.forward(..., frames=...)), eval and train mode (host-rebuilt MLP dropout masks, sliced per utterance), concat
    and is_add, two steps on one cached plan with other counts, poisoned plan buffers;
 3. the plugin: scoring on both precisions and both row layouts against the same model on each utterance alone, training (what x holds
    beyond the lengths reaches no bit; gradients against the CPU chain per utterance, summed), the refusals;
 4. main.py --eval --padding_type none: --batch_size 4 gives the scores of --batch_size 1.

Bars.  Kernels and back-end: the BARS of tests/test_btse_train_gpu.py (out 5e-7, out-max 1e-6, grad_x 1e-6, grad 1e-4, zero-grad 1e-7),
which were measured on gradients summed over 14 - 128 utterances of 199 tokens.  At the small shapes here three of them are missed by the
FIXED-LENGTH entries themselves, on full-length rows of the same sizes (tools/btse_small_shapes_probe.py, profiles/btse_varlen.txt: 12 rows
each of 1, 2, 4, 5, 9, 63 - 66, 70, 128 - 130 tokens, two weight seeds, concat and is_add, against float64): a single utterance's slab row
reaches 9.73e-4 per tensor (conv_k.weight of the last layer at 5 tokens; 1.2e-4 - 3.6e-4 at 63 - 130 tokens: only the read-out row's
query carries a gradient there, dS = P (g - delta) cancels, and the probabilities are recomputed with the fast exponential) and 6.81e-7
of the row's largest gradient on an analytically zero tensor; summed over the six utterances of the back-end test's two steps, 2.11e-4
(zero tensors 3.0e-7).  Those three bars are 3 x the measured values, as the fixed-length kernels set them, not the code under test: per
slab row grad 2.9e-3 and zero-grad 2.0e-6, back-end grad 6.3e-4; the other bars stand.  Measured with the own-last-token entries on the
MI355X: slab rows grad 2.2e-4, zero-grad 2.7e-7, scores 2.5e-7 / 2.6e-7; back-end grad 1.8e-4, zero-grad 3.1e-8, grad_x 4.1e-7, out
2.8e-7 / 4.3e-7.  A gradient tensor that is analytically zero for an utterance (conv_k.bias always: the soft-max is shift-invariant;
conv_q / conv_k / emb_rel_k of a one-token utterance; the float64 oracle gives < 1e-10 of the row's largest gradient) is bounded by the
zero-grad bar against the row's largest reference gradient.  Plugin: the
comparisons and bars of tests/test_resnet_varlen_gpu.py for padded-against-alone (same encoder; the back-end adds fp32 round-off only).
The tiny preset has 16-wide heads, which only the fp32 scoring path masks; bf16 scoring, training and the packed layouts use the 64-wide-head
SMALL config of tests/test_resnet_varlen_train_gpu.py, as those tests do."""
import os
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import btse as OB  # noqa: E402
from oracle import wav2vec2 as W  # noqa: E402
from oracle.aasist import fill_state  # noqa: E402
from scl_amd import btse_head as BH  # noqa: E402
from scl_amd import encoder as ENC  # noqa: E402
from scl_amd import model_front as MF  # noqa: E402
from scl_amd import model_linear as ML  # noqa: E402
from scl_amd import ops  # noqa: E402
from scl_amd.btse_head import BtseHead  # noqa: E402
from scl_amd.encoder import W2VConfig  # noqa: E402
from scl_amd.lib import SclError  # noqa: E402
from scl_amd.model_btse import Model  # noqa: E402
import test_btse_train_gpu as TT  # noqa: E402
from test_backends_train_gpu import Report, maxrel, rl2, upstream  # noqa: E402
from test_resnet_varlen_train_gpu import SMALL  # noqa: E402

pytestmark = pytest.mark.gpu

BARS = TT.BARS
ROW_BARS = dict(BARS, **{"grad": 2.9e-3,          # 3 x 9.73e-4: the fixed-length entries on one full-length utterance (see the docstring)
                         "zero-grad": 2.0e-6})    # 3 x 6.81e-7
HEAD_BARS = dict(BARS, grad=6.3e-4)               # 3 x 2.11e-4: the fixed-length entries' rows summed over the six utterances of STEPS
ZERO_REF = 1e-10      # a float64 reference gradient below this share of the row's largest one is an analytic zero
NAN = float("nan")


def _head(dev, is_add, seed):
    args = OB.default_args(is_add=is_add, bio_out=128 if is_add else 64)
    filled = {k: torch.from_numpy(v) for k, v in fill_state(OB.state_shapes(args, 128), seed=seed).items()}
    head = BtseHead(args).to(dev)
    missing, unexpected = head.load_state_dict({k: v for k, v in filled.items() if not k.startswith("backend.LL.")}, strict=True)
    assert not missing and not unexpected
    return args, filled, head


# ---- 1. the bio kernels ----------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [("concat-70", (1, 2, 4, 5, 9, 63, 64, 65, 70, 70), 70, False),
                ("add-70", (1, 2, 4, 5, 9, 63, 64, 65, 70, 70), 70, True),
                ("concat-130", (64, 128, 129, 130), 130, False),
                ("add-130", (64, 128, 129, 130), 130, True)]


class Bio:
    """The bio transformer alone: a plan's buffers and descriptor, driven through ops.btse_bio_* as _BtseFn does."""

    def __init__(self, dev, is_add, Lt, B, seed):
        self.args, filled, self.head = _head(dev, is_add, seed)
        self.sd = {k: v.double().requires_grad_(True) for k, v in filled.items()}
        self.pl = BH._plan(self.head, B, 1, Lt, dev, own=True)
        self.names = [next(n for n, q in self.head.named_parameters() if q is p) for p in BtseHead.bio_params(self.head)]
        self.B, self.Lt, self.dev = B, Lt, dev
        self.pl["ws"].zero_()

    def run(self, bio, lens, d_out, own=True):
        """-> (scores [B, bio_out], slab [B, NP]) of one forward + backward."""
        pl = self.pl
        pl["bio"].copy_(bio.to(torch.int32)); pl["lens"].copy_(torch.as_tensor(lens, dtype=torch.int32))
        (ops.btse_bio_fwd_own if own else ops.btse_bio_fwd)(pl["desc"])
        out = (pl["s"] if self.args["is_add"] else pl["bvec"][:, BH.HID:]).clone()
        pl["ds"].copy_(d_out)
        (ops.btse_bio_bwd_own if own else ops.btse_bio_bwd)(pl["desc"])
        ops.reduce_slabs(pl["slab"], pl["gbio"], pl["NP"], self.B, pl["NP"])
        torch.cuda.synchronize()
        return out.cpu(), pl["slab"].clone().cpu(), pl["gbio"].clone().cpu()

    def oracle(self, bio, lens, d_out):
        """float64, every utterance alone at its own token count -> (scores, {name: [B, ...] gradient rows})."""
        scores, rows = [], {n: [] for n in self.names}
        leaves = [self.sd[n] for n in self.names]
        for b, k in enumerate(lens):
            s = OB.bio_encoder(self.sd, self.args, bio[b:b + 1, :k], torch.tensor([k], dtype=torch.int32))
            g = torch.autograd.grad(s, leaves, d_out[b:b + 1].double(), allow_unused=True)
            scores.append(s.detach())
            for n, leaf, gi in zip(self.names, leaves, g):
                rows[n].append(torch.zeros_like(leaf) if gi is None else gi)
        return torch.cat(scores), {n: torch.stack(v) for n, v in rows.items()}

    def split(self, slab_row):
        return dict(zip(self.names, torch.split(slab_row, self.pl["sizes"])))


def _kernel_inputs(B, Lt, bo, seed):
    rs = np.random.RandomState(seed)
    bio = torch.from_numpy(rs.randint(0, 3, size=(B, Lt)).astype(np.int32))
    d_out = torch.randn(B, bo, generator=torch.Generator().manual_seed(seed))
    return bio, d_out


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_own_entries_against_the_float64_oracle_alone(dev, case):
    tag, counts, Lt, is_add = case
    B = len(counts)
    k = Bio(dev, is_add, Lt, B, 4000 + Lt)
    bio, d_out = _kernel_inputs(B, Lt, k.args["bio_out"], Lt + B)
    out, slab, _ = k.run(bio, counts, d_out.to(dev))
    ref, rows = k.oracle(bio, counts, d_out)
    rep = Report(tag, ROW_BARS)
    rep.check("out", "scores", rl2(out, ref))
    rep.check("out-max", "scores", maxrel(out, ref))
    for b, n in enumerate(counts):
        rep.check("out", "scores[%d] (%d tokens)" % (b, n), rl2(out[b], ref[b]))
        got = k.split(slab[b])
        rowmax = max(rows[name][b].abs().max().item() for name in k.names)
        rep.check("grad", "slab row %d (%d tokens)" % (b, n), rl2(slab[b], torch.cat([rows[name][b].flatten() for name in k.names])))
        for name in k.names:
            r, g = rows[name][b].flatten(), got[name]
            if r.abs().max().item() < ZERO_REF * rowmax:
                rep.check("zero-grad", "%s row %d (%d tokens)" % (name, b, n), g.abs().max().item() / rowmax)
            else:
                rep.check("grad", "%s row %d (%d tokens)" % (name, b, n), rl2(g, r))
    rep.done()


@pytest.mark.parametrize("is_add", [False, True], ids=["concat", "add"])
def test_full_length_rows_are_bit_identical_to_the_fixed_length_entries(dev, is_add):
    B, Lt = 5, 70
    k = Bio(dev, is_add, Lt, B, 4100)
    bio, d_out = _kernel_inputs(B, Lt, k.args["bio_out"], 11)
    fixed = k.run(bio, [Lt] * B, d_out.to(dev), own=False)
    k.pl["slab"].fill_(NAN)
    own = k.run(bio, [Lt] * B, d_out.to(dev), own=True)
    assert fixed[0].abs().max() > 0 and fixed[1].abs().max() > 0
    assert all(torch.equal(a, b) for a, b in zip(fixed, own))
    # and with shorter rows the fixed-length entries keep the reference's read-out: zeros, where the own entries score
    lens = [Lt, 9, Lt, 64, 1]
    fixed, own = k.run(bio, lens, d_out.to(dev), own=False), k.run(bio, lens, d_out.to(dev), own=True)
    for b, n in enumerate(lens):
        assert torch.equal(fixed[0][b], own[0][b]) == (n == Lt) and torch.equal(fixed[1][b], own[1][b]) == (n == Lt)
        assert (n == Lt) or (not fixed[0][b].any() and not fixed[1][b].any() and own[0][b].any() and own[1][b].any())


def test_a_count_of_zero_gives_an_exactly_zero_score_and_slab_row(dev):
    B, Lt = 4, 70
    k = Bio(dev, False, Lt, B, 4200)
    bio, d_out = _kernel_inputs(B, Lt, 64, 12)
    k.pl["slab"].fill_(NAN); k.pl["bvec"].fill_(NAN)
    out, slab, gbio = k.run(bio, [0, 70, -3, 5], d_out.to(dev))
    for b in (0, 2):      # the kernel clamps a count to 0..Lt
        assert (out[b] == 0).all() and (slab[b] == 0).all()
    assert out[1].any() and out[3].any() and torch.isfinite(slab).all() and torch.isfinite(gbio).all()
    ref, _ = k.oracle(bio[[1, 3]], [70, 5], d_out[[1, 3]])
    assert rl2(out[[1, 3]], ref) < BARS["out"]


def test_nothing_beyond_the_tokens_reaches_a_bit(dev):
    counts, Lt = (1, 2, 4, 5, 9, 63, 64, 65, 70, 70), 70
    B = len(counts)
    k = Bio(dev, False, Lt, B, 4300)
    bio, d_out = _kernel_inputs(B, Lt, 64, 13)
    d_out = d_out.to(dev)
    clean = k.run(bio, counts, d_out)
    assert all(torch.isfinite(t).all() for t in clean) and clean[1].abs().max() > 0
    # other token ids beyond the counts (out-of-range ones too: the kernel clamps an id before it indexes the embedding)
    junk = bio.clone()
    rs = np.random.RandomState(5)
    for b, n in enumerate(counts):
        junk[b, n:] = torch.from_numpy(rs.choice([0, 1, 2, 7, -1], size=Lt - n).astype(np.int32))
    assert not torch.equal(junk, bio)
    assert all(torch.equal(a, b) for a, b in zip(clean, k.run(junk, counts, d_out)))
    # the scratch last used by a launch of another token count (same buffer, other layout), slab and gbio full of NaN
    other = BH._plan(k.head, B, 1, 33, dev, own=True)
    d = other["desc"]
    d.ws = k.pl["ws"].data_ptr()      # the larger buffer; ws_stride stays the 33-token stride
    other["bio"].copy_(bio[:, :33]); other["lens"].copy_(torch.tensor([min(n, 33) for n in counts], dtype=torch.int32))
    ops.btse_bio_fwd_own(d)
    other["ds"].copy_(d_out)
    ops.btse_bio_bwd_own(d)
    torch.cuda.synchronize()
    k.pl["slab"].fill_(NAN); k.pl["gbio"].fill_(NAN)
    assert all(torch.equal(a, b) for a, b in zip(clean, k.run(junk, counts, d_out)))
    # the scratch full of NaN: every entry is written before it is read
    k.pl["ws"].fill_(NAN); k.pl["slab"].fill_(NAN); k.pl["gbio"].fill_(NAN)
    assert all(torch.equal(a, b) for a, b in zip(clean, k.run(bio, counts, d_out)))


# ---- 2. the back-end -------------------------------------------------------------------------------------------------------------------
T_PAD, LT = 12, 70
STEPS = [((12, 1, 3, 7, 12, 5), (70, 1, 5, 64, 65, 9)),
         ((3, 12, 12, 1, 6, 11), (4, 70, 63, 70, 2, 66))]      # the second step, on the cached plan
HEAD_CASES = [("concat-eval", False, False), ("concat-train", False, True), ("add-eval", True, False), ("add-train", True, True)]


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_backend_with_frames_matches_the_oracle_on_every_utterance_alone(dev, case):
    tag, is_add, training = case
    B = 6
    args, filled, head = _head(dev, is_add, 5000 + is_add)
    head.train(training)
    BtseHead.reseed(head, 77 + is_add)
    sd = TT.oracle_sd(filled)
    hp = dict(head.named_parameters())
    y = torch.tensor([1, 1, 1, 0, 0, 0])
    rs = np.random.RandomState(9)
    rep = Report(tag, HEAD_BARS)
    plan = None
    for step, (frames, counts) in enumerate(STEPS):
        rep.step = step
        x = torch.randn(B, T_PAD, 128, generator=torch.Generator().manual_seed(31 * step + is_add))
        bio = torch.from_numpy(rs.randint(0, 3, size=(B, LT)).astype(np.int32))
        lens = torch.tensor(counts, dtype=torch.int32)
        masks = TT.dropout_masks(head.__dict__["_seed"], B, T_PAD) if training else None
        xg = x.to(dev).requires_grad_(True)
        tok, tl = (bio, lens) if step == 0 else (bio.to(dev), lens.to(dev))      # host tokens, then device-resident ones
        logp, b = BtseHead.forward(head, xg, tok, tl, frames=list(frames))
        plans = [pl for key, pl in head.__dict__["_btse_plans"].items() if key[:3] == (B, T_PAD, LT)]
        assert len(plans) == 1 and (plan is None or plans[0] is plan), "the second step did not reuse the cached plan"
        plan = plans[0]
        assert plan["frames"].tolist() == list(frames)
        omasks, flips = TT.product_branches(sd, x, masks, plan["pre"])
        # ---- float64: every utterance alone at its own frames and tokens, its masks sliced from the padded [B, T, 128] ones
        alone = lambda i: OB.forward(sd, args, x[i:i + 1, :frames[i]].double(), bio[i:i + 1, :counts[i]], lens[i:i + 1],   # noqa: E731
                                     [m[i:i + 1, :frames[i]] for m in omasks])
        with torch.no_grad():
            outs = [alone(i) for i in range(B)]
        ro, rb = torch.cat([o[0] for o in outs]), torch.cat([o[2] for o in outs])
        dl, db = upstream(ro, rb, x.double(), y, 1.0)
        assert dl.abs().max() > 0 and db.abs().max() > 0
        rdx = torch.zeros(B, T_PAD, 128, dtype=torch.float64)
        for i in range(B):
            xi = x[i:i + 1, :frames[i]].double().requires_grad_(True)
            lp, _, bb = OB.forward(sd, args, xi, bio[i:i + 1, :counts[i]], lens[i:i + 1], [m[i:i + 1, :frames[i]] for m in omasks])
            torch.autograd.backward([lp, bb], [dl[i:i + 1], db[i:i + 1]])
            rdx[i, :frames[i]] = xi.grad[0]
        # ---- product backward on poisoned scratch
        for name in TT.POISONED:
            plan[name].fill_(NAN)
        for t in plan["dpre"]:
            t.fill_(NAN)
        torch.autograd.backward([logp, b], [dl.float().to(dev), db.float().to(dev)])
        torch.cuda.synchronize()
        if step:
            BtseHead.check_tokens(head)
        print("\n[%s step %d] leaky_relu sign differences (GPU / float64) per layer: %s" % (tag, step, flips))
        blocks = [("logp", logp, ro), ("b", b, rb)]
        if not is_add:
            blocks += [("b[emb]", b[:, :128], rb[:, :128]), ("b[bio]", b[:, 128:], rb[:, 128:])]
        for name, g, r in blocks:
            rep.check("out", name, rl2(g, r))
            rep.check("out-max", name, maxrel(g, r))
        if not is_add:
            assert all(b[i, 128:].any() for i in range(B))      # every utterance scores, the short ones too
        for i, t in enumerate(frames):
            assert (xg.grad[i, t:] == 0).all(), (step, i, t)
        rep.check("grad_x", "feats", rl2(xg.grad, rdx))
        n = TT.compare_head_grads(rep, {k: p.grad for k, p in hp.items()}, sd)
        assert n == len(hp) - 2, n
        for p in list(hp.values()) + list(sd.values()):
            if p.grad is not None:
                p.grad.zero_()
    rep.done()


def test_backend_frames_refusals(dev):
    args, _, head = _head(dev, False, 5100)
    head.eval()
    feats = torch.zeros(2, 12, 128, device=dev)
    bio = torch.zeros(2, 5, dtype=torch.int32)
    ok = torch.tensor([5, 3], dtype=torch.int32)
    with torch.no_grad():
        for bad in ([12], [12, 0], [12, 13], [12, 3, 3]):
            with pytest.raises(ValueError, match="frames"):
                BtseHead.forward(head, feats, bio, ok, frames=bad)
        for bad in ([5, 0], [6, 3]):
            with pytest.raises(ValueError, match="own last token"):
                BtseHead.forward(head, feats, bio, torch.tensor(bad, dtype=torch.int32), frames=[12, 3])
        BtseHead.forward(head, feats, bio, torch.tensor([5, 0], dtype=torch.int32))      # the fixed-length contract is unchanged
        logp, b = BtseHead.forward(head, feats, bio, torch.tensor([5, 0], dtype=torch.int32, device=dev), frames=[12, 3])   # device counts: clamped
        torch.cuda.synchronize()
        assert b[0, 128:].any() and not b[1, 128:].any()


# ---- 3. the plugin ---------------------------------------------------------------------------------------------------------------------
ARGS = dict(OB.default_args(), name="wav2vec2_btse")
LENGTHS = [4000, 1000, 2500, 400]      # 12, 2, 7 frames and the single frame of the shortest row the encoder takes
CONF = {"model": {"contra_mode": "all", "loss_type": 1}}


def toy_tokens(x, fs):
    """A ragged toy tokeniser: one token per 300 samples (13, 3, 8 and 1 for LENGTHS), ids from the length."""
    assert fs == 16000
    n = x.shape[1]
    return [[(5 * i + n // 100) % 3 for i in range(max(1, n // 300))] for _ in range(x.shape[0])]


_CACHE = {}


def _plugin(dev, small, seed=71):
    """-> (model with the toy tokeniser, oracle encoder state, head state dict, oracle config); built once per config."""
    if small not in _CACHE:
        ocfg = W.W2VConfig(**SMALL) if small else W.W2VConfig.tiny()
        ssl = W.init_state(ocfg, seed=seed)
        m = Model(ARGS, dev, w2v_cfg=W2VConfig(**SMALL) if small else W2VConfig.tiny())
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("backend.ssl_model.")}
        head_sd = {k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=seed + 1).items()}
        sd = {"backend.ssl_model.model." + k: v for k, v in ssl.items()}
        sd.update(head_sd)
        m.load_state_dict(sd)
        m.bio_tokenizer = toy_tokens
        _CACHE[small] = (m, ssl, head_sd, ocfg)
    return _CACHE[small]


def _x(seed=2):
    x = torch.zeros(len(LENGTHS), max(LENGTHS))
    gen = torch.Generator().manual_seed(seed)
    for b, n in enumerate(LENGTHS):
        x[b, :n] = 0.1 * torch.randn(n, generator=gen)
    return x


def _tokens_alone(x, b):
    n = LENGTHS[b]
    t = toy_tokens(x[b:b + 1, :n].numpy(), 16000)[0]
    return torch.tensor([t], dtype=torch.int32), torch.tensor([len(t)], dtype=torch.int32)


def _cpu_alone(ssl, ocfg, head_sd, x, b):
    """(log-probs, feats, b) of the CPU chain (fp32 oracle encoder -> oracle back-end) on utterance b alone."""
    bio, lens = _tokens_alone(x, b)
    with torch.no_grad():
        return OB.forward(head_sd, OB.default_args(), W.forward(ssl, ocfg, x[b:b + 1, :LENGTHS[b]].contiguous()), bio, lens)


def _alone_on_gpu(m, x, dev):
    with torch.no_grad():
        return [tuple(t.clone() for t in m(x[b:b + 1, :n].to(dev))) for b, n in enumerate(LENGTHS)]


def test_the_toy_tokeniser_is_ragged():
    assert [len(toy_tokens(np.zeros((1, n)), 16000)[0]) for n in LENGTHS] == [13, 3, 8, 1]


@pytest.mark.parametrize("small", [False, True], ids=["tiny", "small"])
def test_fp32_scoring_of_a_padded_batch(dev, monkeypatch, small):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    m, ssl, head_sd, ocfg = _plugin(dev, small)
    m.eval()
    assert m.min_samples() == 400
    x = _x()
    with torch.no_grad():
        out, feats, b = (t.clone() for t in m(x.to(dev), lengths=LENGTHS))
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, dev)
    assert out.shape == (4, 2) and b.shape == (4, 192) and feats.shape == (4, 12, 128)
    for i, n in enumerate(LENGTHS):
        Tb = m.cfg.conv_lens(n)[-1]
        ro, rf, rb = _cpu_alone(ssl, ocfg, head_sd, x, i)
        assert rf.shape[1] == Tb and (feats[i, Tb:] == 0).all() and b[i, 128:].any()
        e = (rl2(feats[i, :Tb], rf[0]), rl2(b[i], rb[0]), rl2(out[i], ro[0]))
        go, gf, gb = alone[i]
        g = (maxrel(out[i], go[0]), maxrel(b[i], gb[0]), maxrel(feats[i, :Tb], gf[0]))
        print("fp32 n=%d (%d frames): rel-L2 against the CPU chain alone feats %.2e b %.2e log-probs %.2e | max-rel against the GPU alone "
              "log-probs %.2e b %.2e feats %.2e" % ((n, Tb) + e + g))
        assert e[0] < 1e-2 and e[1] < 3e-2 and e[2] < 3e-2, (n, e)
        assert max(g) < 1e-3, (n, g)
    if small:      # SCL_SCORE_PACK=1: the packed rows against the padded layout
        monkeypatch.setattr(ENC, "SCORE_PACK", True)
        with torch.no_grad():
            packed = tuple(t.clone() for t in m(x.to(dev), lengths=LENGTHS))
            torch.cuda.synchronize()
        p = tuple(maxrel(a, r) for a, r in zip(packed, (out, feats, b)))
        print("fp32 packed against padded: log-probs %.2e feats %.2e b %.2e" % p)
        assert max(p) < 1e-3, p


@pytest.mark.parametrize("pack", [False, True], ids=["padded", "packed"])
def test_bf16_scoring_of_a_padded_batch(dev, monkeypatch, pack):
    """SCL_SCORE_FP32=0 (and SCL_VARLEN_PACK): per tensor the bar is the larger of rel-L2 1e-2 feats / 3e-2 b and log-probs and twice the
    error the fixed-length bf16 path makes on the same utterance alone, both against the CPU chain on that utterance alone."""
    monkeypatch.setattr(MF, "SCORE_FP32", False); monkeypatch.setattr(ML, "SCORE_FP32", False)
    monkeypatch.setattr(ENC, "VARLEN_PACK", pack)
    m, ssl, head_sd, ocfg = _plugin(dev, True)
    m.eval()
    x = _x()
    with torch.no_grad():
        out, feats, b = (t.clone() for t in m(x.to(dev), lengths=LENGTHS))
        torch.cuda.synchronize()
    alone = _alone_on_gpu(m, x, dev)
    for i, n in enumerate(LENGTHS):
        Tb = m.cfg.conv_lens(n)[-1]
        ro, rf, rb = _cpu_alone(ssl, ocfg, head_sd, x, i)
        assert (feats[i, Tb:] == 0).all()
        go, gf, gb = alone[i]
        for name, got, fixed, ref, floor in (("feats", feats[i, :Tb], gf[0], rf[0], 1e-2), ("b", b[i], gb[0], rb[0], 3e-2),
                                             ("log-probs", out[i], go[0], ro[0], 3e-2)):
            err, base = rl2(got, ref), rl2(fixed, ref)
            print("bf16 %s n=%d (%d frames) %s: rel-L2 %.2e, the fixed-length path alone %.2e, bar %.2e"
                  % ("packed" if pack else "padded", n, Tb, name, err, base, max(floor, 2 * base)))
            assert err < max(floor, 2 * base), (name, n, err, base)
    assert ((4, 4000, "packed") if pack else (4, 4000)) in m._vstates      # a state per layout of the shape


def _step(m, x, dev, seed, coef):
    """One training step on LENGTHS with a loss that is a fixed linear form of the outputs (so that it splits over the utterances)
    -> (log-probs, feats, b, the whole flat gradient buffer)."""
    m._drop_step = seed
    BtseHead.reseed(m, seed)
    m.zero_torch_grads()
    out, feats, b = m(x.to(dev), lengths=LENGTHS)
    loss = (out * coef[0].to(dev)).sum() + (feats * coef[1].to(dev)).sum() + (b * coef[2].to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), feats.detach().clone(), b.detach().clone(), m.P.grad.clone()


def test_plugin_trains_on_ragged_lengths_like_the_cpu_chain_on_every_utterance_alone(dev, monkeypatch):
    monkeypatch.setattr(ENC, "VARLEN_PACK", False)
    m, ssl, head_sd, ocfg = _plugin(dev, True)
    m.train()
    try:
        cfg, T = m.cfg, m.cfg.conv_lens(max(LENGTHS))[-1]
        assert (cfg.dropout, cfg.attention_dropout, cfg.activation_dropout, cfg.dropout_input, cfg.encoder_layerdrop) == (0, 0, 0, 0, 0)
        gen = torch.Generator().manual_seed(8)
        coef = (torch.randn(4, 2, generator=gen), 0.05 * torch.randn(4, T, 128, generator=gen), torch.randn(4, 192, generator=gen))
        x = _x()
        junk = x.clone()
        for i, n in enumerate(LENGTHS):
            junk[i, n:] = 1e3 * torch.randn(max(LENGTHS) - n, generator=gen)
        first = _step(m, x, dev, 1234, coef)
        again = _step(m, junk, dev, 1234, coef)       # what x holds beyond the lengths reaches no bit of any output or gradient
        assert all(torch.isfinite(t).all() for t in first) and first[3].abs().max() > 0
        assert all(torch.equal(a, r) for a, r in zip(first, again))
        out, feats, b, grad = first
        # ---- the CPU chain per utterance alone, gradients summed.  As tests/test_resnet_varlen_train_gpu.py does: the oracle head (float32,
        # the MLP dropout masks sliced from the padded [B, T, 128] ones) runs on the plugin's OWN feats of that utterance — a leaky_relu
        # whose input moved by the bf16 encoder's 8e-3 changes its slope 100 x on a share of the 22 valid rows that no bar would cover —
        # and LL and the encoder take the gradient the head hands back
        masks = TT.dropout_masks(1234 & 0x7FFFFFFF, 4, T)
        for k, _, tr in W.param_shapes(ocfg):
            ssl[k].requires_grad_(bool(tr))
        hsd = {k: v.clone().requires_grad_(True) for k, v in head_sd.items()}
        ident = dict(hsd, **{"backend.LL.weight": torch.eye(128), "backend.LL.bias": torch.zeros(128)})
        for i, n in enumerate(LENGTHS):
            Tb = cfg.conv_lens(n)[-1]
            bio, lens = _tokens_alone(x, i)
            chain = F.linear(W.forward(ssl, ocfg, x[i:i + 1, :n].contiguous()), hsd["backend.LL.weight"], hsd["backend.LL.bias"])
            f = feats[i:i + 1, :Tb].detach().cpu().requires_grad_(True)
            ro, rf, rb = OB.forward(ident, OB.default_args(), f, bio, lens, [mk[i:i + 1, :Tb] for mk in masks])
            ((ro * coef[0][i:i + 1]).sum() + (rf * coef[1][i:i + 1, :Tb]).sum() + (rb * coef[2][i:i + 1]).sum()).backward()
            chain.backward(f.grad)
            assert (feats[i, Tb:] == 0).all() and b[i, 128:].any()
            e = (rl2(feats[i, :Tb], chain[0]), rl2(b[i], rb[0]), rl2(out[i], ro[0]))
            print("train n=%d (%d frames): rel-L2 feats against the CPU chain alone %.2e; b %.2e and log-probs %.2e against the oracle head on "
                  "the plugin's feats" % ((n, Tb) + e))
            assert e[0] < 1e-2 and e[1] < 3e-2 and e[2] < 3e-2, (n, e)      # the floors of the scoring comparisons above
        g = lambda name: grad[m.P.off(name):m.P.off(name) + m.P.g(name).numel()].view(m.P.g(name).shape)          # noqa: E731
        failed = []
        # bars of tests/test_btse_gpu.py::test_plugin_forward_and_train_step_against_the_cpu_chain: 5e-2 head and LL, 8e-2 encoder
        for k in ("fc2.weight", "bioScoring.bio_scoring.weight", "bioScoring.bio_embedding.weight", "bioScoring.encoder.attn_layers.0.conv_v.weight",
                  "bioScoring.encoder.attn_layers.1.emb_rel_v", "bioScoring.encoder.ffn_layers.2.conv_1.weight",
                  "backend.mlp.m_frame_level.linear_1.weight", "backend.mlp.m_frame_level.linear_2.bias", "backend.LL.weight"):
            name = k[len("backend."):] if k.startswith("backend.LL.") else k
            err = rl2(g(name), hsd[k].grad)
            print("train grad %s: rel-L2 %.3e (bar 5e-2)" % (k, err))
            if not err < 5e-2:
                failed.append((k, err))
        for n in ("post_extract_proj.weight", "encoder.layers.1.fc1.weight", "feature_extractor.conv_layers.0.0.weight"):
            err = rl2(g("ssl_model.model." + n), ssl[n].grad)
            print("train grad %s: rel-L2 %.3e (bar 8e-2)" % (n, err))
            if not err < 8e-2:
                failed.append((n, err))
        assert not failed, failed
        # SCL_VARLEN_PACK=1: the encoder on packed rows (the back-end stays padded) against the padded layout, outputs at the bars
        # tests/test_resnet_varlen_train_gpu.py holds for a packed step
        monkeypatch.setattr(ENC, "VARLEN_PACK", True)
        packed = _step(m, x, dev, 1234, coef)
        for name, a, r in zip(("log-probs", "feats", "b"), packed[:3], first[:3]):
            print("packed vs padded %s: rel-L2 %.2e max-rel %.2e" % (name, rl2(a, r), maxrel(a, r)))
            assert rl2(a, r) < 1e-2 and maxrel(a, r) < 3e-2, name
        assert torch.isfinite(packed[3]).all() and any(st["row0"] is not None for st in m._vstates_train.values())
    finally:
        for v in ssl.values():
            v.requires_grad_(False); v.grad = None
        m.eval()


def test_plugin_refusals(dev, monkeypatch):
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    monkeypatch.setattr(ENC, "SCORE_PACK", False)
    m, _, _, _ = _plugin(dev, False)
    x = _x().to(dev)
    m.eval()
    with pytest.raises(NotImplementedError, match="scoring mode"):
        m(x, lengths=LENGTHS)      # eval with autograd on
    m.train()
    try:
        with torch.no_grad(), pytest.raises(NotImplementedError, match="scoring mode"):
            m(x, lengths=LENGTHS)
    finally:
        m.eval()
    bio = torch.zeros(4, 6, dtype=torch.int32)
    with torch.no_grad():
        with pytest.raises(ValueError, match="own last token"):
            m(x, bio, torch.tensor([6, 0, 3, 1], dtype=torch.int32), lengths=LENGTHS)
        with pytest.raises(ValueError, match="lengths"):
            m(x, lengths=[4000, 1000, 2500, 399])      # below the 400 samples of one frame
        with pytest.raises(SclError, match="tokens <= 512"):
            m(x, torch.zeros(4, 513, dtype=torch.int32), torch.full((4,), 513, dtype=torch.int32), lengths=LENGTHS)
        out = m(x, bio, torch.tensor([6, 2, 3, 1], dtype=torch.int32), lengths=LENGTHS)      # explicit tokens of different counts
        assert torch.isfinite(out[0]).all()


# ---- 4. main.py --eval --padding_type none ---------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_main_eval_padding_type_none_with_the_btse_plugin(dev, tmp_path, monkeypatch):
    import yaml
    import main as M
    from scl_amd import pack
    monkeypatch.setattr(MF, "SCORE_FP32", True); monkeypatch.setattr(ML, "SCORE_FP32", True)
    (tmp_path / "toy_bio.py").write_text("def tok(x, fs):\n    n = x.shape[1]\n    return [[(5 * i + n // 100) % 3 for i in range(max(1, n // 300))] for _ in range(x.shape[0])]\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    root = tmp_path / "data"
    rs = np.random.RandomState(0)
    sizes = [1600, 4000, 8000, 12345, 16000, 24000]      # 0.1 to 1.5 s
    ids = ["u%d.wav" % i for i in range(len(sizes))]
    for u, n in zip(ids, sizes):
        _write_wav(str(root / u), 0.1 * rs.randn(n))
    (root / "protocol.txt").write_text("".join("%s eval bonafide\n" % u for u in ids))
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "conf-5-btse-trans64.yaml")) as f:
        model = yaml.safe_load(f)["model"]
    cfg = {"model": dict(model, w2v_arch="tiny", bio_tokenizer="toy_bio:tok"), "data": {"name": "eval_only", "kwargs": {}}}
    cfg_path = tmp_path / "conf.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ref_model = M.MODEL_REGISTRY["wav2vec2_btse"](cfg["model"], dev, seed=5)
    shapes = {k: tuple(v.shape) for k, v in ref_model.state_dict().items() if not k.startswith("backend.ssl_model.")}
    ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(shapes, seed=6).items()}, strict=False)
    ck = tmp_path / "ck.pth"
    torch.save({"module." + k: v for k, v in ref_model.state_dict().items()}, ck)
    ref_model.eval()
    want = []
    with torch.no_grad():
        for u, n in zip(ids, sizes):
            x = torch.from_numpy(np.asarray(pack.load_audio(str(root / u), 16000), dtype=np.float32))
            assert x.shape[0] == n
            want.append(ref_model(x[None].to(dev))[0][0].cpu().numpy())      # each file alone at its own length
    relerr = lambda got, ref: np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()      # noqa: E731
    scores = {}
    for bs in (4, 1):
        out = tmp_path / ("scores%d.txt" % bs)
        assert M.main(["--config", str(cfg_path), "--database_path", str(root), "--batch_size", str(bs), "--eval", "--model_path", str(ck),
                       "--padding_type", "none", "--eval_output", str(out)]) == 0
        lines = out.read_text().strip().split("\n")
        assert [l.split()[0] for l in lines] == ids
        scores[bs] = [[float(v) for v in l.split()[1:]] for l in lines]
    for a, o, ref in zip(scores[4], scores[1], want):
        assert relerr(a, np.asarray(o)) < 1e-3 and relerr(a, ref) < 1e-3 and relerr(o, ref) < 1e-3, (a, o, ref)
    assert len({tuple(s) for s in scores[4]}) == len(ids)
