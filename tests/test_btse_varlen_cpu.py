"""Variable-length batches on the `wav2vec2_btse` plugin, the parts that need no GPU.

The DEFINITION of what row b of a zero-padded batch of whole utterances gets: the bio score read at the utterance's OWN last token
k_b - 1 (oracle.btse.bio_encoder(..., return_x=True) gives the encoder output x * mask; the scoring conv is applied here) equals the
oracle on that utterance alone at its own token count — masked keys take the fill value -1e4 and their soft-max weight underflows to
exactly 0, so the valid positions do not see the padding.  Measured on the CPU, fill_state(..., seed=7), token counts 1, 2, 4, 5, 9, 63,
64, 65, 70 padded to 70: 3.9e-16 relative in fp64, 2.4e-7 in fp32.  The reference's own read-out (the last PADDED position times its mask,
model.py:234-236) is exactly 0 for every row shorter than the longest: right for its fixed-length batches, which keep it, and the reason
the `lengths` mode reads elsewhere.  The mean over time of the frame-level MLP over an utterance's own frames equals the mean alone.
Besides: the plugin's flags, main.py's start-up checks (--eval --padding_type none reaches the model build without any switch; the plugin
is not routed into --padding_type zero --batch_size k training), and the host-side padding of ragged tokeniser rows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import btse as OB
from oracle.aasist import fill_state

COUNTS = (1, 2, 4, 5, 9, 63, 64, 65, 70)
LT = 70


def own_score(sd, args, bio, lens):
    """The definition: the scoring conv on the encoder output at every utterance's own last token (zeros for an empty utterance)."""
    _, x = OB.bio_encoder(sd, args, bio, lens, return_x=True)
    Ws, bs = sd["bioScoring.bio_scoring.weight"][:, :, 0], sd["bioScoring.bio_scoring.bias"]
    rows = [F.linear(x[b, int(k) - 1], Ws, bs) if int(k) > 0 else torch.zeros_like(bs) for b, k in enumerate(lens.tolist())]
    return torch.stack(rows)


def alone_score(sd, args, bio, lens):
    return torch.cat([OB.bio_encoder(sd, args, bio[b:b + 1, :int(k)], lens[b:b + 1]) for b, k in enumerate(lens.tolist())])


def _case(dtype):
    args = OB.default_args()
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in fill_state(OB.state_shapes(args, 128), seed=7).items()}
    bio = torch.from_numpy(np.random.RandomState(7).randint(0, 3, size=(len(COUNTS), LT)).astype(np.int32))
    return args, sd, bio, torch.tensor(COUNTS, dtype=torch.int32)


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def test_own_last_token_score_equals_the_utterance_alone_in_float64():
    args, sd, bio, lens = _case(torch.float64)
    with torch.no_grad():
        own, alone = own_score(sd, args, bio, lens), alone_score(sd, args, bio, lens)
        junk = bio.clone()
        for b, k in enumerate(COUNTS):
            junk[b, k:] = (junk[b, k:] + 1) % 3      # other ids beyond the counts: nothing may move
        own_junk = own_score(sd, args, junk, lens)
    worst = max(_rel(own[b], alone[b]) for b in range(len(COUNTS)))
    print("own-last-token score against the utterance alone, fp64: %.2e relative" % worst)
    assert alone.abs().max() > 1e-3
    assert worst < 1e-12            # measured 3.9e-16
    assert torch.equal(own, own_junk)


def test_own_last_token_score_in_float32():
    args, sd, bio, lens = _case(torch.float32)
    with torch.no_grad():
        own, alone = own_score(sd, args, bio, lens), alone_score(sd, args, bio, lens)
    worst = max(_rel(own[b], alone[b]) for b in range(len(COUNTS)))
    print("own-last-token score against the utterance alone, fp32: %.2e relative" % worst)
    assert worst < 5e-6             # measured 2.4e-7: fp32 round-off of three layers, a handful of ulps


def test_the_reference_read_out_of_every_shorter_row_is_exactly_zero():
    args, sd, bio, lens = _case(torch.float64)
    x = sd["bioScoring.bio_embedding.weight"].clone().requires_grad_(True)
    sd = dict(sd, **{"bioScoring.bio_embedding.weight": x})
    s = OB.bio_encoder(sd, args, bio, lens)
    for b, k in enumerate(COUNTS):
        assert (k < LT) == bool((s[b] == 0).all()), (b, k)
    (g,) = torch.autograd.grad(s[:-1].sum(), x, allow_unused=True)      # and no gradient either
    assert g is None or not g.any()


def test_masked_mean_over_the_own_frames_equals_the_mean_alone():
    args = OB.default_args()
    sd = {k: torch.from_numpy(v).double() for k, v in fill_state(OB.state_shapes(args, 128), seed=7).items()}
    sd["backend.LL.weight"], sd["backend.LL.bias"] = torch.eye(128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64)
    frames = [12, 1, 3, 7, 12, 5]
    T = 12
    feats = torch.randn(len(frames), T, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    bio, lens = torch.zeros(len(frames), 3, dtype=torch.int32), torch.full((len(frames),), 3, dtype=torch.int32)
    with torch.no_grad():
        h = feats
        for i in range(3):
            h = F.leaky_relu(F.linear(h, sd["backend.mlp.m_frame_level.linear_%d.weight" % i], sd["backend.mlp.m_frame_level.linear_%d.bias" % i]), 0.01)
        keep = (torch.arange(T)[None, :] < torch.tensor(frames)[:, None]).double()[:, :, None]
        masked = (h * keep).sum(1) / torch.tensor(frames, dtype=torch.float64)[:, None]
        for b, t in enumerate(frames):
            alone = OB.forward(sd, args, feats[b:b + 1, :t], bio[b:b + 1], lens[b:b + 1])[2][0, :128]
            assert _rel(masked[b], alone) < 1e-13, (b, t)
        assert _rel(h.mean(1)[1], masked[1]) > 1e-2      # the plain mean over the padded frames is something else


def test_the_plugin_declares_both_modes():
    from scl_amd.model_btse import Model
    assert Model.head_takes_frames is True and Model.head_trains_frames is True
    m = Model.__new__(Model)
    assert m.head_min_frames() == 1 and m.head_max_frames() is None


def test_ragged_token_rows_are_padded_with_token_zero_and_keep_their_counts():
    from scl_amd.model_btse import pad_token_rows
    bio, lens = pad_token_rows([[1, 2, 2], [2], [1, 1, 2, 1, 2], []])
    assert bio.dtype == torch.int32 and lens.dtype == torch.int32
    assert bio.tolist() == [[1, 2, 2, 0, 0], [2, 0, 0, 0, 0], [1, 1, 2, 1, 2], [0, 0, 0, 0, 0]] and lens.tolist() == [3, 1, 5, 0]
    bio, lens = pad_token_rows([np.array([2, 1]), (0, 1)])
    assert bio.tolist() == [[2, 1], [0, 1]] and lens.tolist() == [2, 2]


def test_get_bio_own_calls_the_tokeniser_once_per_utterance_on_its_own_samples():
    from scl_amd.model_btse import Model
    seen = []

    def tok(x, fs):
        seen.append(x.shape)
        return [[1 + (i % 2) for i in range(x.shape[1] // 1000)] for _ in range(x.shape[0])]
    m = Model.__new__(Model)
    m.__dict__["bio_tokenizer"] = tok
    bio, lens = m.get_bio_own(torch.zeros(3, 4000), [4000, 1000, 2500], 16000)
    assert seen == [(1, 4000), (1, 1000), (1, 2500)]
    assert bio.tolist() == [[1, 2, 1, 2], [1, 0, 0, 0], [1, 2, 0, 0]] and lens.tolist() == [4, 1, 2]
    for bad in ([4000, 1000], [4000, 0, 10], [4000, 4001, 10]):
        with pytest.raises(ValueError, match="lengths"):
            m.get_bio_own(torch.zeros(3, 4000), bad, 16000)


def test_main_scores_this_plugin_with_lengths_and_does_not_route_it_into_padded_training(monkeypatch):
    import main as M
    monkeypatch.delenv("SCL_AASIST_LENGTHS", raising=False)
    assert M._scores_varlen("wav2vec2_btse") is True
    assert "wav2vec2_btse" in M.VARLEN_SCORING_MODELS
    assert "wav2vec2_btse" not in M.VARLEN_MODELS and "wav2vec2_btse" not in M.VARLEN_SCORING_OPT_IN
    assert not M._scores_varlen("wav2vec2_aasist")


def test_main_eval_padding_type_none_reaches_the_model_build(tmp_path, monkeypatch):
    import yaml
    import main as M

    class Reached(Exception):
        pass

    def build(*a, **k):
        raise Reached()
    (tmp_path / "toy_bio.py").write_text("def tok(x, fs):\n    return [[1] * max(1, x.shape[1] // 1000) for _ in range(x.shape[0])]\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    cfg = {"model": dict(OB.default_args(), name="wav2vec2_btse", w2v_arch="tiny", bio_tokenizer="toy_bio:tok"),
           "data": {"name": "eval_only", "kwargs": {}}}
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SCL_AASIST_LENGTHS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)      # the start-up checks come before anything touches a device
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    monkeypatch.setitem(M.MODEL_REGISTRY, "wav2vec2_btse", build)      # the model is the first thing behind the start-up checks
    argv = ["--config", str(tmp_path / "conf.yaml"), "--database_path", str(tmp_path), "--eval", "--padding_type", "none",
            "--eval_output", str(tmp_path / "x.txt")]
    with pytest.raises(Reached):
        M.main(argv)
    # without a tokeniser the plugin cannot run from main.py at all: that refusal is unchanged
    cfg["model"].pop("bio_tokenizer")
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit, match="bio_tokenizer"):
        M.main(argv)
