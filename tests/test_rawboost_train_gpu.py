"""RawBoost as training runs it: the fast sampler (main.py's default, what bench.py times) at the shapes the pack builder and the bench
feed the kernels, every row against the fp64 oracle (oracle/rawboost.py) given the very draws the sampler made.

The draws are recorded by wrapping augment._fast_lnl / _fast_isd / _fast_ssi: each wrapper returns what the original returned and keeps
it, and the oracle's given-draws forms (lnl_apply, isd_apply, ssi_apply) are applied to it in the algo's chain order
(datautils/asvspoof_2019_augall_3.py:377-439).  Shapes: 64 x 64000 (bench.py: 16 FIR tiles per clip, the last one 2560 samples, 64 clips
in one launch), 16 x 64000 for every algo, and one-clip calls as the pack builder makes them, from shorter than the filter to ~50 tiles.
Rows get different amplitudes, some peaking above 1 and some below, so both branches of the conditional peak normalisation run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import augment as AUG  # noqa: E402
from scl_amd.datautils_common import default_rawboost_args  # noqa: E402
from oracle import rawboost as RB  # noqa: E402

BAR = 3e-5                                  # tests/test_augment_gpu.py: fp32 direct-form FIR vs the reference's float64
CHAINS = {1: "L", 2: "I", 3: "S", 4: "LIS", 5: "LI", 6: "LS", 7: "IS"}      # oracle/rawboost.py:146-180
UNNORMALISED = {3, 4, 6, 7}                 # the chain ends in SSI: x + noise, no peak normalisation


@pytest.fixture
def draws(monkeypatch):
    rec = {"L": [], "I": [], "S": []}
    for key, name in (("L", "_fast_lnl"), ("I", "_fast_isd"), ("S", "_fast_ssi")):
        def wrap(*a, _orig=getattr(AUG, name), _key=key, **kw):
            out = _orig(*a, **kw)
            rec[_key].append(out)
            return out
        monkeypatch.setattr(AUG, name, wrap)
    return rec


def _oracle(x, algo, d, i, g_sd):
    """row i through the algo's chain with the recorded draws of that row"""
    stage = {"L": lambda v: RB.lnl_apply(v, d["L"][0][i]),
             "I": lambda v: RB.isd_apply(v, d["I"][0][i][0], d["I"][0][i][1], g_sd),
             "S": lambda v: RB.ssi_apply(v, *d["S"][0][i])}
    if algo == 8:
        return RB.norm_wav(stage["L"](x) + stage["I"](x), 0)
    for st in CHAINS[algo]:
        x = stage[st](x)
    return x


def _run(dev, draws, x, algo, seed):
    """rawboost_batch(sampler="fast") on x [n, L]; per row (worst |err|, |err| / row peak, the oracle row)."""
    args = default_rawboost_args()
    for v in draws.values():
        v.clear()
    AUG.seed_fast_sampler(seed)
    y = AUG.rawboost_batch(torch.from_numpy(x).to(dev), args, algo, 16000, sampler="fast")
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert y.shape == x.shape and y.dtype == np.float32 and np.isfinite(y).all()
    stages = "LI" if algo == 8 else CHAINS[algo]
    assert all(len(draws[st]) == (1 if st in stages else 0) for st in "LIS"), {k: len(v) for k, v in draws.items()}
    assert all(len(draws[st][0]) == x.shape[0] for st in stages)
    errs, rels, refs = [], [], []
    for i in range(x.shape[0]):
        ref = _oracle(x[i], algo, draws, i, args.g_sd)
        e = float(np.abs(y[i].astype(np.float64) - ref).max())
        errs.append(e)
        rels.append(e / float(np.abs(ref).max()))
        refs.append(ref)
    return np.array(errs), np.array(rels), refs


def _check(tag, algo, errs, rels):
    print("rawboost fast %s algo %d: worst |err| %.3e (row %d)%s" % (tag, algo, errs.max(), int(errs.argmax()),
          ", worst |err| / row peak %.3e" % rels.max() if algo in UNNORMALISED else ""))
    bad = np.nonzero(errs >= BAR)[0]
    assert bad.size == 0, "%s algo %d: rows %s miss the %.0e bar, worst %.3e" % (tag, algo, bad.tolist()[:16], BAR, errs.max())
    if algo in UNNORMALISED:
        bad = np.nonzero(rels >= BAR)[0]
        assert bad.size == 0, "%s algo %d: rows %s miss %.0e relative to the row peak, worst %.3e" % (tag, algo, bad.tolist()[:16], BAR,
                                                                                                       rels.max())


def _rows(n, L, seed):
    """n rows of Gaussian noise at amplitudes spread over 0.04 .. 0.8 in shuffled order: peaks from ~0.15 to ~3.5"""
    rs = np.random.RandomState(seed)
    amp = np.geomspace(0.04, 0.8, n)[rs.permutation(n)]
    x = (amp[:, None] * rs.randn(n, L)).astype(np.float32)
    peak = np.abs(x).max(axis=1)
    assert (peak > 1).any() and (peak < 1).any()
    return x


@pytest.mark.parametrize("algo", [5, 4])
def test_64_clips_of_64000_every_row(dev, draws, algo):
    """bench.py's configuration (algo 5, 64 x 64000) and the full LnL -> ISD -> SSI chain at the same size: clip strides past clip 16
    and the 16th, partial FIR tile (2560 of 4096 samples) of every clip."""
    x = _rows(64, 64000, 11)
    errs, rels, refs = _run(dev, draws, x, algo, 1000 + algo)
    _check("64x64000", algo, errs, rels)
    if algo == 5:
        lnl_peak = np.array([np.abs(RB.lnl_apply(x[i], draws["L"][0][i])).max() for i in range(64)])
        assert (lnl_peak > 1 - 1e-9).any() and (lnl_peak < 0.999).any()      # LnL normalised some rows and left others alone


@pytest.mark.parametrize("algo", range(1, 9))
def test_16_clips_of_64000_every_algo(dev, draws, algo):
    x = _rows(16, 64000, 20 + algo)
    errs, rels, _ = _run(dev, draws, x, algo, 2000 + algo)
    _check("16x64000", algo, errs, rels)


@pytest.mark.parametrize("L", [200, 4095, 4096, 4097, 12289, 211000])
@pytest.mark.parametrize("algo", [5, 3, 8])
def test_one_clip_as_the_pack_builder_calls(dev, draws, L, algo):
    """One utterance per call (scl_amd/pack.py RawBoost12): 200 samples is shorter than most filters (their half-length reaches past
    both ends), 4095 / 4096 / 4097 straddle one FIR tile, 12289 is three tiles and one sample, 211000 is a ~13 s utterance: 52 tiles
    and up to 21100 ISD positions."""
    rs = np.random.RandomState(L + algo)
    for amp in (0.1, 0.6):
        x = (amp * rs.randn(1, L)).astype(np.float32)
        errs, rels, _ = _run(dev, draws, x, algo, 3000 + 7 * algo + L)
        _check("1x%d amp %.1f" % (L, amp), algo, errs, rels)
        if algo != 3:
            assert len(draws["L"][0][0]) == 5
        if algo == 5 and L >= 12289:
            assert len(draws["I"][0][0][0]) > 0
