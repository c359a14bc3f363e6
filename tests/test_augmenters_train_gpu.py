"""The four conf-5 augmenters besides RawBoost — RIR reverb, MUSAN overlay, pydub speed, librosa pitch — at the lengths training feeds
them, against the oracle restatements (oracle/audio_int16.py, oracle/audio_speed_pitch.py; both pinned to the reference's goldens and
to CPython audioop by tests/test_oracle_golden.py), and a conf-5 pack at trim length 64000 checked view by view.

The augmenters run on the whole decoded utterance before the multi-view crop (scl_amd/pack.py), so they see speech of 1 - 13 s
(16 000 - 211 000 samples), MUSAN files longer than the speech and RIRs of 1e3 - 5e4 taps.  Every bar below carries its measured
worst value (MI355X) in its comment and every check prints the worst value it saw, so the log records the margin."""
import math
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from scl_amd import augment as AUG  # noqa: E402
from scl_amd import ops  # noqa: E402
from oracle import audio_int16 as AI  # noqa: E402
from oracle import audio_speed_pitch as SP  # noqa: E402
from oracle import multiview as OM  # noqa: E402
from oracle import rawboost as RB  # noqa: E402
from tests import reverb_ties as RT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- bars (measured worst on MI355X in the comments) ------------------------------------------------------------------------------
# RIR convolution: tests/reverb_ties.py (CONV_REL_SUM, CONV_REL_MAX)
FIR_LONG_REL_SUM = 1e-5   # fir_kernel at 4096 - 48000 taps (SCL_RIR_GEMM=0), / sum|x||h|.  measured 7.2e-7 (211000 x 48000)
FIR_LONG_REL_MAX = 1e-4   # the same, / max|y|.  measured 1.6e-5 (211000 x 48000)
FIR_LONG_TIES = 0.1       # fraction of samples where the GEMM and fir_kernel outputs truncate apart.  measured 5.5e-2 (211000 x 48000)
STFT_REL = 1e-6           # STFT vs numpy's float64 FFT, / max |D| (tests/test_augment_gpu.py: 2e-5).  measured 2.2e-7
PV_MAG_REL = 1e-6         # phase-vocoder magnitudes, / max |out|.  measured 3.2e-7
PV_PHASE0_ULP = 4         # arg out[k, 0] vs angle(D[k, 0]), in float32 steps at pi.  measured 1.5
PV_INC_C = 16             # phase increments within ulp(|acc|) + c ulp(pi) (oracle.audio_speed_pitch.phase_increment_errors); the bar is
                          # 1.0 of that bound.  measured 0.500 (the accumulator's own float32 rounding), 3.1e-2 rad in the top bins
ISTFT_ABS = 2e-6          # tests/test_augment_gpu.py.  measured 1.8e-7
RESAMPLE_ABS = 1e-6       # tests/test_augment_gpu.py.  measured 0
RESAMPLE_ULP = 1          # both sides sum in float64 and round once to float32: float32 steps of |out|.  measured 0 (bit-identical)
PITCH_REL_L2 = 2e-3       # end to end at 64000 / 211000 samples, int16 output.  measured 1.07e-3 (211000 white noise, n_steps +1)
PITCH_FRAME_REL = 3e-3    # per-frame magnitude spectrum of the int16 output, ||(|G| - |R|)|| / ||R||.  measured 1.68e-3 (the same case)


def _speech(L, seed, amp=0.3):
    """speech-like: two partials under a syllable-rate envelope, plus noise"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / 16000.0
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + rs.uniform(0, 6)) ** 2
    x = env * (np.sin(2 * np.pi * 180 * t) + 0.5 * np.sin(2 * np.pi * 1130 * t + 1.0)) + 0.1 * rs.randn(L)
    return (amp / np.abs(x).max() * x).astype(np.float32)


def _rir(R, seed):
    """exponentially decaying noise (as the goldens' RIRs), the decay constant a fifth of the length"""
    rs = np.random.RandomState(seed)
    return (np.exp(-np.arange(R) / (R / 5.0)) * rs.randn(R) * 0.3).astype(np.float32)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- 1. reverb ---------------------------------------------------------------------------------------------------------------------
FIR_R = [256, 257, 1023]                              # fir_kernel: whole / partial 256-tap chunks
GEMM_R = [1024, 1025, 4096, 16000, 48000]             # Toeplitz GEMM, split-K 8 .. 32
REVERB_SHAPES = [(L, R) for L in (16000, 64000, 211000) for R in FIR_R + GEMM_R] + [(8000, 16000), (16000, 48000)]


def _fir_conv(x, rir):
    """the fir_kernel branch of augment.reverb, pre-quantisation"""
    L, R = x.numel(), rir.numel()
    Lout = L + R - 1
    z0, zr = AUG._h2d_pack([np.zeros(1, dtype=np.int32), np.array([R], dtype=np.int32)], x.device)
    y = torch.empty(Lout, device=x.device)
    part = torch.empty(ops.fir_nblocks(Lout) * 4, device=x.device)
    ops.fir_multi(x, L, L, rir, z0, zr, z0, 1, 1, False, y, Lout, Lout, part)
    return y


def _gpu_conv(x, rir):
    if rir.numel() >= AUG._RIR_GEMM_MIN_TAPS:
        y, _, Lout = AUG._rir_full_conv_gemm(x, rir)
        return y[:Lout]
    return _fir_conv(x, rir)


def _splitk(L, R):
    Kp = (R + 63 + 15) // 16 * 16
    M = (L + R - 1 + 63) // 64
    return max(1, min(32, (Kp // 16) // 8, (4 * 256) // max(1, (M + 63) // 64))), Kp // 16


@pytest.mark.parametrize("L,R", REVERB_SHAPES)
def test_reverb_convolution_against_float64(dev, L, R):
    """Pre-quantisation: the float32 convolution (fir_kernel below 1024 taps, the split-K Toeplitz GEMM above) against the float64
    one, relative to sum_t |x[m - t]| |h[t]| per sample.  The reference's own float32 np.convolve is held to the same bar.  In none
    of the GEMM shapes does the K range (Kp / 16 steps) divide evenly by the split."""
    x, h = _speech(L, L + R), _rir(R, R)
    y = _np(_gpu_conv(torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev))).astype(np.float64)
    y64, S = RT.conv_refs(x, h)
    assert y.shape == y64.shape
    e, emax = RT.conv_errors(y, y64, S)
    e_np, emax_np = RT.conv_errors(np.convolve(x, h), y64, S)
    sk, nk = _splitk(L, R)
    if R >= AUG._RIR_GEMM_MIN_TAPS:
        assert sk > 1 and nk % sk != 0, (sk, nk)
    print("reverb conv %d x %d (%s): |err| / sum|x||h| GPU %.2e numpy %.2e, |err| / max|y| GPU %.2e numpy %.2e" % (
        L, R, "gemm split %d of %d" % (sk, nk) if R >= AUG._RIR_GEMM_MIN_TAPS else "fir", e, e_np, emax, emax_np))
    assert e <= RT.CONV_REL_SUM and e_np <= RT.CONV_REL_SUM, (e, e_np)
    assert emax <= RT.CONV_REL_MAX and emax_np <= RT.CONV_REL_MAX, (emax, emax_np)


@pytest.mark.parametrize("L,R", REVERB_SHAPES)
def test_reverb_int16_against_the_oracle_up_to_ties(dev, L, R):
    """augment.reverb against oracle.audio_int16.reverb (float32 np.convolve, / max, C cast): equal everywhere except at ties, a tie
    being a sample whose exact value lies within the measured error band (tests/reverb_ties.py) of an integer."""
    x, h = _speech(L, L + R), _rir(R, R)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
    got = _np(AUG.reverb(xd, hd))
    ref = AI.reverb(x, h)
    y64, S = RT.conv_refs(x, h)
    n, med, frac, _ = RT.check_up_to_ties("%dx%d" % (L, R), got, ref, y64, S, [_np(_gpu_conv(xd, hd)), np.convolve(x, h)])
    print("reverb int16 %d x %d: %d of %d samples differ (ties); band median %.1e LSB, %.2e of samples inside it" % (L, R, n, got.size, med, frac))


@pytest.mark.parametrize("path", ["fir", "gemm"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("where", ["first", "last"])
def test_reverb_peak_in_the_first_and_last_tile(dev, path, sign, where):
    """The convolution's peak in the first / last FIR tile (4096 outputs) and 64-row GEMM block, positive (+1.0 * 32768 wraps to
    -32768) and negative: a clip_affine that misses a block's peak or the last partial block gets the scale wrong everywhere."""
    L, R = 64000, (700 if path == "fir" else 5000)
    rs = np.random.RandomState(7)
    x = (0.01 * rs.randn(L)).astype(np.float32)
    h = (0.05 * _rir(R, 3)).astype(np.float32)
    if where == "first":
        x[2] = sign
        h[0] = 1.0
        m = 2
    else:
        x[L - 3] = sign
        h[R - 1] = 1.0
        m = L - 3 + R - 1
    y64, S = RT.conv_refs(x, h)
    assert int(np.abs(y64).argmax()) == m and np.sign(y64[m]) == sign
    Lout = L + R - 1
    assert (m < 4096 and m < 64) if where == "first" else (m >= (Lout - 1) // 4096 * 4096 and m >= (Lout - 1) // 64 * 64)
    if path == "gemm":
        assert R >= AUG._RIR_GEMM_MIN_TAPS and AUG.RIR_GEMM
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
    got = _np(AUG.reverb(xd, hd)).astype(np.int64)
    ref = AI.reverb(x, h).astype(np.int64)
    assert ref[m] == -32768
    assert got[m] in ((-32768, 32767) if sign > 0 else (-32768, -32767)), got[m]
    n, _, _, _ = RT.check_up_to_ties("peak %s %s %+d" % (path, where, sign), got, ref, y64, S, [_np(_gpu_conv(xd, hd)), np.convolve(x, h)])
    print("reverb peak %s %s %+.0f: got[peak] %d, %d ties" % (path, where, sign, got[m], n))


def test_toeplitz_image_cache(dev, monkeypatch):
    """augment._TOEPLITZ (one thread): an RIR reused for clips of three lengths; an RIR freed and replaced by a new tensor of the same
    length in the same storage (the weak reference must reject the stale image); more than 256 RIRs (the cache is cleared).  Every
    output equals the computation with an empty cache."""
    monkeypatch.setattr(AUG, "_TOEPLITZ", {})

    def uncached(x, h):
        saved = dict(AUG._TOEPLITZ)
        AUG._TOEPLITZ.clear()
        out = _np(AUG.reverb(x, h))
        AUG._TOEPLITZ.clear()
        AUG._TOEPLITZ.update(saved)
        return out

    h = torch.from_numpy(_rir(4096, 1)).to(dev)
    for L in (16000, 211000, 5000):
        x = torch.from_numpy(_speech(L, L)).to(dev)
        assert np.array_equal(_np(AUG.reverb(x, h)), uncached(x, h)), L
    assert len(AUG._TOEPLITZ) == 1
    x = torch.from_numpy(_speech(16000, 3)).to(dev)
    h1 = torch.from_numpy(_rir(16000, 2)).to(dev)
    first = _np(AUG.reverb(x, h1))
    h2 = h1[:]                                          # a new tensor object on the same storage, as a reallocation would give
    p1 = h1.data_ptr()
    del h1                                              # the cached entry's weak reference is dead now, its key still matches
    h2.copy_(torch.from_numpy(_rir(16000, 9)))
    assert h2.data_ptr() == p1 and (p1, 16000, str(h2.device)) in AUG._TOEPLITZ
    second = _np(AUG.reverb(x, h2))
    assert np.array_equal(second, uncached(x, h2)) and not np.array_equal(second, first)
    keep = [torch.from_numpy(_rir(1024, 100 + i)).to(dev) for i in range(260)]
    xs = torch.from_numpy(_speech(3000, 4)).to(dev)
    sizes = []
    for i, hh in enumerate(keep):
        out = _np(AUG.reverb(xs, hh))
        sizes.append(len(AUG._TOEPLITZ))
        if i in (0, 255, 256, 257, 259):
            assert np.array_equal(out, uncached(xs, hh)), i
    assert max(sizes) == 257 and sizes[-1] < 257, sizes[250:]
    assert np.array_equal(_np(AUG.reverb(xs, keep[0])), uncached(xs, keep[0]))      # an RIR whose image the clear dropped
    print("toeplitz cache: cache sizes around the clear %s" % sizes[252:260])


@pytest.mark.parametrize("L,R", [(64000, 4096), (16000, 16000), (211000, 48000), (8000, 16000)])
def test_reverb_gemm_switch_off_gives_the_same_int16(dev, monkeypatch, L, R):
    """augment.RIR_GEMM = False (SCL_RIR_GEMM=0) puts every RIR on fir_kernel: same int16 output up to ties.  fir_kernel sums the
    taps of an output in one float32 chain, so its error at these tap counts exceeds the GEMM's (split-K: shorter chains): its own
    bars (FIR_LONG_*)."""
    x, h = _speech(L, L + R), _rir(R, R)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
    a = _np(AUG.reverb(xd, hd))
    monkeypatch.setattr(AUG, "RIR_GEMM", False)
    b = _np(AUG.reverb(xd, hd))
    y64, S = RT.conv_refs(x, h)
    n, med, _, errs = RT.check_up_to_ties("switch %dx%d" % (L, R), a, b, y64, S, [_np(_gpu_conv(xd, hd)), _np(_fir_conv(xd, hd))],
                                          bars=(FIR_LONG_REL_SUM, FIR_LONG_REL_MAX), max_frac=FIR_LONG_TIES)
    print("reverb gemm vs fir %d x %d: %d ties (%.2e of the samples), band median %.1e LSB; fir_kernel |err| / sum|x||h| %.2e, / max|y| "
          "%.2e" % (L, R, n, n / a.size, med, errs[1][0], errs[1][1]))


# ---- 2. background noise -----------------------------------------------------------------------------------------------------------
def _noise(n, seed, amp=800.0):
    rs = np.random.RandomState(seed)
    return np.clip(np.round(amp * rs.randn(n)), -32768, 32767).astype(np.int16)


def _overlay_both_paths(dev, x, noise, snr, tag):
    ref, gain = AI.background_noise(x, noise, snr)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    got = _np(AUG.background_noise(xd, nd, snr))
    nsq = int((noise.astype(np.int64) ** 2).sum())
    got_h = _np(AUG.background_noise(xd, nd, snr, sumsq=(AUG.host_i16_sumsq(x), nsq)))
    assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float32)), (tag, np.abs(got - ref).max())
    assert np.array_equal(got_h, got), tag
    return ref, gain


@pytest.mark.parametrize("L", [16000, 64000, 211000])
def test_background_noise_bit_exact_at_corpus_lengths(dev, L):
    """MUSAN files longer than the speech (480 000 and ~4.8 M samples: the usual case), as long, and shorter; SNR 5 / 10 / 15; the
    device power path (i16_sumsq) and the host one the pack builder takes (host_i16_sumsq) — both bit-exact against the oracle."""
    x = _speech(L, L, amp=0.5)
    for nn in (480000, 4800017, L, L // 3 + 1):
        noise = _noise(nn, nn)
        for snr in (5, 10, 15):
            _, gain = _overlay_both_paths(dev, x, noise, snr, (L, nn, snr))
    print("background noise L %d: bit-exact for 4 noise lengths x 3 SNRs, last gain %.2f dB" % (L, gain))


def test_background_noise_saturation_and_silence(dev):
    """audioop.mul saturating (loud speech, quiet noise: a gain of ~+100 dB), the overlay add saturating (full-scale noise), and speech
    below one LSB (rms 0, dBFS = -inf, gain 0).  Not covered: a noise file of digital silence — its dBFS is -inf, the gain +inf, and
    what audioop.mul does with an infinite factor is undefined C in the reference."""
    L = 64000
    loud = _speech(L, 1, amp=0.95)
    for snr in (5, 10, 15):
        ref, gain = _overlay_both_paths(dev, loud, _noise(480000, 2, amp=3.0), snr, ("mul saturates", snr))
        assert gain > 40 and (np.abs(ref) >= 32767).mean() > 0.3, gain
        ref, gain = _overlay_both_paths(dev, _speech(L, 3, amp=0.3), (np.random.RandomState(4).randint(-32768, 32768, 480000)).astype(np.int16),
                                        snr, ("add saturates", snr))
        assert (np.abs(ref) >= 32767).mean() > 0.01
    quiet = (4e-6 * np.random.RandomState(5).randn(L)).astype(np.float32)
    assert not AI.librosa_to_int16(quiet).any()
    for snr in (5, 15):
        ref, gain = _overlay_both_paths(dev, quiet, _noise(480000, 6), snr, ("silent speech", snr))
        assert gain == 0 and np.array_equal(ref, _noise(480000, 6)[:L])
    print("background noise: saturating mul / add and silent speech bit-exact")


# ---- 3. speed ----------------------------------------------------------------------------------------------------------------------
FACTORS = (0.9, 0.931, 0.97, 0.999, 1.0, 1.004, 1.0067, 1.01, 1.02, 1.05, 1.0999, 1.1)


@pytest.mark.parametrize("L", [16000, 64000, 64001, 150017, 211000])
def test_speed_bit_exact_at_corpus_lengths(dev, L):
    """pydub speedup at 1 - 13 s: up to ~80 chunk launches; 64001 ends one frame into a new millisecond, 150017 a partial last slice"""
    x = _speech(L, L, amp=0.8)
    x[1000:1040] = 1.2                                 # wrap-around in the int16 conversion, saturation in the overlays
    for f in FACTORS:
        ref = SP.speed(x, f)
        got = _np(AUG.speed(torch.from_numpy(x).to(dev), f))
        assert got.shape == ref.shape and np.array_equal(got.astype(np.int32), ref.astype(np.int32)), (L, f)
    print("speed L %d: bit-exact for %d factors" % (L, len(FACTORS)))


# ---- 4. pitch ----------------------------------------------------------------------------------------------------------------------
def _pitch_signal(kind, L):
    if kind == "noise":
        return (0.1 * np.random.RandomState(L).randn(L)).astype(np.float32)
    t = np.arange(L) / 16000.0
    rs = np.random.RandomState(L + 1)
    return (0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1230 * t + 1.0) + 0.01 * rs.randn(L)).astype(np.float32)


def _c64(flat, frames):
    return torch.view_as_complex(flat.view(frames, 1025, 2)).cpu().numpy().T


def _to_dev_c64(D, dev):
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(D.T)).to(dev)).contiguous()


PITCH_CASES = [(L, kind) for L in (64000, 211000) for kind in ("harmonic", "noise")]


@pytest.mark.parametrize("L,kind", PITCH_CASES)
def test_pitch_stages_at_corpus_lengths(dev, L, kind):
    """STFT (126 / 413 frames; 211000 is not a multiple of 512); the phase vocoder fed the oracle's STFT, checked without
    accumulating over steps: magnitudes, the initial phase, and every step's phase increment against the oracle's float64 increment
    (oracle.audio_speed_pitch.phase_increment_errors); the iSTFT fed the oracle's vocoder output, last frames included."""
    torch.cuda.synchronize()
    y = _pitch_signal(kind, L)
    nfr = ops.stft_nframes(L)
    D = torch.empty(nfr * 1025 * 2, device=dev)
    ops.stft(torch.from_numpy(y).to(dev), L, D, nfr)
    Dg, Dr = _c64(D, nfr), SP.stft(y)
    e_stft = float(np.abs(Dg - Dr).max() / np.abs(Dr).max())
    assert Dg.shape == Dr.shape and e_stft < STFT_REL, e_stft
    Din = _to_dev_c64(Dr, dev)
    for n_steps in (-1, 0, 1):
        rate = 2.0 ** (-n_steps / 12)
        nsteps = len(np.arange(0, nfr, rate))
        Ds = torch.empty(nsteps * 1025 * 2, device=dev)
        ops.phase_vocoder(Din, nfr, rate, Ds, nsteps)
        out, ref = _c64(Ds, nsteps), SP.phase_vocoder(Dr, rate)
        assert out.shape == ref.shape
        am, ar = np.abs(out).astype(np.float64), np.abs(ref).astype(np.float64)
        e_mag = float(np.abs(am - ar).max() / ar.max())
        live0 = ar[:, 0] > 1e-6 * ar.max()
        d0 = np.abs(SP.wrap_pi(np.angle(out[:, 0].astype(np.complex128)) - np.angle(Dr[:, 0]).astype(np.float64)))[live0]
        e_ph0 = float(d0.max() / np.spacing(np.float32(np.pi)))
        inc_ratio, inc_err, n_chk = SP.phase_increment_errors(out, Dr, rate, c=PV_INC_C)
        live = ar > 1e-6 * ar.max()
        drift = float(np.abs(SP.wrap_pi(np.angle(out.astype(np.complex128)) - np.angle(ref.astype(np.complex128))))[live].max())
        length = int(round(L / rate))
        nuse = min(nsteps, int(np.ceil((length + 2048) / 512)))
        ws, ys = torch.empty(nuse * 2048, device=dev), torch.empty(length, device=dev)
        ops.istft(_to_dev_c64(ref, dev), nuse, ws, ys, length)
        e_istft = float(np.abs(_np(ys) - SP.istft(ref, length)).max())
        print("pitch stages L %d %s n %+d (%d frames -> %d): stft %.2e, pv |mag| %.2e, phase0 %.1f ulp(pi), increments %.3f of the bound "
              "(%.1e rad, %d checked), accumulated phase drift %.1e rad, istft %.2e" % (L, kind, n_steps, nfr, nsteps, e_stft, e_mag, e_ph0,
                                                                                        inc_ratio, inc_err, n_chk, drift, e_istft))
        assert e_mag <= PV_MAG_REL, e_mag
        assert e_ph0 <= PV_PHASE0_ULP, e_ph0
        assert n_chk > 0.5 * out.size and inc_ratio <= 1.0, (inc_ratio, n_chk)
        assert e_istft <= ISTFT_ABS, e_istft


@pytest.mark.parametrize("n_in", [60000, 150001, 220000])
def test_resampler_at_corpus_lengths(dev, n_in):
    x = _pitch_signal("noise", n_in)
    worst = worst_ulp = 0.0
    for ratio in (2.0 ** (1 / 12), 2.0 ** (-1 / 12)):
        n_out = int(math.ceil(n_in * ratio))
        out = torch.empty(n_out, device=dev)
        ops.resample_sinc(torch.from_numpy(x).to(dev), n_in, ratio, out, n_out)
        got, ref = _np(out), SP.resample_sinc(x, ratio)
        e = float(np.abs(got - ref).max())
        ulps = float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref))).max())
        worst, worst_ulp = max(worst, e), max(worst_ulp, ulps)
        assert e <= RESAMPLE_ABS and ulps <= RESAMPLE_ULP, (ratio, e, ulps)
    print("resampler n_in %d: worst |err| %.2e, %.1f float32 steps of the output" % (n_in, worst, worst_ulp))


def _frame_spectrum_rel(got, ref):
    """per 2048-sample frame (hop 512) of the int16 outputs: || |G| - |R| || / || R ||, worst over frames with energy"""
    G, R = np.abs(SP.stft(got / 32768.0)), np.abs(SP.stft(ref / 32768.0))
    nr = np.linalg.norm(R, axis=0)
    live = nr > 1e-3 * nr.max()
    return float((np.linalg.norm(G - R, axis=0)[live] / nr[live]).max())


def _pitch_e2e(dev, x, n):
    ref = SP.pitch(x, n).astype(np.float64)
    got = _np(AUG.pitch_shift(torch.from_numpy(x).to(dev), n)).astype(np.float64)
    assert got.shape == ref.shape == x.shape
    return got, ref, float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(np.abs(got - ref).max()), float((np.abs(got - ref) > 1).mean())


@pytest.mark.parametrize("L,kind", PITCH_CASES)
def test_pitch_end_to_end_at_corpus_lengths(dev, L, kind):
    """augment.pitch_shift against oracle pitch at 4 and 13 s: rel-L2 of the int16 output, per-frame magnitude spectra (insensitive to
    the phase drift of the float32 accumulators), and for the harmonic signal the 440 Hz partial at 440 * 2^(n/12)."""
    x = _pitch_signal(kind, L)
    for n in (-1, 0, 1):
        got, ref, rel, mx, frac = _pitch_e2e(dev, x, n)
        fr = _frame_spectrum_rel(got, ref)
        print("pitch e2e L %d %s n %+d: rel-L2 %.2e, max |diff| %.0f LSB, > 1 LSB on %.3f %%, worst frame spectrum %.2e" % (
            L, kind, n, rel, mx, 100 * frac, fr))
        assert rel <= PITCH_REL_L2 and fr <= PITCH_FRAME_REL, (rel, fr)
        if kind == "harmonic":
            seg = got[2048:-2048]
            spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
            peak = np.argmax(spec[: int(800 * len(seg) / 16000)]) * 16000.0 / len(seg)
            assert abs(peak - 440 * 2 ** (n / 12)) < 3.0, (n, peak)


# ---- 5. a conf-5 pack at trim length 64000 ---------------------------------------------------------------------------------------
def _flac(path, q):
    from flac_writer import write_flac
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(write_flac(q.astype(np.int64), 16000, 16, 4096))


def _wav(path, q):
    import wave
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(q.astype("<i2").tobytes())


def _q(x):
    return np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)


@pytest.fixture
def recorder(monkeypatch):
    """wraps the augmenters, the fast RawBoost draws and the crop: each wrapper keeps (inputs, output) and returns the output"""
    rec = {k: [] for k in ("background_noise", "reverb", "speed", "pitch_shift", "rawboost_batch", "_fast_lnl", "_fast_isd", "multiview_crop")}

    def host(v):
        return _np(v) if torch.is_tensor(v) else v

    for name in rec:
        def wrap(*a, _orig=getattr(AUG, name), _name=name, **kw):
            state = np.random.get_state() if _name == "multiview_crop" else None
            out = _orig(*a, **kw)
            args = [[host(t) for t in v] if isinstance(v, list) else host(v) for v in a]
            rec[_name].append((args, kw, host(out) if torch.is_tensor(out) else out, state))
            return out
        monkeypatch.setattr(AUG, name, wrap)
    return rec


def test_conf5_pack_at_trim_64000_against_the_oracles(dev, tmp_path, recorder):
    """datautils.asvspoof_2019_augall_5 with configs/conf-5-linear.yaml's augmenters, the fast RawBoost sampler (main.py's), FLAC
    utterances of 211 003 and 50 021 samples (the second shorter than the trim: repeat_pad), 480 000-sample MUSAN files, RIRs of 16 000
    and 4000 taps.  Every augmenter's output is checked against its oracle given the recorded input and draws, with the bars above,
    and the finished [64000, V] pack against oracle.multiview applied to the recorded views with the crop's recorded draw, bit-exact."""
    import yaml
    import datautils.asvspoof_2019_augall_5 as D
    from scl_amd.datautils_common import default_rawboost_args
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "conf-5-linear.yaml")))["data"]["kwargs"]
    methods = list(cfg["augmentation_methods"])
    assert methods == ["RawBoost12", "background_noise_wrapper", "reverb_wrapper", "speed_wrapper", "pitch_wrapper"]
    root = str(tmp_path / "data")
    lens = {"LA_T_0.flac": 211003, "LA_T_1.flac": 50021, "LA_T_2.flac": 70000}
    files = {}
    for i, (u, n) in enumerate(lens.items()):
        files["bonafide/" + u] = _q(_speech(n, 10 + i, amp=0.4))
        for v in cfg["vocoders"]:
            files["vocoded/%s_%s" % (v, u)] = _q(_speech(n - 300, 20 + i, amp=0.3))
        files["spoof/s_" + u] = _q(0.1 * np.random.RandomState(30 + i).randn(66000 + 1000 * i))
    for p, q in files.items():
        _flac(os.path.join(root, p), q)
    for i in range(2):
        _wav(os.path.join(root, "musan", "n%d.wav" % i), _q(0.05 * (1 + i) * np.random.RandomState(40 + i).randn(480000)))
    _wav(os.path.join(root, "rir16000", "r.wav"), _q(_rir(16000, 50)))
    _wav(os.path.join(root, "rir4000", "r.wav"), _q(_rir(4000, 51)))
    args = default_rawboost_args()
    args.device, args.is_train, args.rawboost_sampler = "cuda:0", True, "fast"
    ds = D.Dataset_for(args, list_IDs=list(lens), labels=[], base_dir=root + "/", algo=5, vocoders=cfg["vocoders"],
                       augmentation_methods=methods, num_additional_real=cfg["num_additional_real"],
                       num_additional_spoof=cfg["num_additional_spoof"], trim_length=64000, wav_samp_rate=16000, online_aug=True,
                       aug_dir=str(tmp_path / "aug"), noise_path=os.path.join(root, "musan"), rir_path=None, repeat_pad=True)
    nv = len(cfg["vocoders"])
    for idx, rirdir, seed in ((0, "rir16000", 1), (1, "rir4000", 2)):
        for v in recorder.values():
            v.clear()
        args.rir_path = os.path.join(root, rirdir)
        AUG.seed_fast_sampler(seed)
        np.random.seed(seed); random.seed(seed)
        uid, data, label = ds[idx]
        pack = _np(data).T                                                          # [V, 64000]
        u = list(lens)[idx]
        real = files["bonafide/" + u].astype(np.float32) / 32768.0
        V = 1 + len(methods) + cfg["num_additional_real"] + 2 * nv + cfg["num_additional_spoof"]
        assert uid == u and pack.shape == (V, 64000) and label.numel() == V
        # RawBoost (algo 5: LnL then ISD), once per vocoded file and once on the anchor: the oracle given the recorded draws
        rb = recorder["rawboost_batch"]
        assert len(rb) == nv + 1 and len(recorder["_fast_lnl"]) == len(recorder["_fast_isd"]) == nv + 1
        rb_err = 0.0
        for (a, _, y, _), lnl, isd in zip(rb, recorder["_fast_lnl"], recorder["_fast_isd"]):
            xin = a[0][0]
            ref = RB.isd_apply(RB.lnl_apply(xin, lnl[2][0]), isd[2][0][0], isd[2][0][1], args.g_sd)
            rb_err = max(rb_err, float(np.abs(y[0].astype(np.float64) - ref).max()))
        assert rb_err < 3e-5, rb_err
        assert np.array_equal(rb[nv][0][0][0], real)                               # the anchor's RawBoost view got the anchor
        # MUSAN overlay: bit-exact
        (a, kw, y, _), = recorder["background_noise"]
        assert np.array_equal(a[0], real) and a[1].size == 480000
        host_power = kw.get("sumsq") is not None
        ref, _ = AI.background_noise(a[0], a[1], a[2])
        assert np.array_equal(y, ref.astype(np.float32))
        # RIR: up to ties
        (a, _, y_rev, _), = recorder["reverb"]
        assert np.array_equal(a[0], real) and a[1].size == int(rirdir[3:])
        y64, S = RT.conv_refs(a[0], a[1])
        y_gpu = _np(_gpu_conv(torch.from_numpy(a[0]).to(dev), torch.from_numpy(a[1]).to(dev)))
        n_ties, _, _, _ = RT.check_up_to_ties("pack reverb", y_rev, AI.reverb(a[0], a[1]), y64, S, [y_gpu, np.convolve(a[0], a[1])])
        # speed: bit-exact; pitch: the long-clip bars
        (a, _, y, _), = recorder["speed"]
        assert np.array_equal(a[0], real) and np.array_equal(y.astype(np.int32), SP.speed(a[0], a[1]).astype(np.int32)), a[1]
        (a, _, y, _), = recorder["pitch_shift"]
        pref = SP.pitch(a[0], a[1]).astype(np.float64)
        prel = float(np.linalg.norm(y - pref) / max(np.linalg.norm(pref), 1e-30))
        pfr = _frame_spectrum_rel(y.astype(np.float64), pref)
        assert np.array_equal(a[0], real) and prel <= PITCH_REL_L2 and pfr <= PITCH_FRAME_REL, (a[1], prel, pfr)
        # the crop: the views it was handed are the loaded files and the recorded augmenter outputs, in the plugin's order
        (a, kw, y, state), = recorder["multiview_crop"]
        views = a[0]
        assert len(views) == V and np.array_equal(views[0], real)
        outs = [rb[nv][2][0], recorder["background_noise"][0][2], y_rev, recorder["speed"][0][2], recorder["pitch_shift"][0][2]]
        for k, o in enumerate(outs):
            assert np.array_equal(views[1 + k], o), methods[k]
        for k in range(nv):
            assert np.array_equal(views[1 + len(methods) + cfg["num_additional_real"] + nv + k], rb[k][2][0]), k
        rng = np.random.RandomState()
        rng.set_state(state)
        ref = OM.batch_pad_for_multiview([v.reshape(-1, 1) for v in views], 16000, 64000, random_trim_nosil=True, repeat_pad=True, rng=rng)
        ref = np.stack([r[:, 0] for r in ref]).astype(np.float32)
        assert np.array_equal(pack, ref)
        print("conf-5 pack %s (%d samples, RIR %s): %d views; RawBoost worst %.2e, noise (%s power) / speed bit-exact, reverb %d ties, "
              "pitch n %+d rel-L2 %.2e frame %.2e; pack bit-exact" % (u, real.size, rirdir[3:], V, rb_err, "host" if host_power else "device",
                                                                      n_ties, recorder["pitch_shift"][0][0][1], prel, pfr))
