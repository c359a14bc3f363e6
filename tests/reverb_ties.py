"""Ties of the int16 reverb output (test helper).  reverb.py:33-44 truncates 32768 * y / max|y| of a float32 convolution toward zero;
two float32 evaluations of y (the HIP kernels, numpy's np.convolve) can truncate to different integers only where the exact value lies
within their measured error of an integer.  The fixed bars below hold both evaluations (tests/test_augmenters_train_gpu.py::
test_reverb_convolution_against_float64, MI355X); the tie band of a case is built from the errors measured on that very case."""
import numpy as np
from scipy.signal import fftconvolve

CONV_REL_SUM = 4e-6     # |y32 - y64| / sum_t |x[m - t]| |h[t]| per sample.  measured: HIP 1.5e-6 (fir_kernel, 700 taps under a dominant
                        # spike), 4.9e-7 (golden "short", 900 taps), 3.5e-7 (1023 taps), Toeplitz GEMM 2.3e-7; numpy 8.1e-8
CONV_REL_MAX = 4e-6     # |y32 - y64| / max|y64|.  measured: HIP 2.2e-6 (fir_kernel, 1023 taps), GEMM 1.7e-6; numpy 5.9e-7


def conv_refs(x, h):
    """float64 convolution and the per-sample magnitude scale sum_t |x[m - t]| |h[t]|"""
    x64, h64 = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    return fftconvolve(x64, h64), fftconvolve(np.abs(x64), np.abs(h64))


def conv_errors(y32, y64, S):
    """(worst |err| / sum|x||h|, worst |err| / max|y64|)"""
    e = np.abs(np.asarray(y32, dtype=np.float64) - y64)
    return float((e / S).max()), float(e.max() / np.abs(y64).max())


def tie_band(y64, S, eps_sum, eps_max):
    """how far from an integer the exact value v = 32768 y / max|y| may lie for two evaluations, each within eps_sum * S[m] of y64 at
    every sample and within eps_max * max|y| anywhere (so also at the peak: the scale), to truncate apart; plus the quantisers' own
    rounding (reciprocal and product on the GPU, the division in numpy: < 2^-21 of full scale)"""
    M = np.abs(y64).max()
    return 32768.0 * (eps_sum * S / M + np.abs(y64) / M * eps_max) + 32768.0 * 2.0 ** -21


def check_up_to_ties(tag, got, ref, y64, S, convs, bars=(CONV_REL_SUM, CONV_REL_MAX), max_frac=1e-2):
    """got == ref except at ties, and there off by one LSB or the +-32768 wrap of the peak sample (+1.0 * 32768 wraps to -32768).  The
    band is built from the errors of the float32 convolutions `convs` behind got and ref, measured here against y64 (and held to
    `bars` first); at most `max_frac` of the samples may be ties.  Returns (ties taken, median band in LSB, fraction of samples inside the band, the measured errors)."""
    errs = [conv_errors(y, y64, S) for y in convs]
    assert all(es <= bars[0] and em <= bars[1] for es, em in errs), (tag, errs)
    got, ref = np.asarray(got, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    v = 32768.0 * y64 / np.abs(y64).max()
    dist = np.abs(v - np.round(v))
    band = tie_band(y64, S, max(e[0] for e in errs), max(e[1] for e in errs))
    d = np.abs(got - ref)
    wrap = d == 65535
    bad = d != 0
    assert np.all(d[bad & ~wrap] == 1), (tag, np.unique(d[bad]))
    assert np.all(dist[bad] <= band[bad]), (tag, float((dist[bad] - band[bad]).max()))
    assert bad.mean() < max_frac, (tag, bad.mean())
    return int(bad.sum()), float(np.median(band)), float((dist <= band).mean()), errs
