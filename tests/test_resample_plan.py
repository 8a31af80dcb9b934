"""CPU: the resampler's filter design (shazam_amd/resample.py) -- ratios, tap counts, exact DC gain, frequency response, refusals."""
import math

import numpy as np
import pytest

from resample_twin import resample_twin
from shazam_amd import resample as R

PAIRS = [(8000, 44100), (11025, 44100), (16000, 44100), (22050, 44100), (32000, 44100), (48000, 44100), (96000, 44100),
         (44100, 48000)]
LM = {(8000, 44100): (441, 80), (11025, 44100): (4, 1), (16000, 44100): (441, 160), (22050, 44100): (2, 1),
      (32000, 44100): (441, 320), (48000, 44100): (147, 160), (96000, 44100): (147, 320), (44100, 48000): (160, 147)}


@pytest.mark.parametrize("pair", PAIRS)
def test_ratio_and_tap_count(pair):
    L, M, T, taps = R.resample_plan(*pair)
    assert (L, M) == LM[pair]
    assert T == 2 * math.ceil(16 * max(1.0, M / L)) and T % 2 == 0
    assert taps.shape == (L, T) and taps.dtype == np.int32
    assert R.resample_plan(*pair)[3] is taps   # cached per rate pair


def test_tap_count_of_the_issue_example():
    assert R.resample_plan(96000, 44100)[2] == 70
    assert R.resample_plan(48000, 44100, zero_crossings=8)[2] == 2 * math.ceil(8 * 160 / 147)


@pytest.mark.parametrize("pair", PAIRS)
def test_every_phase_sums_to_one(pair):
    L, M, T, taps = R.resample_plan(*pair)
    assert np.all(taps.astype(np.int64).sum(axis=1) == 1 << 30)


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("value", [1, -32768, 32767, 12345])
def test_twin_keeps_a_constant(pair, value):
    L, M, T, taps = R.resample_plan(*pair)
    n = 6 * T + 50
    y = resample_twin(np.full(n, value, np.int16), L, M, T, taps)
    assert len(y) == -(-n * L // M)
    i0 = (np.arange(len(y), dtype=np.int64) * M) // L + T // 2
    inner = (i0 - (T - 1) >= T) & (i0 < n - T)     # further than T inputs from either edge
    assert inner.sum() > 0 and np.all(y[inner] == value)


def _response(L, T, taps):
    """|H| of the prototype h[k L + p] = taps[p][k] at the upsampled rate, DC gain L taken out; f in cycles per sample."""
    h = taps.astype(np.float64).T.reshape(-1) / (L * 2.0 ** 30)
    nfft = 1 << int(np.ceil(np.log2(L * T * 16)))
    return np.arange(nfft // 2 + 1) / nfft, np.abs(np.fft.rfft(h, nfft))


@pytest.mark.parametrize("pair", PAIRS)
def test_frequency_response(pair):
    """Stopband >= 80 dB down beyond cutoff + df / 2, passband within 0.01 dB below cutoff - df / 2, df = Kaiser's transition
    width for beta = 9 (A = beta / 0.1102 + 8.7 = 90.4 dB) and the prototype's length N = L T: (A - 7.95) / (14.36 (N - 1)).
    Measured for these pairs: stopband -89.2 .. -90.7 dB, passband deviation <= 0.0004 dB."""
    L, M, T, taps = R.resample_plan(*pair)
    f, H = _response(L, T, taps)
    A = 9.0 / 0.1102 + 8.7
    df = (A - 7.95) / (14.36 * (L * T - 1))
    fc = 0.5 / max(L, M)
    stop = 20 * np.log10(H[f >= fc + df / 2].max())
    ripple = np.abs(20 * np.log10(H[f <= fc - df / 2])).max()
    assert stop <= -80.0
    assert ripple <= 0.01


def test_refusals_name_the_limit():
    with pytest.raises(NotImplementedError, match=str(R.MAX_TAPS)):
        R.resample_plan(44100 * 300, 44100)                  # T = 2 * 16 * 300
    with pytest.raises(NotImplementedError, match=str(R.MAX_TABLE)):
        R.resample_plan(44100, 1048583)                      # coprime: L = 1,048,583, L * T = 33.5 M taps
    with pytest.raises(ValueError):
        R.resample_plan(0, 44100)


def test_equal_rates_are_a_copy():
    x = np.arange(-5, 5, dtype=np.int16)
    (y,) = R.resample_batch([x], 44100, 44100)
    assert np.array_equal(y, x) and y is not x
