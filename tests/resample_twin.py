"""Test helpers for the resampler (not a conftest, not collected): the integer formula of shz_resample_i16 stated in numpy,
and songs defined as functions of time, so that their 48 kHz and 44.1 kHz versions are independent samplings of one signal
and neither is made by the code under test."""
import numpy as np


def resample_twin(x, L, M, T, taps, in_base=0, m_first=0, m_end=None):
    """out[m] = sat16((sum_k taps[p][k] x[i0 - k] + 2^29) >> 30), p = (m M) mod L, i0 = (m M) div L + T / 2, in int64;
    x[i] is the buffer's sample i - in_base inside the buffer and 0 elsewhere; m in [m_first, m_end), default all
    ceil(n L / M) outputs."""
    x = np.asarray(x).astype(np.int64)
    n = len(x)
    taps = np.asarray(taps).astype(np.int64).reshape(L, T)
    if m_end is None:
        m_end = -(-n * L // M)
    m = np.arange(m_first, m_end, dtype=np.int64)
    p, i0 = (m * M) % L, (m * M) // L + T // 2
    acc = np.zeros(len(m), np.int64)
    for k in range(T):
        idx = i0 - k - in_base
        ok = (idx >= 0) & (idx < n)
        acc += taps[p, k] * np.where(ok, x[np.clip(idx, 0, max(n - 1, 0))] if n else 0, 0)
    return np.clip((acc + (1 << 29)) >> 30, -32768, 32767).astype(np.int16)


def song_bursts(seed, seconds=30.0):
    """The score of a song: tone bursts (start s, duration s, frequency Hz, amplitude LSB, phase), 200-9000 Hz."""
    rng = np.random.default_rng(seed)
    n = int(seconds / 0.08)
    start = np.sort(rng.uniform(-0.2, seconds, n))
    return np.stack([start, rng.uniform(0.15, 0.45, n), rng.uniform(200.0, 9000.0, n), rng.uniform(1200.0, 4000.0, n),
                     rng.uniform(0.0, 2 * np.pi, n)], 1)


def song_at_rate(seed, fs, seconds=30.0, t0=0.0, noise_sigma=30.0):
    """int16 samples of song `seed` at rate fs, from time t0: every burst is a Hann-shaped tone evaluated at n / fs.  Tones
    at or above 0.45 fs are left out, as the anti-alias filter of a converter at that rate leaves them out.  The noise
    floor is drawn per (seed, fs): no two rates share a sample."""
    n = int(round(seconds * fs))
    t = t0 + np.arange(n, dtype=np.float64) / fs
    x = np.zeros(n, np.float64)
    for s, d, f, a, ph in song_bursts(seed, 30.0):
        if f >= 0.45 * fs:
            continue
        i0, i1 = np.searchsorted(t, s), np.searchsorted(t, s + d)
        if i1 <= i0:
            continue
        tt = t[i0:i1]
        x[i0:i1] += a * np.sin(np.pi * (tt - s) / d) ** 2 * np.sin(2 * np.pi * f * tt + ph)
    x += np.random.default_rng([seed, int(fs)]).normal(0.0, noise_sigma, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
