"""Test helpers for recognition under two warp factors (not a conftest, not collected): the integer warp of
shz_warp_pair_hash_tf stated in numpy, the best-variant rule, and the note corpus the tests cut their songs and their
time-stretched / pitch-shifted queries from, which is not made by the code under test."""
import numpy as np

from oracle import cpu_ref as O
from oracle import synth
from speed_twin import F_MAX, S_ONE, aligned_votes, q16, table_of  # noqa: F401  (re-exported for the tests)


def warp_peaks_tf(f, t, t16: int, f16: int):
    """The peaks (f, t) of a query that runs t16 / 65536 times as fast and sounds f16 / 65536 times as high as the table's
    copy, mapped to the table's domain: t' = (t t16 + 32768) >> 16, f' = (2 65536 f + f16) // (2 f16) in 64-bit integers,
    peaks with f' > 2048 dropped, the rest ordered by (t', f', original index).  Returns (f', t') as int64."""
    f, t, t16, f16 = np.asarray(f).astype(np.int64), np.asarray(t).astype(np.int64), int(t16), int(f16)
    tp = (t * t16 + 32768) >> 16
    fp = (2 * S_ONE * f + f16) // (2 * f16)
    keep = np.flatnonzero(fp <= F_MAX)
    order = keep[np.lexsort((keep, fp[keep], tp[keep]))]
    return fp[order], tp[order]


def warp_pair_tf(f, t, t16: int, f16: int, fan_value: int = 5):
    """(key32, t1) of the warped peaks, paired like generate_hashes (oracle.cpu_ref.pair_keys)."""
    return O.pair_keys(*warp_peaks_tf(f, t, t16, f16), fan_value)


def warp_pair_batch_tf(peak_f, peak_t, peak_off, query_clip0, tempos, pitches, fan_value: int = 5):
    """shz_warp_pair_hash_tf in numpy: (key32, t1, hash_off) in the library's order -- for query q, for warp v, for every
    clip c of q: the hashes of (c, v); hash_off has n_clips * n_warps + 1 entries in that order."""
    assert len(tempos) == len(pitches)
    ks, ts, off = [], [], [0]
    for q in range(len(query_clip0) - 1):
        for t16, f16 in zip(tempos, pitches):
            for c in range(int(query_clip0[q]), int(query_clip0[q + 1])):
                a, b = int(peak_off[c]), int(peak_off[c + 1])
                k, t1 = warp_pair_tf(peak_f[a:b], peak_t[a:b], int(t16), int(f16), fan_value)
                ks.append(k)
                ts.append(t1)
                off.append(off[-1] + len(k))
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)
    return cat(ks), cat(ts), np.asarray(off, np.uint64)


def best_variant_tf(top1_aligned, tempos, pitches) -> int:
    """Index of the greatest top-1 aligned count; ties to the smaller |t16 - 65536| + |f16 - 65536|, then to the lower
    index."""
    return min(range(len(tempos)), key=lambda v: (-int(top1_aligned[v]),
                                                  abs(int(tempos[v]) - S_ONE) + abs(int(pitches[v]) - S_ONE), v))


NOTE_LEN = tuple(1 << s for s in synth.MUSIC_LEN_SHIFT)       # 16384, 32768, 8192, 4096 samples
NOTE_AMP, BURST_AMP, BED_AMP = 3000.0, 1500.0, 100.0
MAX_NOTES = 4096                                               # per voice and clip: 6 minutes of the shortest notes


def notes_clip(seed: int, clip: int, seconds: float, tempo: float = 1.0, pitch: float = 1.0, rate: int = 44100) -> np.ndarray:
    """`seconds` of a note-based, music-like clip rendered in float: synth.music_clip's four voices (note lengths 16384,
    32768, 8192, 4096 samples; octaves 1, 1, 1, 2), every note eight harmonics with MUSIC_HARM weights and a linear decay
    over the note, voice 0's notes opened by a decaying white burst of 2,048 samples, a +-100 white bed.  The score (which
    notes, their start phases, their bursts) depends on (seed, clip) alone.  tempo divides every note boundary and the burst
    length -- the piece runs `tempo` times as fast, the pitch kept --, pitch multiplies every fundamental and reads the
    burst's noise `pitch` times as fast (linear interpolation), so everything that sounds moves by the one factor;
    harmonics above Nyquist are dropped.  int16."""
    n = int(round(seconds * rate))
    x = np.arange(n, dtype=np.float64)
    acc = np.random.default_rng([seed, clip, 0xBED]).uniform(-BED_AMP, BED_AMP, n)
    harm = np.asarray(synth.MUSIC_HARM, np.float64) / 256.0
    for v, L0 in enumerate(NOTE_LEN):
        L = L0 / float(tempo)
        n_notes = int(n / L) + 1
        assert n_notes <= MAX_NOTES
        rng = np.random.default_rng([seed, clip, v])            # one stream per voice, MAX_NOTES draws of each property:
        on = rng.integers(0, 16, MAX_NOTES) != 0                 # note k is the same note at any tempo and any length
        degree = rng.integers(0, 48, MAX_NOTES)
        detune = (63488 + rng.integers(0, 4096, MAX_NOTES)) / 65536.0
        phase = rng.uniform(0.0, 2 * np.pi, MAX_NOTES)
        burst_seed = rng.integers(0, 1 << 62, MAX_NOTES)
        f0 = 110.0 * 2.0 ** (degree / 12.0) * synth.MUSIC_OCTAVE[v] * detune * float(pitch)
        for k in range(n_notes):
            a, b = int(np.ceil(k * L)), min(int(np.ceil((k + 1) * L)), n)
            if not on[k] or a >= b:
                continue
            m = x[a:b] - k * L                                   # time inside the note, in samples of the query
            env = 1.0 - m / L
            s = np.zeros(b - a)
            for h in range(1, synth.MUSIC_NHARM + 1):
                if f0[k] * h < rate / 2:
                    s += harm[h - 1] * np.sin(phase[k] * h + 2 * np.pi * f0[k] * h / rate * m)
            acc[a:b] += NOTE_AMP * env * s
            if v == 0:
                lb = synth.MUSIC_BURST_LEN / float(tempo)
                nb = min(int(np.ceil(lb)), b - a)
                # the note's own white noise, read `pitch` times as fast: its spectrum moves with the pitch like the
                # harmonics do (a burst left in place would hand a pitch-shifted query its onsets' peaks unchanged)
                white = np.random.default_rng(int(burst_seed[k])).uniform(-BURST_AMP, BURST_AMP, int(lb * pitch) + 3)
                pos = np.maximum(m[:nb], 0.0) * float(pitch)
                acc[a:a + nb] += np.interp(pos, np.arange(len(white), dtype=np.float64), white) * np.maximum(1.0 - m[:nb] / lb, 0.0)
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16)
