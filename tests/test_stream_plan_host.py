"""CPU: the window plan of a live-stream push (shz_stream_plan) and the locality argument behind it, on the oracle.

A stream is fingerprinted push by push: each push extracts the window clip the plan names, keeps the peaks of the newly
settled frames, and emits the hashes of the settled peaks that can no longer gain a partner.  Every window and the whole
signal go through the same numpy functions (cpu_ref.spectrogram_db + peaks_2d), so the concatenated output must equal
cpu_ref.fingerprint_keys(whole) bit for bit -- any difference is a frame the plan got wrong.  No GPU."""
import os

import numpy as np
import pytest

from oracle import cpu_ref as O
from oracle import synth
from shazam_amd import _ffi

FAN = 5


def _stream_oracle(x, bounds, wratio=0.5, fan=FAN, fs=44100):
    """Push x[bounds[i]:bounds[i+1]] chunk by chunk, the last push ending the stream.  Returns (keys, t1) emitted in order
    and, per push, (settled_after, number emitted)."""
    hop = 4096 - int(4096 * wratio)
    pend_f = np.zeros(0, np.int64)
    pend_t = np.zeros(0, np.int64)
    settled = 0
    keys, t1s, log = [], [], []
    for i in range(len(bounds) - 1):
        ending = i == len(bounds) - 2
        wf0, ws0, ws1, h = _ffi.stream_plan(bounds[i], bounds[i + 1], settled, hop, ending)
        assert ws0 == wf0 * hop and h >= settled
        if ws1 > ws0:
            assert h > settled
            A = O.spectrogram_db(x[ws0:ws1], fs, 4096, wratio)
            f, t = O.sort_peaks(*O.peaks_2d(A))
            keep = (t >= settled - wf0) & (t < h - wf0)
            pend_f = np.concatenate([pend_f, f[keep]])
            pend_t = np.concatenate([pend_t, t[keep] + wf0])
        else:
            assert h == settled and not ending
        settled = h
        m = len(pend_t)
        if ending:
            e = m
        else:
            e = max(m - (fan - 1), int(np.searchsorted(pend_t, h - 200, side="left")) if h > 200 else 0, 0)
        n0 = len(keys)
        for a in range(e):
            for j in range(a + 1, min(a + fan, m)):
                dt = pend_t[j] - pend_t[a]
                if 0 <= dt <= 200:
                    keys.append(int(O.pack_key(pend_f[a], pend_f[j], dt)))
                    t1s.append(int(pend_t[a]))
        log.append((h, len(keys) - n0))
        pend_f, pend_t = pend_f[e:], pend_t[e:]
        assert len(pend_t) <= fan - 1 or ending
    return np.array(keys, np.uint32), np.array(t1s, np.uint32), log


def _schedules(n, seed):
    rng = np.random.default_rng(seed)
    hop = 2048
    out = {}
    cuts = np.sort(rng.integers(0, n + 1, size=12))
    out["random"] = [0] + cuts.tolist() + [n]                     # includes zero-length chunks where cuts repeat
    out["with_empties"] = [0, 0, 5000, 5000, 5000, n // 2, n // 2, n]
    on_hop = list(range(0, n, 16 * hop)) + [n]                     # chunks ending exactly on a hop boundary
    out["on_hop"] = on_hop
    out["off_hop"] = [0] + [min(n, b + 1) for b in on_hop[1:-1]] + [n]   # ... and one sample past it
    out["single_then_big"] = list(range(0, min(n, 9000))) + [min(n, 9000), n]   # single samples, then one large chunk
    out["one_push"] = [0, n]
    return out


def _check(x, bounds, wratio=0.5, fan=FAN):
    bounds = [int(b) for b in bounds]
    assert bounds == sorted(bounds)
    k, t1, _ = _stream_oracle(x, bounds, wratio, fan)
    wk, wt1, _, _ = O.fingerprint_keys(x, wratio=wratio, fan_value=fan)
    assert np.array_equal(k, wk) and np.array_equal(t1, wt1), (len(k), len(wk))


@pytest.mark.parametrize("clip", [0, 1])
def test_synth_clip_schedules(clip):
    x = synth.synth_clip(77, clip, 441000, 4000 * clip, 8000)     # 10 s: white noise / tonal + noise
    for name, b in _schedules(len(x), 100 + clip).items():
        _check(x, b)


def test_other_overlap():
    x = synth.synth_clip(78, 3, 441000, 4000, 1500)
    rng = np.random.default_rng(5)
    b = [0] + np.sort(rng.integers(0, len(x), 20)).tolist() + [len(x)]
    _check(x, b, wratio=0.75)
    _check(x, [0, len(x)], wratio=0.75)
    _check(x, list(range(0, len(x), 8192)) + [len(x)], wratio=0.25)


def test_edge_case_lengths():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "edge_cases.npz"))
    for name in ("short_3000", "exact_4096", "ragged_6143", "two_frames_6144"):
        x = g[f"{name}_pcm"]
        n = len(x)
        for b in ([0, n], [0, 1, n], [0, n // 2, n], [0, 2048, 4095, 4096, n] if n >= 4096 else [0, 2048, n],
                  list(range(0, n + 1, 1000)) + ([n] if n % 1000 else [])):
            _check(x, sorted(set(b) | {0, n}))


def test_fan_one_and_long_fan():
    x = synth.synth_clip(79, 0, 220500, 4000, 4000)
    b = list(range(0, len(x), 8192)) + [len(x)]
    _check(x, b, fan=1)
    _check(x, b, fan=20)


def test_plan_contract():
    hop = 2048
    # nothing settles before frame 10 + 1 is complete
    assert _ffi.stream_plan(0, 4096 + 10 * hop - 1, 0, hop) == (0, 0, 0, 0)
    wf0, ws0, ws1, h = _ffi.stream_plan(0, 4096 + 10 * hop, 0, hop)
    assert (wf0, ws0, h) == (0, 0, 1) and ws1 == 4096 + 10 * hop
    # a later push starts its window 10 frames in front of the horizon
    wf0, ws0, ws1, h = _ffi.stream_plan(100000, 200000, 30, hop)
    assert wf0 == 20 and ws0 == 20 * hop and h == (200000 - 4096) // hop + 1 - 10 and ws1 == (h + 9) * hop + 4096
    # at the end every frame settles; a stream shorter than one frame has one zero-padded frame
    assert _ffi.stream_plan(0, 3000, 0, hop, True) == (0, 0, 3000, 1)
    assert _ffi.stream_plan(0, 0, 0, hop, True) == (0, 0, 0, 1)
    for bad in ((10, 5, 0, hop), (0, 10, 0, 0), (0, 10, 0, 4097), (0, 5000, 3, hop)):
        with pytest.raises(_ffi.ShzError):
            _ffi.stream_plan(*bad)
