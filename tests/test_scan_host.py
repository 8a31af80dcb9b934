"""CPU: the host half of scanning (include/shz.h at shz_scan_*): the window count against its formula, and the timeline fold
shz_scan_timeline against a Python twin written here from the contract -- hand-built window sequences for every rule of
the fold, then a few hundred seeded random ones."""
import numpy as np
import pytest

from shazam_amd import _ffi


# ---- twins ------------------------------------------------------------------------------------------------------------
def window_count_twin(frames, window, step):
    if frames == 0:
        return 0                      # a recording without clips
    if frames <= window:
        return 1
    return -(-(frames - window) // step) + 1


def timeline_twin(win_off, sid, delta, aligned, nres, step, min_aligned, max_gap):
    """[(rec, sid, shift, first, last, hits, best)]; sid / delta / aligned are [n_windows, topn], rank 0 is read."""
    segs = []
    for r in range(len(win_off) - 1):
        cur = None
        for w in range(int(win_off[r + 1]) - int(win_off[r])):
            g = int(win_off[r]) + w
            if int(nres[g]) < 1 or int(aligned[g][0]) < min_aligned:
                continue
            ident = (int(sid[g][0]), int(delta[g][0]) - w * step)
            if cur is not None and (cur[1], cur[2]) == ident and w - cur[4] - 1 <= max_gap:
                cur[4] = w
                cur[5] += 1
                cur[6] = max(cur[6], int(aligned[g][0]))
                continue
            if cur is not None:
                segs.append(tuple(cur))
            cur = [r, ident[0], ident[1], w, w, 1, int(aligned[g][0])]
        if cur is not None:
            segs.append(tuple(cur))
    return segs


def _lib_segments(win_off, sid, delta, aligned, nres, step, min_aligned, max_gap):
    s = _ffi.scan_timeline(win_off, sid, delta, aligned, nres, step, min_aligned, max_gap)
    assert s["shift"].dtype == np.int64
    return [tuple(int(s[k][i]) for k, _ in _ffi.SEGMENT_FIELDS) for i in range(len(s["rec"]))]


def _cols(rows, topn=1, filler=(77, 12345, 999)):
    """rows: (sid, delta, aligned, nres) per window -> arrays of stride topn whose other ranks hold `filler`."""
    n = len(rows)
    sid, delta, aligned = (np.full((n, topn), f, d) for f, d in zip(filler, (np.uint32, np.int32, np.uint32)))
    for i, (s, d, a, _) in enumerate(rows):
        sid[i, 0], delta[i, 0], aligned[i, 0] = s, d, a
    return sid, delta, aligned, np.array([r[3] for r in rows], np.uint32)


def _both(win_off, rows, step, min_aligned, max_gap, topn=1):
    sid, delta, aligned, nres = _cols(rows, topn)
    want = timeline_twin(win_off, sid, delta, aligned, nres, step, min_aligned, max_gap)
    assert _lib_segments(win_off, sid, delta, aligned, nres, step, min_aligned, max_gap) == want
    return want


# ---- the window count -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,step", [(108, 22), (5, 1), (3, 7), (1, 1), (7, 7), ((1 << 20) - 1, 1000)])
def test_window_count_is_the_formula(window, step):
    for frames in (0, 1, window - 1, window, window + 1, window + step - 1, window + step, window + step + 1,
                   window + 10 * step, window + 10 * step + 1, 343, 1 << 20):
        assert _ffi.scan_window_count(frames, window, step) == window_count_twin(frames, window, step), (frames, window, step)
    # with step <= window every frame lies in a window and the last window starts inside the recording (with step > window
    # frames between the windows are skipped, and the formula's last window may start behind the end: it is empty)
    if step <= window:
        for frames in (window + 1, window + step + 1, 5 * window + 3):
            w = _ffi.scan_window_count(frames, window, step)
            assert (w - 1) * step + window >= frames and (w - 1) * step < frames


def test_window_count_values():
    assert _ffi.scan_window_count(343, 108, 22) == 12          # the recipe of tests/test_gpu_scan.py
    assert _ffi.scan_window_count(30, 1, 1) == 30
    assert _ffi.scan_window_count(30, 4, 9) == 4               # step > window: frames between the windows are skipped
    assert _ffi.scan_window_count(1, 108, 22) == 1
    assert _ffi.scan_window_count(0, 108, 22) == 0


# ---- the fold, rule by rule -------------------------------------------------------------------------------------------
STEP = 22


def _hit(sid, shift, w, aligned=100):
    return (sid, shift + w * STEP, aligned, 1)


MISS = (9, 4, 0, 0)          # nres = 0: whatever the columns hold is not read as a hit


def test_extend_and_identity_change():
    rows = [_hit(2, -43, w) for w in range(8)] + [_hit(4, -194, w) for w in range(8, 12)]
    assert _both([0, 12], rows, STEP, 50, 1) == [(0, 2, -43, 0, 7, 8, 100), (0, 4, -194, 8, 11, 4, 100)]
    # the same song at another shift is another segment
    rows = [_hit(2, -43, 0), _hit(2, -43, 1), _hit(2, -44, 2), _hit(2, -44, 3)]
    assert _both([0, 4], rows, STEP, 50, 1) == [(0, 2, -43, 0, 1, 2, 100), (0, 2, -44, 2, 3, 2, 100)]
    # ... and another song at the same shift too
    rows = [_hit(2, -43, 0), _hit(3, -43, 1), _hit(2, -43, 2)]
    assert _both([0, 3], rows, STEP, 50, 5) == [(0, 2, -43, 0, 0, 1, 100), (0, 3, -43, 1, 1, 1, 100), (0, 2, -43, 2, 2, 1, 100)]


@pytest.mark.parametrize("max_gap", [0, 1, 2, 5])
def test_a_gap_at_max_gap_extends_and_one_past_it_does_not(max_gap):
    at = [_hit(5, 7, 0)] + [MISS] * max_gap + [_hit(5, 7, max_gap + 1)]
    assert _both([0, len(at)], at, STEP, 1, max_gap) == [(0, 5, 7, 0, max_gap + 1, 2, 100)]
    past = [_hit(5, 7, 0)] + [MISS] * (max_gap + 1) + [_hit(5, 7, max_gap + 2)]
    assert _both([0, len(past)], past, STEP, 1, max_gap) == [(0, 5, 7, 0, 0, 1, 100), (0, 5, 7, max_gap + 2, max_gap + 2, 1, 100)]


def test_min_aligned_at_above_and_below_the_count():
    rows = [_hit(1, 0, 0, aligned=50), _hit(1, 0, 1, aligned=49), _hit(1, 0, 2, aligned=51)]
    assert _both([0, 3], rows, STEP, 50, 1) == [(0, 1, 0, 0, 2, 2, 51)]        # 49 is no hit; the gap of one is bridged
    assert _both([0, 3], rows, STEP, 50, 0) == [(0, 1, 0, 0, 0, 1, 50), (0, 1, 0, 2, 2, 1, 51)]
    assert _both([0, 3], rows, STEP, 49, 0) == [(0, 1, 0, 0, 2, 3, 51)]
    assert _both([0, 3], rows, STEP, 52, 0) == []
    assert _both([0, 3], rows, STEP, 0, 0) == [(0, 1, 0, 0, 2, 3, 51)]


def test_nres_zero_is_no_hit_even_with_a_count_in_the_columns():
    rows = [_hit(1, 0, 0), (1, STEP, 500, 0), _hit(1, 0, 2)]
    assert _both([0, 3], rows, STEP, 1, 0) == [(0, 1, 0, 0, 0, 1, 100), (0, 1, 0, 2, 2, 1, 100)]
    assert _both([0, 3], [MISS] * 3, STEP, 0, 1) == []


def test_recordings_do_not_share_a_segment_and_an_empty_one_lies_between():
    # recording 0 ends inside a segment, recording 1 has no window, recording 2 goes on with the same identity from ITS
    # window 0: three recordings, two segments, window numbers local to the recording
    rows = [_hit(3, 10, 0), _hit(3, 10, 1)] + [_hit(3, 10, 0), _hit(3, 10, 1), _hit(3, 10, 2)]
    assert _both([0, 2, 2, 5], rows, STEP, 1, 1) == [(0, 3, 10, 0, 1, 2, 100), (2, 3, 10, 0, 2, 3, 100)]
    assert _both([0, 0, 0], [], STEP, 1, 1) == []
    assert _both([0], [], STEP, 1, 1) == []


def test_negative_and_large_shifts_in_64_bits():
    big = 2 ** 31 - 1
    rows = [(1, -2 ** 31, 10, 1), (1, -2 ** 31 + STEP, 10, 1), (2, big, 10, 1), (2, big, 10, 1)]
    want = _both([0, 4], rows, STEP, 1, 0)
    assert want == [(0, 1, -2 ** 31, 0, 1, 2, 10), (0, 2, big - 2 * STEP, 2, 2, 1, 10), (0, 2, big - 3 * STEP, 3, 3, 1, 10)]
    # a step so large that w * step leaves 32 bits
    step = 2 ** 31
    rows = [(1, 5, 10, 1), (1, 5, 10, 1), (1, 5, 10, 1)]
    assert _both([0, 3], rows, step, 1, 0) == [(0, 1, 5, 0, 0, 1, 10), (0, 1, 5 - 2 ** 31, 1, 1, 1, 10), (0, 1, 5 - 2 ** 32, 2, 2, 1, 10)]


@pytest.mark.parametrize("topn", [2, 3, 10])
def test_only_rank_zero_is_read_at_any_stride(topn):
    rows = [_hit(2, -43, w, aligned=60 + w) for w in range(5)]
    assert _both([0, 5], rows, STEP, 50, 1, topn=topn) == [(0, 2, -43, 0, 4, 5, 64)]


def test_the_capacity_two_call():
    rows = [_hit(1 + (w // 2), 0, w) for w in range(10)]      # five segments of two windows
    sid, delta, aligned, nres = _cols(rows)
    args = ([0, 10], sid, delta, aligned, nres, STEP, 1, 0)
    want = timeline_twin(*args)
    assert len(want) == 5
    rc, _, n = _ffi.scan_timeline_raw(*args, cap=0)
    assert (rc, n) == (_ffi.E_CAPACITY, 5)
    rc, seg, n = _ffi.scan_timeline_raw(*args, cap=3)          # too little room: the count, and the first three written
    assert (rc, n) == (_ffi.E_CAPACITY, 5)
    assert [tuple(int(seg[k][i]) for k, _ in _ffi.SEGMENT_FIELDS) for i in range(3)] == want[:3]
    for cap in (5, 8):
        rc, seg, n = _ffi.scan_timeline_raw(*args, cap=cap)
        assert (rc, n) == (_ffi.OK, 5)
        assert [tuple(int(seg[k][i]) for k, _ in _ffi.SEGMENT_FIELDS) for i in range(5)] == want
        assert not any(seg[k][5:].any() for k, _ in _ffi.SEGMENT_FIELDS), "nothing is written behind the segments"
    rc, _, n = _ffi.scan_timeline_raw([0, 0], sid[:0], delta[:0], aligned[:0], nres[:0], STEP, 1, 0, cap=0)
    assert (rc, n) == (_ffi.OK, 0)


def test_bad_arguments():
    sid, delta, aligned, nres = _cols([_hit(1, 0, 0)])
    L = _ffi.lib()
    import ctypes as C
    cnt = C.c_uint64()
    wo = np.array([0, 1], np.uint64)
    none7 = [None] * 7
    # topn 0, no count, a win_off that decreases
    assert L.shz_scan_timeline(wo.ctypes.data_as(_ffi.u64p), 1, _ffi.ptr(sid), _ffi.ptr(delta), _ffi.ptr(aligned), _ffi.ptr(nres),
                               0, 1, 1, 1, *none7, 0, C.byref(cnt)) == _ffi.E_INVALID
    assert L.shz_scan_timeline(wo.ctypes.data_as(_ffi.u64p), 1, _ffi.ptr(sid), _ffi.ptr(delta), _ffi.ptr(aligned), _ffi.ptr(nres),
                               1, 1, 1, 1, *none7, 0, None) == _ffi.E_INVALID
    bad = np.array([1, 0], np.uint64)
    assert L.shz_scan_timeline(bad.ctypes.data_as(_ffi.u64p), 1, _ffi.ptr(sid), _ffi.ptr(delta), _ffi.ptr(aligned), _ffi.ptr(nres),
                               1, 1, 1, 1, *none7, 0, C.byref(cnt)) == _ffi.E_INVALID
    # room announced but no arrays
    assert L.shz_scan_timeline(wo.ctypes.data_as(_ffi.u64p), 1, _ffi.ptr(sid), _ffi.ptr(delta), _ffi.ptr(aligned), _ffi.ptr(nres),
                               1, 1, 1, 1, *none7, 4, C.byref(cnt)) == _ffi.E_INVALID


# ---- random sequences -------------------------------------------------------------------------------------------------
def test_random_sequences_equal_the_twin():
    rng = np.random.default_rng(20261017)
    n_segments = 0
    for case in range(400):
        n_recs = int(rng.integers(1, 5))
        topn = int(rng.integers(1, 4))
        step = int(rng.integers(1, 40))
        max_gap = int(rng.integers(0, 4))
        min_aligned = int(rng.integers(0, 60))
        counts = [int(rng.integers(0, 40)) if rng.random() > 0.15 else 0 for _ in range(n_recs)]
        win_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        rows = []
        for n in counts:
            # a few songs play in turn, each at one shift; windows drop out, fall under the threshold, or name another song
            w = 0
            while w < n:
                song, shift = int(rng.integers(1, 4)), int(rng.integers(-300, 300))
                for _ in range(int(rng.integers(1, 12))):
                    if w >= n:
                        break
                    u = rng.random()
                    if u < 0.15:
                        rows.append((song, shift + w * step, int(rng.integers(0, 200)), 0))
                    elif u < 0.25:
                        rows.append((int(rng.integers(1, 4)), int(rng.integers(-300, 300)), int(rng.integers(0, 120)), 1))
                    else:
                        rows.append((song, shift + w * step, int(rng.integers(30, 120)), int(rng.integers(1, topn + 1))))
                    w += 1
        n_segments += len(_both(win_off, rows, step, min_aligned, max_gap, topn=topn))
    assert n_segments > 1000, "the cases must produce segments to compare"
