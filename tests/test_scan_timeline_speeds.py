"""CPU: shz_scan_timeline_speeds (host only, no GPU) against its plain-Python twin (tests/scan_speed_twin.py) on hand-built
arrays: the two delta series measured for the pitched recording of the GPU test fold into two segments although the rung
flips between neighbours; a rung jump, a shift jump, a gap and a song change each split a segment; the most-chosen-rung
tie rule; counting with cap = 0 and SHZ_E_CAPACITY with the first cap segments written."""
import numpy as np
import pytest

import scan_speed_twin as ST
from shazam_amd import _ffi

LADDER = np.asarray([63512, 63604, 63696, 65444, 65536, 65628, 67376, 67468, 67560], np.uint32)
STEP = 22
# measured on the CPU oracle + twin: the song frame at every window's start, windows 0-9 at 1.03 and 10-19 at 0.97
FAST = [-23, 0, 22, 45, 68, 90, 113, 136, 158, 181]
SLOW = [-58, -36, -15, 6, 27, 49, 70, 91, 112, 134]
FIELDS = [k for k, _ in _ffi.SPEED_SEGMENT_FIELDS]


def _arrays(rows, topn=2):
    """rows: per window (sid, delta, aligned, best) or None for a window without a result."""
    n = len(rows)
    sid, delta = np.zeros((n, topn), np.uint32), np.zeros((n, topn), np.int32)
    aligned, nres, best = np.zeros((n, topn), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for w, row in enumerate(rows):
        if row is not None:
            sid[w, 0], delta[w, 0], aligned[w, 0], best[w] = row
            nres[w] = 1
            sid[w, 1:], aligned[w, 1:] = 99, 1      # rank 1 is never read
    return sid, delta, aligned, nres, best


def _both(win_off, rows, min_aligned=40, ladder=LADDER, **kw):
    sid, delta, aligned, nres, best = _arrays(rows)
    seg = _ffi.scan_timeline_speeds(win_off, sid, delta, aligned, nres, best, STEP, ladder, min_aligned, **kw)
    want = ST.timeline(win_off, sid, delta, aligned, nres, best, STEP, ladder.tolist(), min_aligned, **kw)
    got = [{k: int(seg[k][i]) for k in FIELDS} for i in range(len(seg["rec"]))]
    assert got == want, (got, want)
    return got


def _measured_rows():
    rows = [(2, d, 60 + 5 * i, 7) for i, d in enumerate(FAST)]
    rows += [(4, d, 54 + 3 * i, i % 2) for i, d in enumerate(SLOW)]      # the rung flips between 63512 and 63604
    return rows


def test_measured_series_give_two_segments():
    segs = _both([0, 20], _measured_rows())
    assert len(segs) == 2
    a, b = segs
    assert (a["sid"], a["first"], a["last"], a["hits"], a["pos_first"], a["pos_last"], a["rung"]) == (2, 0, 9, 10, -23, 181, 7)
    assert (b["sid"], b["first"], b["last"], b["hits"], b["pos_first"], b["pos_last"]) == (4, 10, 19, 10, -58, 134)
    assert a["best"] == 105 and b["best"] == 81
    assert b["rung"] == 1, "five hits each at rungs 0 and 1: the tie goes to the factor nearer 65536"
    # the plain timeline's constant shift does not exist here: it would cut the same windows into many segments
    sid, delta, aligned, nres, _ = _arrays(_measured_rows())
    plain = _ffi.scan_timeline([0, 20], sid, delta, aligned, nres, STEP, 40)
    assert len(plain["rec"]) > 2
    # below the threshold nothing is a hit
    assert _both([0, 20], _measured_rows(), min_aligned=1000) == []


def test_rung_jump_splits():
    rows = _measured_rows()[:10]
    rows[5] = (2, FAST[5], 80, 4)                  # 3 rungs below its neighbours
    segs = _both([0, 10], rows)
    assert [(s["first"], s["last"]) for s in segs] == [(0, 4), (5, 5), (6, 9)]
    assert len(_both([0, 10], rows, rung_tol=3)) == 1


def test_shift_jump_splits():
    rows = _measured_rows()[:10]
    for w in range(6, 10):
        rows[w] = (2, FAST[w] + 3, 80, 7)          # the song skips 3 frames between windows 5 and 6: beyond shift_tol = 2
    segs = _both([0, 10], rows)
    assert [(s["first"], s["last"]) for s in segs] == [(0, 5), (6, 9)]
    assert len(_both([0, 10], rows, shift_tol=4)) == 1
    rows = _measured_rows()[:10]
    for w in range(6, 10):
        rows[w] = (2, FAST[w] - 1, 80, 7)          # one frame back: within the rounding the tolerance is for
    assert len(_both([0, 10], rows)) == 1


def test_gap_splits():
    rows = _measured_rows()[:10]
    rows[4] = None                                   # no result
    rows[5] = (2, FAST[5], 10, 7)                    # below min_aligned
    segs = _both([0, 10], rows)
    assert [(s["first"], s["last"], s["hits"]) for s in segs] == [(0, 3, 4), (6, 9, 4)]
    one = _both([0, 10], rows, max_gap=2)            # the advance is judged over the three steps between windows 3 and 6
    assert [(s["first"], s["last"], s["hits"]) for s in one] == [(0, 9, 8)]
    assert len(_both([0, 10], rows, max_gap=0)) == 2


def test_sid_change_and_recording_border_split():
    rows = _measured_rows()[:10]
    rows[3] = (3, FAST[3], 80, 7)
    segs = _both([0, 10], rows)
    assert [(s["sid"], s["first"], s["last"]) for s in segs] == [(2, 0, 2), (3, 3, 3), (2, 4, 9)]
    # the same windows as two recordings: a segment never crosses the border, window numbers restart
    segs = _both([0, 4, 4, 10], _measured_rows()[:4] + _measured_rows()[:6])
    assert [(s["rec"], s["first"], s["last"]) for s in segs] == [(0, 0, 3), (2, 0, 5)]


def test_most_chosen_rung_and_its_ties():
    def seg_of(rungs, ladder=LADDER):
        rows = [(2, d, 80, v) for d, v in zip(FAST, rungs)]
        (s,) = _both([0, len(rows)], rows, ladder=ladder, rung_tol=8)
        return s["rung"]
    assert seg_of([7, 7, 6, 6, 6, 8]) == 6                        # the most often
    assert seg_of([7, 6, 7, 6]) == 6                              # 2 : 2 -> 67376 is nearer 65536 than 67468
    assert seg_of([3, 5, 3, 5]) == 3                              # 65444 and 65628 are equally near: the lower index
    assert seg_of([0, 1], np.asarray([65628, 65444, 65536], np.uint32)) == 0


def test_cap_zero_counts_and_cap_below_count_writes_the_first():
    rows = _measured_rows()
    rows[3] = (3, FAST[3], 80, 7)                                 # segments: 0-2, 3, 4-9, 10-19
    sid, delta, aligned, nres, best = _arrays(rows)
    args = ([0, 20], sid, delta, aligned, nres, best, STEP, LADDER, 40, 1, 1, 2)
    rc, _, n = _ffi.scan_timeline_speeds_raw(*args, 0)
    assert rc == _ffi.E_CAPACITY and n == 4
    rc, full, n = _ffi.scan_timeline_speeds_raw(*args, 4)
    assert rc == _ffi.OK and n == 4
    rc, part, n = _ffi.scan_timeline_speeds_raw(*args, 2)
    assert rc == _ffi.E_CAPACITY and n == 4
    for k in FIELDS:
        assert np.array_equal(part[k], full[k][:2]), k
    # no hit: no segment, OK with no room
    rc, _, n = _ffi.scan_timeline_speeds_raw([0, 20], sid, delta, aligned, nres, best, STEP, LADDER, 10 ** 6, 1, 1, 2, 0)
    assert rc == _ffi.OK and n == 0


def test_bad_arguments():
    sid, delta, aligned, nres, best = _arrays(_measured_rows())
    for ladder in (np.asarray([1], np.uint32), np.asarray([65536, 200000], np.uint32), LADDER[:7]):   # out of range; best >= K
        with pytest.raises(_ffi.ShzError) as e:
            _ffi.scan_timeline_speeds([0, 20], sid, delta, aligned, nres, best, STEP, ladder, 40)
        assert e.value.code == _ffi.E_INVALID
