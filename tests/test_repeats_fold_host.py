"""CPU: shz_repeats_fold (host only, no GPU, no ctx) against the plain-Python fold of tests/repeat_twin.py -- built cell lists at
every edge of the linking rule, of the order and of min_pairs, random lists whose components merge often, the capacity idiom
and the refusals."""
import numpy as np

import repeat_twin as twin
from shazam_amd import _ffi

FILL = 0x5A5A5A5A


def _cells(rows):
    """rows: per recording a list of (lag, block, pairs, first, last), any order -> cell_off and the five columns, sorted"""
    off, cols = [0], [[] for _ in range(5)]
    for rec in rows:
        for c in sorted(rec):
            for k in range(5):
                cols[k].append(c[k])
        off.append(len(cols[0]))
    return off, cols


def _cell(lag, block, pairs=10, shift=5, lo=0, hi=None):
    hi = (1 << shift) - 1 if hi is None else hi
    return (lag, block, pairs, (block << shift) + lo, (block << shift) + hi)


def _check(rows, lag_tol=1, max_gap=1, min_pairs=1):
    off, cols = _cells(rows)
    want = twin.fold(off, *cols, lag_tol, max_gap, min_pairs)
    got = _ffi.repeats_fold(off, *cols, lag_tol, max_gap, min_pairs)
    assert len(got["rec"]) == len(want)
    for k, _ in _ffi.REPEAT_FIELDS:
        assert [int(x) for x in got[k]] == [w[k] for w in want], k
    return want


def test_lag_distance_at_and_beyond_the_tolerance():
    for tol in (0, 1, 3):
        assert len(_check([[_cell(100, 4), _cell(100 + tol, 5)]], lag_tol=tol)) == 1
        assert len(_check([[_cell(100, 4), _cell(100 + tol + 1, 5)]], lag_tol=tol)) == 2
        assert len(_check([[_cell(100 + tol, 4), _cell(100, 5)]], lag_tol=tol)) == 1
        assert len(_check([[_cell(100 + tol + 1, 4), _cell(100, 5)]], lag_tol=tol)) == 2


def test_block_distance_at_and_beyond_the_gap():
    for gap in (0, 1, 4):
        assert len(_check([[_cell(100, 4), _cell(100, 4 + gap + 1)]], max_gap=gap)) == 1
        assert len(_check([[_cell(100, 4), _cell(100, 4 + gap + 2)]], max_gap=gap)) == 2
        # the same across two lags, in either direction
        assert len(_check([[_cell(100, 9), _cell(101, 9 - gap - 1)]], max_gap=gap)) == 1
        assert len(_check([[_cell(100, 9), _cell(101, 9 - gap - 2)]], max_gap=gap)) == 2
        assert len(_check([[_cell(100, 9 - gap - 1), _cell(101, 9)]], max_gap=gap)) == 1
        assert len(_check([[_cell(100, 9 - gap - 2), _cell(101, 9)]], max_gap=gap)) == 2


def test_chains_link_cells_that_are_not_neighbours_themselves():
    # a chain along the blocks and along the lags: one component although its ends are far apart
    want = _check([[_cell(50, b) for b in range(0, 20, 2)] + [_cell(50 + d, 18) for d in range(1, 6)]])
    assert len(want) == 1 and want[0]["cells"] == 15 and (want[0]["lag_lo"], want[0]["lag_hi"]) == (50, 55)
    # two chains joined only by their last cells (the union arrives late)
    assert len(_check([[_cell(10, b) for b in range(8)] + [_cell(13, b) for b in range(8)] + [_cell(11, 9), _cell(12, 9)]])) == 1
    assert len(_check([[_cell(10, b) for b in range(8)] + [_cell(13, b) for b in range(8)] + [_cell(11, 9)]])) == 2


def test_order_staircase_shares_first_with_a_single_cell():
    # a staircase whose first cell (by index) is not the one with the smallest `first`, and a one-cell component with the same
    # `first` on another lag: (rec, first, lag, smallest cell index) decides
    stairs = [_cell(200, 3), _cell(201, 2), _cell(202, 1, lo=4)]
    single = [_cell(90, 1, lo=4)]
    want = _check([stairs + single], lag_tol=1, max_gap=0)
    assert [w["cells"] for w in want] == [1, 3] and want[0]["first"] == want[1]["first"] == 36
    single = [_cell(300, 1, lo=4)]
    want = _check([stairs + single], lag_tol=1, max_gap=0)
    assert [w["cells"] for w in want] == [3, 1]
    # the same first AND the same lag: the smallest cell index decides
    want = _check([[_cell(40, 1, lo=2), _cell(40, 1 + 3, lo=0), _cell(41, 1 + 6, lo=0), _cell(40, 1 + 9)],
                   ], lag_tol=0, max_gap=0)
    assert len(want) == 4
    want = _check([[(40, 1, 5, 34, 40), (40, 4, 5, 34, 130), (39, 9, 5, 34, 300)]], lag_tol=0, max_gap=0)
    assert [w["lag"] for w in want] == [39, 40, 40] and [w["last"] for w in want] == [300, 40, 130]


def test_min_pairs_met_exactly_and_missed_by_one():
    rows = [[_cell(70, 1, pairs=40), _cell(70, 2, pairs=35), _cell(71, 2, pairs=25), _cell(500, 1, pairs=99)]]
    assert [w["pairs"] for w in _check(rows, min_pairs=100)] == [100]
    assert [w["pairs"] for w in _check(rows, min_pairs=101)] == []
    assert [w["pairs"] for w in _check(rows, min_pairs=99)] == [100, 99]
    assert len(_check(rows, min_pairs=0)) == 2


def test_lag_tie_inside_a_component_takes_the_smaller_lag():
    want = _check([[_cell(81, 1, pairs=30), _cell(80, 1, pairs=10), _cell(80, 2, pairs=20), _cell(82, 2, pairs=29)]])
    assert want[0]["lag"] == 80 and want[0]["pairs"] == 89
    want = _check([[_cell(81, 1, pairs=31), _cell(80, 1, pairs=10), _cell(80, 2, pairs=20), _cell(82, 2, pairs=29)]])
    assert want[0]["lag"] == 81
    want = _check([[_cell(80, 1, pairs=0), _cell(81, 1, pairs=0)]], min_pairs=0)       # nothing but ties at 0
    assert want[0]["lag"] == 80


def test_two_recordings_with_identical_cells_stay_apart():
    rec = [_cell(120, b, pairs=60) for b in (2, 3, 4)] + [_cell(400, 9, pairs=100)]
    want = _check([rec, [], rec], min_pairs=100)
    assert [w["rec"] for w in want] == [0, 0, 2, 2]
    assert [w["pairs"] for w in want] == [180, 100, 180, 100]


def test_no_recordings_no_cells():
    assert _check([]) == []
    assert _check([[], []]) == []


def test_random_lists_whose_components_merge_often():
    rng = np.random.default_rng(20261020)
    for case in range(200):
        rows = []
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(0, 301 if case % 4 == 0 else 60))
            seen = {(int(rng.integers(0, 12)), int(rng.integers(0, 20))) for _ in range(n)}
            rec = []
            for lag, block in seen:
                lo, hi = sorted(int(x) for x in rng.integers(0, 32, 2))
                rec.append((lag, block, int(rng.integers(0, 50)), (block << 5) + lo, (block << 5) + hi))
            rows.append(rec)
        _check(rows, lag_tol=int(rng.integers(0, 3)), max_gap=int(rng.integers(0, 3)), min_pairs=int(rng.integers(0, 120)))


def test_wide_tolerances_do_not_walk_empty_rows():
    # lag_tol and max_gap at the top of their range: the neighbour search hops over rows that hold no cell
    rows = [[_cell(5, 0), _cell(1000000, 3), _cell(0xFFFFFFFF, 0x7FFFFFF, shift=5)]]
    assert len(_check(rows, lag_tol=0xFFFFFFFF, max_gap=0xFFFFFFFF)) == 1
    assert len(_check(rows, lag_tol=999995, max_gap=2)) == 2


def test_capacity_idiom():
    rows = [[_cell(10 * k, 3 * k, pairs=10 + k) for k in range(1, 7)]]
    off, cols = _cells(rows)
    want = twin.fold(off, *cols, 1, 1, 1)
    assert len(want) == 6
    rc, _, n = _ffi.repeats_fold_raw(off, *cols, 1, 1, 1, cap=0)
    assert (rc, n) == (_ffi.E_CAPACITY, 6)
    rc, rep, n = _ffi.repeats_fold_raw(off, *cols, 1, 1, 1, cap=5, fill=FILL)
    assert (rc, n) == (_ffi.E_CAPACITY, 6)
    for k, _ in _ffi.REPEAT_FIELDS:
        assert [int(x) for x in rep[k]] == [w[k] for w in want[:5]]
    rc, rep, n = _ffi.repeats_fold_raw(off, *cols, 1, 1, 1, cap=6)
    assert (rc, n) == (_ffi.OK, 6)
    rc, rep, n = _ffi.repeats_fold_raw(off, *cols, 1, 1, 1, cap=9, fill=FILL)
    assert (rc, n) == (_ffi.OK, 6) and all(int(x) == FILL for x in rep["lag"][6:])


def test_refusals_write_nothing():
    import ctypes as C
    off, cols = _cells([[_cell(10, 1), _cell(10, 2), _cell(11, 0)]])

    def raw(off=off, cols=cols, cap=4):
        rc, rep, n = _ffi.repeats_fold_raw(off, *cols, 1, 1, 1, cap=cap, fill=FILL)
        assert n == FILL and all(int(x) == FILL for k, _ in _ffi.REPEAT_FIELDS for x in rep[k])
        return rc
    swapped = [list(c) for c in cols]
    for c in swapped:
        c[0], c[1] = c[1], c[0]
    assert raw(cols=swapped) == _ffi.E_INVALID                                   # blocks of one lag out of order
    twice = [[c[0], c[0], c[2]] for c in cols]
    assert raw(cols=twice) == _ffi.E_INVALID                                     # the same (lag, block) twice
    lag_down = [list(c) for c in cols]
    lag_down[0] = [10, 12, 11]
    assert raw(cols=lag_down) == _ffi.E_INVALID                                  # lags out of order
    inverted = [list(c) for c in cols]
    inverted[3][1], inverted[4][1] = inverted[4][1], inverted[3][1]
    assert raw(cols=inverted) == _ffi.E_INVALID                                  # first > last
    assert raw(off=[1, 3]) == _ffi.E_INVALID                                     # cell_off does not start at 0
    assert raw(off=[0, 3, 2]) == _ffi.E_INVALID                                  # cell_off decreases
    # the order restarts with every recording: the same list cut in two is fine
    rc, _, n = _ffi.repeats_fold_raw([0, 2, 3], *cols, 1, 1, 1, cap=4)
    assert (rc, n) == (_ffi.OK, 2)
    # NULL arrays
    L = _ffi.lib()
    co = np.asarray(off, np.uint64)
    a = [np.asarray(c, np.uint32) for c in cols]
    cnt = C.c_uint64(FILL)
    none8 = [None] * 8
    assert L.shz_repeats_fold(_ffi.ptr(co), 1, *[_ffi.ptr(x) for x in a], 1, 1, 1, *none8, 0, None) == _ffi.E_INVALID
    assert L.shz_repeats_fold(None, 1, *[_ffi.ptr(x) for x in a], 1, 1, 1, *none8, 0, C.byref(cnt)) == _ffi.E_INVALID
    assert L.shz_repeats_fold(_ffi.ptr(co), 1, None, *[_ffi.ptr(x) for x in a[1:]], 1, 1, 1, *none8, 0, C.byref(cnt)) == _ffi.E_INVALID
    assert L.shz_repeats_fold(_ffi.ptr(co), 1, *[_ffi.ptr(x) for x in a], 1, 1, 1, *none8, 3, C.byref(cnt)) == _ffi.E_INVALID
    assert cnt.value == FILL
    # (without room the rep_* pointers may be NULL)
    assert L.shz_repeats_fold(_ffi.ptr(co), 1, *[_ffi.ptr(x) for x in a], 1, 1, 1, *none8, 0, C.byref(cnt)) == _ffi.E_CAPACITY
    assert cnt.value == 1
