"""CPU: the host half of content shared between recordings (shazam_amd/shared.py) -- shared_occurrences
against the plain-Python definition in tests/shared_twin.py on built lists, the enumeration and the cutting of the job list,
the signed lag window, and shz_repeats_fold on lags biased by 2^20 against repeat_twin.fold on the same arrays."""
import numpy as np
import pytest

import repeat_twin
import shared_twin as twin
from shazam_amd import _ffi, shared

BIAS = 1 << 20


def _s(rec_a, rec_b, first, last, lag):
    return dict(rec_a=rec_a, rec_b=rec_b, first=first, last=last, lag=lag)


def _r(rec, first, last, lag):
    return dict(rec=rec, first=first, last=last, lag=lag)


def _occ(sh, rp=()):
    got = shared.shared_occurrences(sh, rp)
    assert [(g["airings"], g["shared"], g["repeats"]) for g in got] == twin.occurrences(sh, rp)
    return got


def test_overlap_of_exactly_half_the_shorter_interval_and_one_frame_less():
    # in recording 1 the stretches land at [100, 119] and at [110, 149]: 10 of the shorter one's 20 frames overlap -- one airing
    got = _occ([_s(0, 1, 0, 19, 100), _s(2, 1, 500, 539, -390)])
    assert len(got) == 1 and got[0]["airings"] == [(0, 0, 19), (1, 100, 149), (2, 500, 539)] and got[0]["shared"] == [0, 1]
    # ... at [111, 150]: 9 frames -- two airings, two groups
    got = _occ([_s(0, 1, 0, 19, 100), _s(2, 1, 500, 539, -389)])
    assert [g["airings"] for g in got] == [[(0, 0, 19), (1, 100, 119)], [(1, 111, 150), (2, 500, 539)]]
    assert [g["shared"] for g in got] == [[0], [1]]
    # the same two cases with an odd shorter length (21 frames: 11 overlap, then 10)
    assert len(_occ([_s(0, 1, 0, 20, 100), _s(2, 1, 500, 539, -390)])) == 1
    assert len(_occ([_s(0, 1, 0, 20, 100), _s(2, 1, 500, 539, -389)])) == 2


def test_intervals_of_different_recordings_never_merge():
    # the same frames in four recordings: four airings in two groups
    got = _occ([_s(0, 1, 10, 50, 0), _s(2, 3, 10, 50, 0)])
    assert [g["airings"] for g in got] == [[(0, 10, 50), (1, 10, 50)], [(2, 10, 50), (3, 10, 50)]]
    # a repeat of recording 1 over the frames of a stretch between 0 and 2 joins nothing
    got = _occ([_s(0, 2, 10, 50, 5)], [_r(1, 10, 50, 100)])
    assert len(got) == 2 and got[0]["repeats"] == [] and got[1]["shared"] == [] and got[1]["repeats"] == [0]


def test_chains_through_repeats():
    # the advert airs twice in recording 0 (a repeat) and once in recording 1, which shares it with the SECOND airing only; a
    # second repeat chains a third airing of recording 0 on: one group of four airings
    sh = [_s(0, 1, 300, 340, -250)]
    rp = [_r(0, 100, 140, 200), _r(0, 302, 338, 400)]
    got = _occ(sh, rp)
    assert len(got) == 1
    assert got[0]["airings"] == [(0, 100, 140), (0, 300, 340), (0, 702, 738), (1, 50, 90)]
    assert got[0]["shared"] == [0] and got[0]["repeats"] == [0, 1]
    # without the first repeat its first airing is gone, with neither only the stretch is left
    assert [len(g["airings"]) for g in _occ(sh, rp[1:])] == [3]
    assert [len(g["airings"]) for g in _occ(sh)] == [2]
    # a negative frame (first + lag below 0) is an integer like any other
    assert _occ([_s(0, 1, 0, 30, -2)])[0]["airings"] == [(0, 0, 30), (1, -2, 28)]
    # order: by first airing
    got = _occ([_s(2, 3, 5, 9, 0), _s(0, 1, 50, 90, 0), _s(0, 3, 7, 20, 100)])
    assert [g["airings"][0] for g in got] == [(0, 7, 20), (0, 50, 90), (2, 5, 9)]


def test_fuzz_against_the_twin():
    rng = np.random.default_rng(5)
    for _ in range(60):
        sh = [_s(*(int(x) for x in rng.permutation(4)[:2]), first, first + int(rng.integers(0, 40)), int(rng.integers(-60, 60)))
              for first in rng.integers(60, 200, int(rng.integers(0, 7)))]
        rp = [_r(int(rng.integers(0, 4)), first, first + int(rng.integers(0, 40)), int(rng.integers(1, 80)))
              for first in rng.integers(0, 200, int(rng.integers(0, 5)))]
        sh = [dict(p, first=int(p["first"]), last=int(p["last"])) for p in sh]
        rp = [dict(p, first=int(p["first"]), last=int(p["last"])) for p in rp]
        _occ(sh, rp)


def test_empty_input():
    assert shared.shared_occurrences([]) == [] and shared.shared_occurrences([], []) == [] and twin.occurrences([], []) == []


def test_pairs_none_is_every_a_below_b_and_bad_pairs_are_refused():
    assert shared._check_pairs(None, 4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert shared._check_pairs(None, 1) == [] and shared._check_pairs(None, 0) == []
    assert shared._check_pairs([(3, 0), (0, 3), (0, 3)], 4) == [(3, 0), (0, 3), (0, 3)]
    for bad in ([(1, 1)], [(0, 4)], [(-1, 2)]):
        with pytest.raises(ValueError, match="two different recordings"):
            shared._check_pairs(bad, 4)


def test_the_job_list_is_cut_by_jobs_and_by_named_recordings(monkeypatch):
    pairs = [(0, 1), (0, 2), (3, 0), (4, 5), (5, 4)]
    assert shared._plan_calls(pairs) == [(0, pairs, [0, 1, 2, 3, 4, 5])]
    assert shared._plan_calls([]) == []
    monkeypatch.setattr(shared, "MAX_JOBS", 2)
    assert shared._plan_calls(pairs) == [(0, pairs[:2], [0, 1, 2]), (2, pairs[2:4], [0, 3, 4, 5]), (4, pairs[4:], [4, 5])]
    monkeypatch.setattr(shared, "MAX_JOBS", 4096)
    monkeypatch.setattr(shared, "MAX_RECS", 3)
    assert shared._plan_calls(pairs) == [(0, pairs[:2], [0, 1, 2]), (2, pairs[2:3], [0, 3]), (3, pairs[3:], [4, 5])]


def test_signed_seconds_to_frames():
    sr, hop, most = 44100, 2048, (1 << 20) - 1
    assert shared._lag_window(None, None, sr, hop) == (-most, most)
    assert shared._lag_window(-1, 1, sr, hop) == (-22, 22)                     # round(21.53)
    assert shared._lag_window(0, 0, sr, hop) == (0, 0)
    assert shared._lag_window(-12, -3, sr, hop) == (-258, -65)
    assert shared._lag_window(3, None, sr, hop) == (65, most)
    assert shared._lag_window(None, -3, sr, hop) == (-most, -65)
    assert shared._lag_window(-1e9, 1e9, sr, hop) == (-most, most)             # beyond what the library holds: cut
    assert shared._lag_window(-1, 1, 48000, 1024) == (-47, 47)
    with pytest.raises(ValueError, match="below min_lag_seconds"):
        shared._lag_window(2, 1, sr, hop)
    with pytest.raises(ValueError, match="below min_lag_seconds"):
        shared._lag_window(-1, -2, sr, hop)


def test_the_fold_on_biased_lags_equals_the_twins():
    """shz_repeats_fold never looks at a lag but to compare it and to subtract lag_tol: cells whose signed lags straddle 0,
    biased by 2^20, fold as repeat_twin.fold folds the same arrays -- jobs in the place of recordings"""
    rng = np.random.default_rng(11)
    for case in range(30):
        off, lag, block, pairs, first, last = [0], [], [], [], [], []
        for _ in range(int(rng.integers(1, 4))):
            cells = sorted({(int(rng.integers(-4, 5)) if case % 2 else int(rng.integers(-BIAS + 1, BIAS)), int(rng.integers(0, 12)))
                            for _ in range(int(rng.integers(0, 25)))})
            if case == 0:
                cells = sorted(set(cells) | {(-BIAS + 1, 0), (-BIAS + 2, 1), (BIAS - 1, 3), (BIAS - 2, 3), (0, 0), (-1, 0)})
            for g, b in cells:
                lag.append(g + BIAS)
                block.append(b)
                pairs.append(int(rng.integers(1, 60)))
                first.append(32 * b + int(rng.integers(0, 16)))
                last.append(first[-1] + int(rng.integers(0, 16)))
            off.append(len(lag))
        for lag_tol, max_gap, min_pairs in ((1, 1, 1), (0, 0, 30), (2, 3, 100)):
            got = _ffi.repeats_fold(off, lag, block, pairs, first, last, lag_tol, max_gap, min_pairs)
            want = repeat_twin.fold(off, lag, block, pairs, first, last, lag_tol, max_gap, min_pairs)
            for key, _ in _ffi.REPEAT_FIELDS:
                assert [int(x) for x in got[key]] == [w[key] for w in want], (case, key)
