"""CPU: shz_scan_timeline_warps (host only, no GPU, no ctx) against the plain-Python twin (tests/scan_warp_twin.py): seeded
random window sequences with gaps, id changes and unsorted warp lists, the two factor tolerances and the shift tolerance at
exactly tol and tol + 1, SHZ_SCAN_NO_WARP on windows that are no hit, the two-call capacity idiom, and on a uniform sorted
diagonal ladder the speed timeline with rung_tol = 1."""
import numpy as np
import pytest

import scan_speed_twin as ST
import scan_warp_twin as SW
from shazam_amd import _ffi

FIELDS = [k for k, _ in _ffi.WARP_SEGMENT_FIELDS]


def _segs(seg):
    return [{k: int(seg[k][i]) for k in FIELDS} for i in range(len(seg["rec"]))]


def _both(win_off, sid, delta, aligned, nres, best, step, t16, f16, min_aligned, **kw):
    got = _ffi.scan_timeline_warps(win_off, sid, delta, aligned, nres, best, step, t16, f16, min_aligned, **kw)
    want = SW.timeline(win_off, sid, delta, aligned, nres, best, step, t16, f16, min_aligned, **kw)
    assert _segs(got) == want
    return want


def _walk(rng, n, t16, f16, step, topn, min_aligned):
    """A window sequence that mostly continues: the song position advances by the warped step, with small disturbances."""
    K = len(t16)
    sid, delta = np.zeros((n, topn), np.uint32), np.zeros((n, topn), np.int32)
    aligned, nres = np.zeros((n, topn), np.uint32), np.zeros(n, np.uint32)
    best = np.zeros(n, np.uint32)
    s, v, pos = 1, int(rng.integers(K)), int(rng.integers(-50, 500))
    for w in range(n):
        if rng.random() < 0.1:
            s = int(rng.integers(1, 4))
        if rng.random() < 0.3:
            v = int(rng.integers(K))
        pos += SW.W(step, int(t16[v])) + int(rng.choice([0, 0, 0, 1, -1, 2, -2, 3, -3, 40]))
        hit = rng.random() < 0.75
        nres[w] = int(rng.integers(1, topn + 1)) if rng.random() < 0.9 else 0
        sid[w], delta[w] = rng.integers(1, 4, topn), rng.integers(-100, 100, topn)
        aligned[w] = rng.integers(0, min_aligned, topn)
        sid[w, 0], delta[w, 0] = s, pos
        aligned[w, 0] = int(rng.integers(min_aligned, 3 * min_aligned)) if hit else int(rng.integers(0, min_aligned))
        is_hit = nres[w] >= 1 and aligned[w, 0] >= min_aligned
        best[w] = v if is_hit or rng.random() < 0.5 else SW.NO_WARP      # read for hits only
    return sid, delta, aligned, nres, best


@pytest.mark.parametrize("seed", range(8))
def test_random_sequences_equal_the_twin(seed):
    rng = np.random.default_rng([0x5CA9, seed])
    K, topn, step = int(rng.integers(1, 12)), int(rng.integers(1, 4)), int(rng.integers(1, 30))
    t16 = rng.choice([62783, 65536, 68289, 32768, 131072], K).astype(np.uint32)          # unsorted, repeats allowed
    f16 = rng.choice([65457, 65536, 65615, 65694, 32768, 131072], K).astype(np.uint32)
    counts = rng.integers(0, 40, int(rng.integers(1, 5)))
    win_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    cols = _walk(rng, int(win_off[-1]), t16, f16, step, topn, 20)
    total = 0
    for kw in (dict(max_gap=0, tempo_tol=0, pitch_tol=0, shift_tol=0), dict(max_gap=1, tempo_tol=2753, pitch_tol=79, shift_tol=2),
               dict(max_gap=3, tempo_tol=1 << 17, pitch_tol=1 << 17, shift_tol=3)):
        total += len(_both(win_off, *cols, step, t16, f16, 20, **kw))
    assert total or not win_off[-1]


def _two(t16, f16, v0, v1, d1, step=22, **kw):
    """Two hits in neighbouring windows of song 1: variant v0 at position 100, v1 at 100 + W_t(v1)(step) + d1."""
    delta = np.asarray([100, 100 + SW.W(step, int(t16[v1])) + d1], np.int32)
    return _both([0, 2], np.asarray([1, 1], np.uint32), delta, np.asarray([30, 30], np.uint32), np.asarray([1, 1], np.uint32),
                 np.asarray([v0, v1], np.uint32), step, t16, f16, 20, **kw)


def test_tolerances_at_exactly_tol_and_one_above():
    t16 = np.asarray([65536, 65636, 65637, 65436], np.uint32)
    f16 = np.asarray([65536, 65536, 65536, 65536], np.uint32)
    kw = dict(tempo_tol=100, pitch_tol=7, shift_tol=3)
    assert len(_two(t16, f16, 0, 1, 0, **kw)) == 1 and len(_two(t16, f16, 0, 2, 0, **kw)) == 2      # tempo: 100, 101 apart
    assert len(_two(t16, f16, 1, 0, 0, **kw)) == 1 and len(_two(t16, f16, 0, 3, 0, **kw)) == 1      # either direction
    assert len(_two(f16, t16 - 93, 0, 1, 0, **kw)) == 2                                              # pitch: 100 apart, tol 7
    p16 = np.asarray([65536, 65543, 65544, 65529], np.uint32)
    assert len(_two(f16, p16, 0, 1, 0, **kw)) == 1 and len(_two(f16, p16, 0, 2, 0, **kw)) == 2      # pitch: 7, 8 apart
    assert len(_two(f16, p16, 3, 0, 0, **kw)) == 1
    for d, n in ((3, 1), (-3, 1), (4, 2), (-4, 2)):                                                  # the shift
        assert len(_two(t16, f16, 0, 1, d, **kw)) == n, d
    seg = _two(t16, f16, 0, 1, 3, **kw)[0]
    assert (seg["first"], seg["last"], seg["hits"], seg["pos_first"], seg["pos_last"]) == (0, 1, 2, 100, 100 + SW.W(22, 65636) + 3)
    assert seg["warp"] == 0                      # one hit each: the tie goes to the pair nearest (65536, 65536)


def test_the_advance_uses_the_time_factor_alone():
    t16, f16 = np.asarray([98304, 65536], np.uint32), np.asarray([65536, 131072], np.uint32)
    kw = dict(tempo_tol=1 << 17, pitch_tol=1 << 17, shift_tol=0)
    assert len(_two(t16, f16, 1, 0, 0, **kw)) == 1         # 33 frames a 22-frame step at tempo 1.5
    assert len(_two(t16, f16, 0, 1, 0, **kw)) == 1         # 22 at pitch 2, tempo 1
    assert len(_two(t16, f16, 0, 1, 11, **kw)) == 2


def test_no_warp_on_windows_that_are_no_hit_and_bad_indices_on_hits():
    t16 = f16 = np.asarray([65536, 65600], np.uint32)
    sid, aligned = np.ones(4, np.uint32), np.asarray([30, 5, 30, 30], np.uint32)
    delta, nres = np.asarray([0, 0, 44, 66], np.int32), np.asarray([1, 1, 1, 0], np.uint32)
    best = np.asarray([0, SW.NO_WARP, 0, SW.NO_WARP], np.uint32)
    segs = _both([0, 4], sid, delta, aligned, nres, best, 22, t16, f16, 20, max_gap=1)
    assert len(segs) == 1 and (segs[0]["first"], segs[0]["last"], segs[0]["hits"]) == (0, 2, 2)
    best[2] = 2                                          # a hit must name a variant of the list
    rc, _, _ = _ffi.scan_timeline_warps_raw([0, 4], sid, delta, aligned, nres, best, 22, t16, f16, 20)
    assert rc == _ffi.E_INVALID
    for bad_t, bad_f in (([32767], [65536]), ([65536], [131073])):
        rc, _, _ = _ffi.scan_timeline_warps_raw([0, 4], sid, delta, aligned, nres, best * 0, 22, bad_t, bad_f, 20)
        assert rc == _ffi.E_INVALID
    with pytest.raises(_ffi.ShzError):
        _ffi.scan_timeline_warps([0, 4], sid, delta, aligned, nres, best, 22, t16, f16, 20)


def test_the_most_chosen_variant_and_its_ties():
    t16 = np.asarray([65700, 65536, 65536, 65600], np.uint32)
    f16 = np.asarray([65536, 65600, 65472, 65536], np.uint32)
    n = 6
    best = np.asarray([0, 1, 2, 2, 1, 3], np.uint32)       # 1 and 2 twice each, the same distance: the lower index
    delta = np.cumsum([SW.W(10, int(t16[v])) for v in best]).astype(np.int32)
    segs = _both([0, n], np.ones(n, np.uint32), delta, np.full(n, 50, np.uint32), np.ones(n, np.uint32), best, 10, t16, f16, 20,
                 tempo_tol=200, pitch_tol=200, shift_tol=0)
    assert len(segs) == 1 and segs[0]["warp"] == 1 and segs[0]["hits"] == 6


def test_the_capacity_two_call():
    rng = np.random.default_rng(77)
    t16, f16 = np.asarray([65536, 62783, 68289], np.uint32), np.asarray([65536, 65615, 65457], np.uint32)
    cols = _walk(rng, 120, t16, f16, 7, 2, 20)
    args = ([0, 50, 120], *cols, 7, t16, f16, 20, 1, 0, 0, 2)
    want = SW.timeline([0, 50, 120], *cols, 7, t16, f16, 20)
    assert len(want) > 3
    rc, _, n = _ffi.scan_timeline_warps_raw(*args, 0)
    assert rc == _ffi.E_CAPACITY and n == len(want)
    rc, seg, n = _ffi.scan_timeline_warps_raw(*args, 2)
    assert rc == _ffi.E_CAPACITY and n == len(want) and _segs(seg) == want[:2]
    rc, seg, n = _ffi.scan_timeline_warps_raw(*args, len(want))
    assert rc == _ffi.OK and n == len(want) and _segs(seg) == want
    rc, _, n = _ffi.scan_timeline_warps_raw([0], *(c[:0] for c in cols), 7, t16, f16, 20)
    assert rc == _ffi.OK and n == 0


@pytest.mark.parametrize("seed", range(4))
def test_a_uniform_diagonal_ladder_is_the_speed_timeline(seed):
    """Both tolerances at the rung spacing on a sorted uniform ladder: neighbours at most one rung apart, shz_scan_timeline_speeds
    with rung_tol = 1."""
    rng = np.random.default_rng([0xD1A6, seed])
    ladder = (65536 + 92 * np.arange(-4, 5)).astype(np.uint32)
    cols = _walk(rng, 90, ladder, ladder, 22, 2, 20)
    cols = cols[:4] + (np.where(cols[4] == SW.NO_WARP, 0, cols[4]).astype(np.uint32),)   # the speed timeline checks every entry
    win_off = [0, 30, 30, 90]
    for max_gap, shift_tol in ((0, 0), (1, 2), (2, 3)):
        a = _ffi.scan_timeline_warps(win_off, *cols, 22, ladder, ladder, 20, max_gap, 92, 92, shift_tol)
        b = _ffi.scan_timeline_speeds(win_off, *cols, 22, ladder, 20, max_gap, 1, shift_tol)
        assert len(a["rec"]) > 2
        for k in FIELDS:
            assert np.array_equal(a[k], b["rung" if k == "warp" else k]), k
        assert _segs(a) == [dict((("warp", v) if k == "rung" else (k, v)) for k, v in s.items())
                            for s in ST.timeline(win_off, *cols, 22, ladder, 20, max_gap, 1, shift_tol)]


def test_the_advance_is_exact_where_gap_step_and_factor_need_more_than_64_bits():
    """Two hits 2^17 windows apart, step 2^31, time factor 1: the song advances 2^48 frames, and gap x step x t16 = 2^64 is 0
    in 64 bits -- which would continue the segment at equal positions.  Both timelines keep two segments, as the twins do;
    at a gap of 2^15 the product still fits and says the same."""
    one = np.asarray([65536], np.uint32)
    for gap in (1 << 15, 1 << 17):
        n = gap + 1
        sid, delta, aligned, nres = np.ones(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.uint32), np.ones(n, np.uint32)
        aligned[[0, gap]] = 50
        best = np.zeros(n, np.uint32)
        kw = dict(max_gap=(1 << 32) - 1, shift_tol=(1 << 32) - 1)
        want = _both([0, n], sid, delta, aligned, nres, best, 1 << 31, one, one, 20, **kw)
        assert [(s["first"], s["last"], s["hits"]) for s in want] == [(0, 0, 1), (gap, gap, 1)]
        got = _ffi.scan_timeline_speeds([0, n], sid, delta, aligned, nres, best, 1 << 31, one, 20, rung_tol=0, **kw)
        assert got["first"].tolist() == [0, gap] and got["hits"].tolist() == [1, 1]
    # the largest accepted step and gap, the largest factor: far beyond every position, exact in the library and the twin
    n = 3
    two = np.asarray([131072], np.uint32)
    sid, delta, aligned, nres, best = np.ones(n, np.uint32), np.zeros(n, np.int32), np.full(n, 50, np.uint32), np.ones(n, np.uint32), np.zeros(n, np.uint32)
    assert len(_both([0, n], sid, delta, aligned, nres, best, (1 << 32) - 1, two, two, 20, max_gap=(1 << 32) - 1, shift_tol=(1 << 32) - 1)) == 3
