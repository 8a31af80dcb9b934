"""CPU: fold_pairs_warps (shazam_amd/catalog.py), the host half of find_duplicates at a ladder, on hand-made
match_songs arrays with a warp axis -- the best-of rule over both sides and all warps with each of its tie-breaks, the sign
of delta when b's side wins, aligned_plain, thresholds, relations, clusters, empty input -- and the ladder keywords read
into pair lists.  No GPU."""
import numpy as np
import pytest

from shazam_amd import _ffi
from shazam_amd.catalog import (MIN_ALIGNED_WARPED, MIN_COVERAGE_WARPED, PAIR_FIELDS, WARP_PAIR_FIELDS, _ladder_of, fold_pairs,
                                fold_pairs_warps)

ONE = 65536
T16 = np.array([63570, ONE, 67502, 65000], np.uint32)       # 0.97, 1.0, 1.03 and a near rung
F16 = np.array([63570, ONE, 67502, ONE], np.uint32)         # |t - 1| + |f - 1|: 3932, 0, 3932, 536


def _arrays(listed, answers, K=len(T16), topn=3):
    """arrays of match_songs at K warps from {(listed song, warp): [(found song, delta, aligned), ...]}"""
    n = len(listed)
    sid, delta, aligned = (np.zeros((n, K, topn), t) for t in (np.uint32, np.int32, np.uint32))
    nres = np.zeros((n, K), np.uint32)
    for q, s in enumerate(listed):
        for v in range(K):
            for i, (o, d, a) in enumerate(answers.get((s, v), [])):
                sid[q, v, i], delta[q, v, i], aligned[q, v, i] = o, d, a
            nres[q, v] = len(answers.get((s, v), []))
    return sid, delta, aligned, nres


def _fold(listed, answers, rows, min_aligned=10, min_coverage=0.5, t16=T16, f16=F16):
    sid, delta, aligned, nres = _arrays(listed, answers, K=len(t16))
    return fold_pairs_warps(listed, t16, f16, sid, delta, aligned, nres, list(rows), list(rows.values()), min_aligned, min_coverage)


def _by_pair(out):
    return {(int(p["a"]), int(p["b"])): p for p in out["pairs"]}


def test_the_greatest_count_over_both_sides_and_all_warps_is_kept():
    """song 13 is song 1 played 1.03 times as fast: 13's rows at 1.03 meet song 1 (b's side, 466), song 1's rows at 0.97
    meet 13 less well (a's side, 200), both see noise at 1.0"""
    rows = {1: 3090, 13: 3130}
    answers = {(1, 0): [(13, 4, 200)], (1, 1): [(13, -9, 14)], (13, 1): [(1, 31, 12)], (13, 2): [(1, -2, 466)]}
    for listed in ([1, 13], [13, 1]):
        out = _fold(listed, answers, rows, 100, 0.1)
        assert len(out["pairs"]) == 1
        p = out["pairs"][0]
        assert (p["a"], p["b"], p["aligned"], p["warped"]) == (1, 13, 466, "b")
        assert (p["tempo_q16"], p["pitch_q16"]) == (67502, 67502)
        assert p["delta"] == 2                              # b said: a lies at -2 under my warped frame 0; seen from a: +2
        assert p["aligned_plain"] == 14                     # the greater of the two sides at (65536, 65536)
        assert (p["rows_a"], p["rows_b"]) == (3090, 3130)
        assert p["coverage_a"] == 466 / 3090 and p["coverage_b"] == 466 / 3130 and p["relation"] == "same"
        assert out["clusters"] == [[1, 13]]
    # a's side alone (13 was not listed): the 0.97 observation, delta as reported
    p = _fold([1], answers, rows, 100, 0.05)["pairs"][0]
    assert (p["aligned"], p["warped"], p["tempo_q16"], p["delta"], p["aligned_plain"]) == (200, "a", 63570, 4, 14)


def test_tie_breaks_in_order_distance_then_a_side_then_warp_index():
    rows = {2: 100, 5: 100}
    # equal counts at warps 0 (distance 3932) and 3 (distance 536), both from b's side: the nearer warp
    p = _fold([5], {(5, 0): [(2, 1, 60)], (5, 3): [(2, 7, 60)]}, rows)["pairs"][0]
    assert (p["tempo_q16"], p["pitch_q16"], p["warped"], p["delta"]) == (65000, ONE, "b", -7)
    # equal counts, equal distance (warps 0 and 2), one a side each: a's side, although its warp index is the higher
    p = _fold([2, 5], {(5, 0): [(2, 1, 60)], (2, 2): [(5, 3, 60)]}, rows)["pairs"][0]
    assert (p["warped"], p["tempo_q16"], p["delta"]) == ("a", 67502, 3)
    # equal counts, equal distance, the same side: the lower warp index
    p = _fold([2], {(2, 2): [(5, 3, 60)], (2, 0): [(5, 8, 60)]}, rows)["pairs"][0]
    assert (p["warped"], p["tempo_q16"], p["delta"]) == ("a", 63570, 8)
    # a greater count beats every tie-break: b's side, far warp, high index
    p = _fold([2, 5], {(2, 1): [(5, 0, 60)], (5, 2): [(2, 5, 61)]}, rows)["pairs"][0]
    assert (p["aligned"], p["warped"], p["tempo_q16"], p["delta"], p["aligned_plain"]) == (61, "b", 67502, -5, 60)
    # the distance adds both axes: (65300, 65300) at 236 + 236 is nearer than (65000, 65536) at 536
    t16, f16 = np.array([65000, 65300], np.uint32), np.array([ONE, 65300], np.uint32)
    p = _fold([2], {(2, 0): [(5, 1, 60)], (2, 1): [(5, 2, 60)]}, rows, t16=t16, f16=f16)["pairs"][0]
    assert (p["tempo_q16"], p["pitch_q16"], p["delta"]) == (65300, 65300, 2)


def test_aligned_plain_is_zero_without_the_identity_warp_or_without_a_plain_answer():
    rows = {2: 100, 5: 100}
    t16 = f16 = np.array([63570, 67502], np.uint32)
    p = _fold([2], {(2, 0): [(5, 1, 60)]}, rows, t16=t16, f16=f16)["pairs"][0]
    assert p["aligned_plain"] == 0 and p["aligned"] == 60
    p = _fold([2], {(2, 0): [(5, 1, 60)]}, rows)["pairs"][0]        # the ladder holds 65536, the pair is not listed there
    assert p["aligned_plain"] == 0
    p = _fold([2], {(2, 1): [(5, 1, 60)]}, rows)["pairs"][0]        # found at the identity itself
    assert (p["aligned_plain"], p["aligned"], p["tempo_q16"], p["warped"]) == (60, 60, ONE, "a")


def test_thresholds_relations_and_clusters():
    """min_aligned 10, min_coverage 0.5; equality counts as reached on both; coverage uses the PLAIN row counts"""
    rows = {1: 100, 2: 100, 3: 40, 4: 400, 5: 20, 6: 1000, 7: 1000, 8: 100}
    answers = {
        (1, 0): [(2, 0, 50),        # 0.5 / 0.5 -> same
                 (3, 5, 20)],       # 0.2 / 0.5 -> b_in_a
        (1, 2): [(4, -3, 49)],      # 0.49 / 0.12 -> overlap
        (5, 3): [(6, 7, 10),        # 0.5 / 0.01 -> a_in_b, aligned exactly at min_aligned
                 (7, 7, 9)],        # below min_aligned at its best -> dropped
        (5, 0): [(7, 2, 8)],
        (8, 2): [(2, 1, 70)],       # 2 ~ 8 joins 1 ~ 2: one cluster
    }
    out = _fold([1, 5, 8], answers, rows)
    got = {k: str(v["relation"]) for k, v in _by_pair(out).items()}
    assert got == {(1, 2): "same", (1, 3): "b_in_a", (1, 4): "overlap", (2, 8): "same", (5, 6): "a_in_b"}
    assert [(int(x["a"]), int(x["b"])) for x in out["pairs"]] == sorted(got)
    assert out["clusters"] == [[1, 2, 8]]
    assert _by_pair(out)[(2, 8)]["warped"] == "b" and _by_pair(out)[(2, 8)]["delta"] == -1
    # entries past nres are ignored
    sid, delta, aligned, nres = _arrays([1], {(1, 0): [(2, 0, 50)]})
    sid[0, 0, 1], aligned[0, 0, 1] = 77, 1000
    o2 = fold_pairs_warps([1], T16, F16, sid, delta, aligned, nres, [1, 2], [100, 100], 10, 0.5)
    assert [(int(p["a"]), int(p["b"])) for p in o2["pairs"]] == [(1, 2)]
    with pytest.raises(ValueError):
        fold_pairs_warps([1], T16, F16, sid, delta, aligned, nres, [1], [100], 10, 0.5)      # song 2 has no row count


def test_empty_input_and_the_record_layout():
    out = fold_pairs_warps([], T16, F16, np.zeros((0, 4, 5)), np.zeros((0, 4, 5)), np.zeros((0, 4, 5)), np.zeros((0, 4)), [], [])
    assert len(out["pairs"]) == 0 and out["clusters"] == []
    names = tuple(n for n, _ in WARP_PAIR_FIELDS)
    assert out["pairs"].dtype.names == names
    assert names[:len(PAIR_FIELDS)] == tuple(n for n, _ in PAIR_FIELDS)
    assert names[len(PAIR_FIELDS):] == ("tempo_q16", "pitch_q16", "warped", "aligned_plain")
    out = _fold([4, 6], {}, {4: 10, 6: 10})                         # songs listed, nothing found
    assert len(out["pairs"]) == 0 and out["clusters"] == []
    # fold_pairs and its record stay as they were
    assert tuple(n for n, _ in PAIR_FIELDS) == ("a", "b", "delta", "aligned", "rows_a", "rows_b", "coverage_a", "coverage_b", "relation")
    assert fold_pairs([], [], [], [], [], [], [], 10, 0.5)["pairs"].dtype.names == tuple(n for n, _ in PAIR_FIELDS)
    # the defaults lie between the measured distributions (unrelated <= 54 aligned and 0.018 covered at any of
    # 71 rungs; planted half a step beside a rung >= 154 and 0.046)
    assert 54 < MIN_ALIGNED_WARPED < 154 and 0.018 < MIN_COVERAGE_WARPED < 0.046


def test_ladder_keywords_become_pair_lists():
    assert _ladder_of(None, None, None, None) is None
    t, f, row = _ladder_of([63570, ONE], None, None, None)
    assert t.tolist() == f.tolist() == [63570, ONE] and row == 1 and t.dtype == np.uint32
    t, f, row = _ladder_of(None, [60000, ONE], [ONE, 65600, 65700], None)
    assert t.tolist() == [60000] * 3 + [ONE] * 3 and f.tolist() == [ONE, 65600, 65700] * 2 and row == 3
    t, f, row = _ladder_of(None, None, [65000, ONE], None)
    assert t.tolist() == [ONE, ONE] and f.tolist() == [65000, ONE] and row == 2
    t, f, row = _ladder_of(None, None, None, ([60000, 70000], [ONE, 65000]))
    assert t.tolist() == [60000, 70000] and f.tolist() == [ONE, 65000] and row == 1
    for bad in (([ONE], [ONE], None, None), ([ONE], None, None, ([ONE], [ONE])), (None, [ONE], None, ([ONE], [ONE]))):
        with pytest.raises(TypeError):
            _ladder_of(*bad)
    with pytest.raises(TypeError):
        _ladder_of([0.97, 1.0], None, None, None)                   # factors are Q16 integers
    with pytest.raises(ValueError):
        _ladder_of(None, None, None, ([ONE, ONE], [ONE]))


def test_catalog_warp_entries_refuse_null_handles_without_a_gpu():
    """shz_warp_rows / shz_match_songs_warps: no context, no table -> SHZ_E_INVALID before anything touches a device"""
    L = _ffi.lib()
    one = np.array([ONE], np.uint32)
    p = one.ctypes.data_as(_ffi.u32p)
    ro = np.zeros(2, np.uint64)
    assert L.shz_warp_rows(None, None, None, ro.ctypes.data_as(_ffi.u64p), 1, p, p, 1, 0, None, None, None, 0, None) == _ffi.E_INVALID
    nres = np.full(2, 9, np.uint32)
    rc = L.shz_match_songs_warps(None, None, _ffi.ptr(one), 1, 2, p, p, 1, 0, None, None, None, None, None, _ffi.ptr(nres), None,
                                 None, None, None, None)
    assert rc == _ffi.E_INVALID and nres.tolist() == [9, 9]
    assert _ffi.DEBUG_CATALOG_SMALL_SLICES == 64
