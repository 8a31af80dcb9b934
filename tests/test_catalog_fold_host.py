"""CPU: fold_pairs (shazam_amd/catalog.py), the host half of find_duplicates, on hand-made match_songs arrays -- one record
per unordered pair of songs, a's side kept where both sides report, the four relations at their threshold edges, the
clusters of "same" -- and the two catalogue entry points refusing NULL handles before anything touches a device."""
import numpy as np

from shazam_amd import _ffi
from shazam_amd.catalog import PAIR_FIELDS, fold_pairs


def _arrays(listed, answers, topn=3):
    """match_songs arrays from {listed song: [(found song, delta, aligned), ...]}"""
    n = len(listed)
    sid, delta, aligned = np.zeros((n, topn), np.uint32), np.zeros((n, topn), np.int32), np.zeros((n, topn), np.uint32)
    nres = np.zeros(n, np.uint32)
    for q, s in enumerate(listed):
        for i, (o, d, a) in enumerate(answers.get(s, [])):
            sid[q, i], delta[q, i], aligned[q, i] = o, d, a
        nres[q] = len(answers.get(s, []))
    return sid, delta, aligned, nres


def _by_pair(out):
    return {(int(p["a"]), int(p["b"])): p for p in out["pairs"]}


def test_pair_seen_from_both_sides_keeps_a_side_and_its_delta():
    """songs 3 and 8 tie between two deltas: 3 names +17, 8 names -40 (from 8, 3 lies at 40 - that is delta +40 for the
    pair): a's side wins, so the pair says 17; listed order must not matter"""
    rows = {3: 100, 8: 100}
    for listed in ([3, 8], [8, 3]):
        sid, delta, aligned, nres = _arrays(listed, {3: [(8, 17, 60)], 8: [(3, -40, 60)]})
        out = fold_pairs(listed, sid, delta, aligned, nres, list(rows), list(rows.values()), 10, 0.5)
        assert len(out["pairs"]) == 1
        p = out["pairs"][0]
        assert (p["a"], p["b"], p["delta"], p["aligned"]) == (3, 8, 17, 60)
        assert (p["rows_a"], p["rows_b"]) == (100, 100) and p["coverage_a"] == 0.6 and p["relation"] == "same"
        assert out["clusters"] == [[3, 8]]


def test_pair_seen_from_one_side_only():
    """from a's side the delta stands; from b's side alone (a was not listed) it changes sign: delta is off_b - off_a"""
    sid, delta, aligned, nres = _arrays([5], {5: [(9, 23, 50)]})
    p = fold_pairs([5], sid, delta, aligned, nres, [5, 9], [50, 50], 10, 0.5)["pairs"][0]
    assert (p["a"], p["b"], p["delta"]) == (5, 9, 23)
    sid, delta, aligned, nres = _arrays([9], {9: [(5, -23, 50)]})
    p = fold_pairs([9], sid, delta, aligned, nres, [9, 5], [50, 50], 10, 0.5)["pairs"][0]
    assert (p["a"], p["b"], p["delta"], p["aligned"]) == (5, 9, 23, 50)


def test_the_four_relations_and_their_threshold_edges():
    """min_aligned 10, min_coverage 0.5; equality counts as reached on both"""
    rows = {1: 100, 2: 100, 3: 40, 4: 400, 5: 20, 6: 1000, 7: 1000}
    answers = {
        1: [(2, 0, 50),      # 50 / 100 and 50 / 100: both exactly at 0.5 -> same
            (3, 5, 20),      # 20 / 100 < 0.5, 20 / 40 = 0.5 -> b_in_a
            (4, -3, 49)],    # 49 / 100 < 0.5, 49 / 400 -> overlap (49 >= 10)
        5: [(6, 7, 10),      # 10 / 20 = 0.5, 10 / 1000 -> a_in_b, aligned exactly at min_aligned
            (7, 7, 9)],      # 9 < min_aligned -> dropped
        6: [(7, 1, 499)],    # 0.499 both -> overlap
    }
    listed = [1, 5, 6]
    sid, delta, aligned, nres = _arrays(listed, answers)
    out = fold_pairs(listed, sid, delta, aligned, nres, list(rows), list(rows.values()), 10, 0.5)
    got = {k: str(v["relation"]) for k, v in _by_pair(out).items()}
    assert got == {(1, 2): "same", (1, 3): "b_in_a", (1, 4): "overlap", (5, 6): "a_in_b", (6, 7): "overlap"}
    p = _by_pair(out)
    assert p[(1, 3)]["coverage_a"] == 0.2 and p[(1, 3)]["coverage_b"] == 0.5
    assert p[(5, 6)]["aligned"] == 10 and p[(5, 6)]["coverage_a"] == 0.5 and p[(5, 6)]["coverage_b"] == 0.01
    assert out["clusters"] == [[1, 2]]
    assert [(int(x["a"]), int(x["b"])) for x in out["pairs"]] == sorted(p)          # ordered by (a, b)
    # one less row aligned, or one more row in the song, and "same" is gone
    sid, delta, aligned, nres = _arrays([1], {1: [(2, 0, 49)]})
    assert fold_pairs([1], sid, delta, aligned, nres, [1, 2], [100, 100], 10, 0.5)["pairs"][0]["relation"] == "overlap"
    sid, delta, aligned, nres = _arrays([1], {1: [(2, 0, 50)]})
    assert fold_pairs([1], sid, delta, aligned, nres, [1, 2], [100, 101], 10, 0.5)["pairs"][0]["relation"] == "a_in_b"


def test_entries_past_nres_are_ignored():
    sid, delta, aligned, nres = _arrays([1], {1: [(2, 0, 50)]})
    sid[0, 1], aligned[0, 1] = 77, 1000                                             # stale cell behind nres
    out = fold_pairs([1], sid, delta, aligned, nres, [1, 2], [100, 100], 10, 0.5)
    assert [(int(p["a"]), int(p["b"])) for p in out["pairs"]] == [(1, 2)]


def test_clusters_follow_chains_and_stay_apart():
    """a~b and b~c make one cluster although a and c never met; d~e is another; f only overlaps and joins none"""
    rows = {10: 100, 20: 100, 30: 100, 40: 80, 41: 80, 50: 1000}
    answers = {10: [(20, 0, 90)], 20: [(10, 0, 90), (30, 4, 80)], 30: [(20, -4, 80)], 41: [(40, 0, 80), (50, 9, 30)]}
    listed = [41, 30, 20, 10]
    sid, delta, aligned, nres = _arrays(listed, answers)
    out = fold_pairs(listed, sid, delta, aligned, nres, list(rows), list(rows.values()), 10, 0.5)
    assert out["clusters"] == [[10, 20, 30], [40, 41]]
    p = _by_pair(out)
    assert set(p) == {(10, 20), (20, 30), (40, 41), (41, 50)}
    assert p[(20, 30)]["delta"] == 4 and p[(40, 41)]["delta"] == 0 and p[(41, 50)]["relation"] == "overlap"
    # a longer chain listed back to front ends in one component
    chain = list(range(1, 9))
    answers = {s: [(s + 1, 0, 10)] for s in chain[:-1]}
    sid, delta, aligned, nres = _arrays(chain[::-1], answers)
    out = fold_pairs(chain[::-1], sid, delta, aligned, nres, chain, [10] * 8, 1, 1.0)
    assert out["clusters"] == [chain]


def test_empty_input():
    out = fold_pairs([], np.zeros((0, 5)), np.zeros((0, 5)), np.zeros((0, 5)), [], [], [], 10, 0.5)
    assert len(out["pairs"]) == 0 and out["clusters"] == []
    assert out["pairs"].dtype.names == tuple(n for n, _ in PAIR_FIELDS)
    sid, delta, aligned, nres = _arrays([4, 6], {})                                 # songs listed, nothing found
    out = fold_pairs([4, 6], sid, delta, aligned, nres, [4, 6], [10, 10], 10, 0.5)
    assert len(out["pairs"]) == 0 and out["clusters"] == []


def test_catalog_entries_refuse_null_handles_without_a_gpu():
    """shz_table_song_hashes / shz_match_songs: no table, no context -> SHZ_E_INVALID before anything touches a device, the
    output words as they were"""
    L = _ffi.lib()
    sids = np.array([1, 2], np.uint32)
    row_off = np.full(3, 7, np.uint64)
    assert L.shz_table_song_hashes(None, _ffi.ptr(sids), 2, row_off.ctypes.data_as(_ffi.u64p), None, None, 0, 0) == _ffi.E_INVALID
    assert row_off.tolist() == [7, 7, 7]
    rows, nres = np.full(2, 9, np.uint64), np.full(2, 9, np.uint32)
    cells = [np.full(4, 9, t) for t in (np.uint32, np.int32, np.uint32, np.uint32)]
    rc = L.shz_match_songs(None, None, _ffi.ptr(sids), 2, 2, 0, _ffi.ptr(rows), *[_ffi.ptr(c) for c in cells], _ffi.ptr(nres),
                           None, None)
    assert rc == _ffi.E_INVALID
    assert rows.tolist() == [9, 9] and nres.tolist() == [9, 9] and all(c.tolist() == [9] * 4 for c in cells)
    assert _ffi.SONGS_DEVICE_OUT == 128
