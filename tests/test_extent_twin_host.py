"""CPU: the definition of the match extents (tests/extent_twin.py) against the definition of the vote (tests/vote_tol_twin.py),
extent.dense_span on hand-made histograms, and the two entry points' refusal of NULL handles without a GPU."""
import numpy as np
import pytest

from extent_twin import extents, shift_of
from vote_tol_twin import matches_of, vote_tol


def _random_case(seed):
    rng = np.random.default_rng(seed)
    rows = [(int(rng.integers(0, 30)), int(rng.integers(1, 5)), int(rng.integers(0, 25))) for _ in range(300)]
    hashes = [(int(rng.integers(0, 30)), int(rng.integers(0, 25))) for _ in range(int(rng.integers(0, 60)))]
    return rows, hashes


@pytest.mark.parametrize("seed", range(8))
def test_count_is_aligned_of_the_vote_at_tolerance_0(seed):
    rows, hashes = _random_case(seed)
    matches, _, _ = matches_of(rows, hashes)
    winners = vote_tol(matches, 0, topn=4)
    got, shift = extents(rows, hashes, [(s, d, d) for s, d, _ in winners])
    assert shift == shift_of(q for _, q in hashes)
    for (s, d, aligned), e in zip(winners, got):
        assert e["count"] == aligned and aligned > 0
        assert sum(e["hist"]) == e["count"]
        assert e["q_first"] <= e["q_last"] and e["t_first"] <= e["t_last"]
        assert e["t_first"] - e["q_first"] == d == e["t_last"] - e["q_last"]     # (one delta: both ends move together)


@pytest.mark.parametrize("seed", range(4))
def test_ranges_sum_their_bins_and_overlapping_candidates_share_pairs(seed):
    rows, hashes = _random_case(100 + seed)
    matches, _, _ = matches_of(rows, hashes)
    for sid in (1, 2):
        per_d = {}
        for s, d in matches:
            if s == sid:
                per_d[d] = per_d.get(d, 0) + 1
        got, _ = extents(rows, hashes, [(sid, -3, 2), (sid, 0, 5), (sid, 90, 95)])
        assert got[0]["count"] == sum(n for d, n in per_d.items() if -3 <= d <= 2)
        assert got[1]["count"] == sum(n for d, n in per_d.items() if 0 <= d <= 5)
        assert got[2] == {"count": 0, "q_first": 0, "q_last": 0, "t_first": 0, "t_last": 0, "hist": [0] * 64}
        for e in got:
            assert sum(e["hist"]) == e["count"]


@pytest.mark.parametrize("top, want", [(0, 0), (63, 0), (64, 1), (127, 1), (128, 2), ((1 << 20) - 1, 14)])
def test_shift(top, want):
    assert shift_of([0, top]) == want
    _, shift = extents([(1, 1, top)], [(1, top), (1, 0)], [(1, 0, 0)])
    assert shift == want
    assert shift_of([]) == 0


def test_duplicate_hashes_collapse_and_hist_buckets():
    rows = [(7, 1, 100), (7, 1, 164), (8, 1, 228)]
    hashes = [(7, 0), (7, 0), (7, 64), (8, 128), (8, 129)]
    got, shift = extents(rows, hashes, [(1, 100, 100)])
    assert shift == 2                                   # 129 >> 2 = 32
    e = got[0]
    assert e["count"] == 3 and (e["q_first"], e["q_last"], e["t_first"], e["t_last"]) == (0, 128, 100, 228)
    assert e["hist"][0] == 1 and e["hist"][16] == 1 and e["hist"][32] == 1 and sum(e["hist"]) == 3


def test_dense_span():
    from shazam_amd.extent import DENSE_MIN_COUNT, dense_span
    h = np.zeros(64, np.uint32)
    assert dense_span(h, 0) is None
    h[3] = 1                                            # one chance pair
    h[10:20] = 5
    h[40] = 1
    assert dense_span(h, 0, min_count=2) == (10, 20)
    assert dense_span(h, 3, min_count=2) == (80, 160)
    assert dense_span(h, 0, min_count=1) == (3, 41)
    assert dense_span(h, 0, min_count=6) is None
    assert dense_span(h, 0) == dense_span(h, 0, min_count=DENSE_MIN_COUNT)
    h[63] = 9
    assert dense_span(h, 14, min_count=2) == (10 << 14, 64 << 14)
    with pytest.raises(ValueError):
        dense_span(np.zeros(63), 0)


def test_entry_points_refuse_null_handles_without_a_gpu():
    from shazam_amd import _ffi
    L = _ffi.lib()
    out = np.full(4, 7, np.uint32)
    p = _ffi.ptr(out)
    assert L.shz_match_extents(None, None, None, None, None, 1, 1, p, p, p, p, p, p, p, p, p, None, p) == _ffi.E_INVALID
    assert L.shz_match_songs_extents(None, None, p, 1, 1, p, p, p, p, p, p, p, p, p, None, p) == _ffi.E_INVALID
    assert out.tolist() == [7, 7, 7, 7]
