"""No GPU: the twin of shz_match_songs_warps_extents (tests/rows_fit_twin.py) against the twins it is composed from, and the
bookkeeping of catalog.pair_extents_warps -- the sign of d for a pair whose b side was warped, extent.own_frames, which of
a_* / b_* takes which field, the batches, the drift formula -- on a table whose match_songs_warps_extents IS the twin."""
from fractions import Fraction

import numpy as np
import pytest

from extent_twin import SCALARS, expected_extents
from fit_twin import SUMS, expected_moments, own_frames, warp_map
from rows_fit_twin import TwinTable, match_songs_warps_extents as twin, song_rows
from rows_warp_twin import warp_rows

ONE = 65536
DELTA, LO, HI = 37, 120, 219        # song 9: the images under UP of song 5's rows of the frames LO .. HI, shifted by DELTA
UP, DOWN, D2 = 67502, 62000, 21     # song 3: the images under DOWN of song 7's rows of the frames LO .. HI, shifted by D2


def _rows(rng, n, off_hi=300):
    f1, f2, dt = rng.integers(0, 2049, n), rng.integers(0, 2049, n), rng.integers(1, 101, n)
    return ((f1 << 20) | (f2 << 8) | dt).astype(np.int64), rng.integers(0, off_hi, n).astype(np.int64)


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(31)
    k5, o5 = _rows(rng, 400)
    k7, o7 = _rows(rng, 400)
    o5[:4] = o7[:4] = (LO, HI, LO - 1, HI + 1)
    in5, in7 = (o5 >= LO) & (o5 <= HI), (o7 >= LO) & (o7 <= HI)
    k9, o9, keep9 = warp_rows(k5[in5], o5[in5], UP, ONE)
    k3, o3, keep3 = warp_rows(k7[in7], o7[in7], DOWN, ONE)
    assert keep9.all() and keep3.all()
    ke, oe = _rows(rng, 200)
    tk = np.concatenate([k5, k7, k9.astype(np.int64), k3.astype(np.int64), ke])
    ts = np.concatenate([np.full(400, 5), np.full(400, 7), np.full(len(k9), 9), np.full(len(k3), 3), np.full(200, 8)])
    to = np.concatenate([o5, o7, o9.astype(np.int64) + DELTA, o3.astype(np.int64) + D2, oe])
    return tk, ts, to


def test_at_the_identity_the_twin_is_the_extent_and_fit_twins_on_the_songs_rows(rows):
    tk, ts, to = rows
    sids = [5, 9, 4, 3]                                                     # (song 4 has no rows)
    cs, lo, hi = [[9, 5], [5, 8], [5, 5], [7, 3]], [[-50, 0], [-300, -600], [0, 0], [-600, 0]], [[50, 0], [300, 600], [0, 0], [600, 0]]
    cn = [2, 2, 1, 2]
    parts = [song_rows(tk, ts, to, s) for s in sids]
    qk, qo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    qoff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])])
    got = twin(tk, ts, to, sids, [ONE] * 4, [ONE] * 4, cs, lo, hi, cn, hist=True)
    ext = expected_extents(tk, ts, to, qk, qo, qoff, cs, lo, hi, cn)
    mom = expected_moments(tk, ts, to, qk, qo, qoff, cs, lo, hi, cn)
    for q in range(4):
        assert int(got["shift"][q]) == ext[q][1] and int(got["kept"][q]) == len(parts[q][0])
        for c in range(2):
            assert {f: int(got[f][q, c]) for f in SCALARS} == {f: ext[q][0][c][f] for f in SCALARS}
            assert got["hist"][q, c].tolist() == ext[q][0][c]["hist"]
            assert {f: int(got[f][q, c]) for f in SUMS} == mom[q][c]
    assert int(got["count"][0, 1]) == 400 and int(got["count"][2, 0]) == 0 and int(got["kept"][2]) == 0


def _pairs(recs):
    from shazam_amd.catalog import WARP_PAIR_FIELDS
    p = np.zeros(len(recs), np.dtype(list(WARP_PAIR_FIELDS)))
    for i, (a, b, delta, t16, warped) in enumerate(recs):
        p["a"][i], p["b"][i], p["delta"][i], p["tempo_q16"][i], p["pitch_q16"][i], p["warped"][i] = a, b, delta, t16, ONE, warped
        p["aligned"][i], p["relation"][i] = 100 + i, "overlap"
    return p


def test_pair_extents_warps_bookkeeping_on_a_table_that_is_the_twin(rows):
    from shazam_amd.catalog import WARP_EXTENT_PAIR_FIELDS, WARP_PAIR_FIELDS, pair_extents_warps
    from shazam_amd.extent import own_frames as lib_own
    assert [f for f, _ in WARP_EXTENT_PAIR_FIELDS] == [f for f, _ in WARP_PAIR_FIELDS] + [
        "a_first", "a_last", "b_first", "b_last", "count", "warped_first", "warped_last", "tempo_fit", "drift_bins"]
    tk, ts, to = rows
    # (3, 7): song 7's rows were warped (side b); its side reported delta = D2, and fold_pairs_warps turned the sign
    pairs = _pairs([(3, 7, -D2, DOWN, "b"), (5, 9, DELTA, UP, "a"), (5, 8, 4, ONE, "a")])
    t = TwinTable(tk, ts, to)
    out = pair_extents_warps(t, pairs, tol=1, drift_bins=3)
    assert out.dtype == np.dtype(list(WARP_EXTENT_PAIR_FIELDS)) and len(t.calls) == 1
    for f, _ in WARP_PAIR_FIELDS:
        assert np.array_equal(out[f], pairs[f]), f
    call = t.calls[0]
    assert call["job_sid"] == [7, 5, 5] and call["tempos"] == [DOWN, UP, ONE] and call["pitches"] == [ONE] * 3
    assert np.ravel(call["cand_sid"]).tolist() == [3, 9, 8]
    assert np.ravel(call["d_lo"]).tolist() == [D2 - 4, DELTA - 4, 0] and np.ravel(call["d_hi"]).tolist() == [D2 + 4, DELTA + 4, 8]
    assert out["drift_bins"].tolist() == [3, 3, 3]
    # side a warped: a_* are song 5's own frames, b_* song 9's; the images lie on one line of slope 0
    p = out[1]
    wf, wl = warp_map(LO, UP), warp_map(HI, UP)
    assert (int(p["warped_first"]), int(p["warped_last"])) == (wf, wl)
    assert (int(p["a_first"]), int(p["a_last"])) == (LO, HI) == own_frames(wf, wl, UP) == lib_own(wf, wl, UP)
    assert (int(p["b_first"]), int(p["b_last"])) == (wf + DELTA, wl + DELTA)
    assert int(p["count"]) >= int(((to[ts == 5] >= LO) & (to[ts == 5] <= HI)).sum()) and p["tempo_fit"] == float(Fraction(UP, ONE))
    # side b warped: b_* are song 7's own frames (the map below 1.0 is not one to one: the search of fit_twin says which), a_* song 3's
    p = out[0]
    wf, wl = warp_map(LO, DOWN), warp_map(HI, DOWN)
    assert (int(p["warped_first"]), int(p["warped_last"])) == (wf, wl)
    assert (int(p["b_first"]), int(p["b_last"])) == own_frames(wf, wl, DOWN) == lib_own(wf, wl, DOWN)
    assert int(p["b_first"]) <= LO and int(p["b_last"]) >= HI and int(p["b_last"]) - int(p["b_first"]) <= HI - LO + 2
    assert (int(p["a_first"]), int(p["a_last"])) == (wf + D2, wl + D2)
    assert int(p["count"]) > 100 and p["tempo_fit"] == float(Fraction(DOWN, ONE))
    # nothing aligned: zeros, and no fit
    p = out[2]
    assert [int(p[f]) for f in ("a_first", "a_last", "b_first", "b_last", "count", "warped_first", "warped_last")] == [0] * 7
    assert np.isnan(p["tempo_fit"])
    # batches of whole jobs, one job at least: the same records
    t1 = TwinTable(tk, ts, to)
    one = pair_extents_warps(t1, pairs, tol=1, drift_bins=3, batch_rows=1)
    assert len(t1.calls) == 3 and [c["job_sid"] for c in t1.calls] == [[7], [5], [5]]
    for f, _ in WARP_EXTENT_PAIR_FIELDS:
        assert np.array_equal(one[f], out[f], equal_nan=True) if f == "tempo_fit" else np.array_equal(one[f], out[f]), f
    t2 = TwinTable(tk, ts, to)
    pair_extents_warps(t2, pairs, tol=0, drift_bins=0, batch_rows=800)
    assert [c["job_sid"] for c in t2.calls] == [[7, 5], [5]]
    none = pair_extents_warps(TwinTable(tk, ts, to), pairs[:0])
    assert len(none) == 0 and none.dtype == out.dtype


def test_a_rung_beside_the_true_factor_the_fit_moves_towards_the_truth(rows):
    """song 6 holds the images of ALL of song 5's rows under UP; the pair is 'found' at a rung 1.5 % below"""
    from shazam_amd.catalog import pair_extents_warps
    tk, ts, to = rows
    k6, o6, _ = warp_rows(tk[ts == 5], to[ts == 5], UP, ONE)
    t = TwinTable(np.concatenate([tk, k6.astype(np.int64)]), np.concatenate([ts, np.full(len(k6), 6)]), np.concatenate([to, o6.astype(np.int64) + 3]))
    rung = 66500
    out = pair_extents_warps(t, _pairs([(5, 6, 5, rung, "a")]), tol=0, drift_bins=8)
    true = UP / ONE
    assert int(out["count"][0]) > 50 and abs(out["tempo_fit"][0] - true) < abs(rung / ONE - true) / 2


def test_the_entry_point_without_a_context_is_invalid_before_anything_touches_a_device():
    from shazam_amd import _ffi
    L, a = _ffi.lib(), np.ones(4, np.uint32)
    p, q = _ffi.ptr(a), a.ctypes.data_as(_ffi.u32p)
    assert L.shz_match_songs_warps_extents(None, None, q, q, q, 1, 1, *([p] * 16), None, None, None) == _ffi.E_INVALID


def test_warp_drift_bins_is_the_formula():
    from shazam_amd.catalog import warp_drift_bins
    assert warp_drift_bins(1000, [UP], 0) == 0 and warp_drift_bins(1000, [UP, UP], 3) == 0                # one rung: no gap
    # t_max = (1000 * 67502 + 32768) >> 16 = 1030, gap 5502: ceil(1030 * 5502 / 131072) = 44
    assert warp_drift_bins(1000, [DOWN, UP, UP], 0) == 44 == -(-(((1000 * UP + 32768) >> 16) * (UP - DOWN)) // (2 * ONE))
    assert warp_drift_bins(1000, [DOWN, 64000, UP], 0) == -(-1030 * 3502 // (2 * ONE))                       # the LARGEST gap
    assert warp_drift_bins(10 ** 6, [DOWN, UP], 0) == 2047 and warp_drift_bins(10 ** 6, [DOWN, UP], 5) == 2042   # 2 (tol + drift) + 1 <= 4095
