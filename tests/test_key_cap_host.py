"""CPU: the key cap's definition (tests/key_cap_twin.py) on tables made by hand, and the arithmetic of shazam_amd.keycap on
built histograms.  No GPU; every comparison is exact."""
from fractions import Fraction

import numpy as np
import pytest

from key_cap_twin import dropped, expected_match_cap, kept_rows
from shazam_amd import floor, keycap
from vote_tol_twin import expected_match


def _table(sizes):
    """key k + 1 holds sizes[k] rows: song = the row's number under its key, offset 100 + that"""
    tk = np.concatenate([np.full(n, k + 1) for k, n in enumerate(sizes)]).astype(np.uint32)
    ts = np.concatenate([np.arange(n) for n in sizes]).astype(np.uint32)
    return tk, ts, (ts + 100).astype(np.uint32)


@pytest.mark.parametrize("c", [1, 2, 16, 17, 64])
def test_a_key_at_the_cap_stays_and_one_above_goes(c):
    tk, ts, to = _table([1, c, c + 1])
    m = kept_rows(tk, c)
    assert m[tk == 1].all() and m[tk == 2].all() and not m[tk == 3].any()
    assert kept_rows(tk, c + 1).all() and kept_rows(tk, 0).all() and kept_rows(tk, (1 << 64) - 1).all()
    assert np.array_equal(kept_rows(tk, c, ts, to), m)
    qk, qo, qoff = np.array([1, 2, 3, 3], np.uint32), np.array([5, 5, 5, 6], np.uint32), np.array([0, 4], np.uint64)
    (ranked, npairs, nhash), = expected_match_cap(tk, ts, to, qk, qo, qoff, 0, 3, c)
    assert npairs == 1 + c and nhash == 4
    assert dropped(tk, ts, to, qk, qo, qoff, c) == (1, 2 * (c + 1))
    assert dropped(tk, ts, to, qk, qo, qoff, c + 1) == (0, 0) == dropped(tk, ts, to, qk, qo, qoff, 0)
    assert expected_match_cap(tk, ts, to, qk, qo, qoff, 0, 3, c + 1) == expected_match(tk, ts, to, qk, qo, qoff, 0, 3)


def test_duplicate_rows_count_once():
    tk, ts, to = _table([3, 2])
    tk2, ts2, to2 = (np.concatenate([a, a[:3], a[:3]]) for a in (tk, ts, to))   # key 1's three rows, three times each
    assert kept_rows(tk2, 3, ts2, to2).all()                                    # three distinct rows: at the cap
    m = kept_rows(tk2, 2, ts2, to2)
    assert not m[tk2 == 1].any() and m[tk2 == 2].all()
    assert not kept_rows(tk2, 8)[tk2 == 1].any()                                # (keys alone: nine entries)
    qk, qo, qoff = np.array([1, 2], np.uint32), np.array([0, 0], np.uint32), np.array([0, 2], np.uint64)
    assert expected_match_cap(tk2, ts2, to2, qk, qo, qoff, 0, 4, 3) == expected_match(tk, ts, to, qk, qo, qoff, 0, 4)
    assert dropped(tk2, ts2, to2, qk, qo, qoff, 2) == (1, 3)


def test_bucket_hi_against_bucket_lo_at_all_buckets():
    for b in range(31):
        hi = keycap.bucket_hi(b)
        assert hi == floor.bucket_lo(b + 1) - 1 and hi >= floor.bucket_lo(b)
        assert floor.bucket_of(hi) == b and floor.bucket_of(hi + 1) == b + 1
    assert keycap.bucket_hi(31) == (1 << 64) - 1 and floor.bucket_of((1 << 64) - 1) == 31
    for b in (-1, 32):
        with pytest.raises(ValueError):
            keycap.bucket_hi(b)


def _hist(sizes):
    """the histogram Table.key_hist() gives for keys of these sizes"""
    keys, rows = np.zeros(32, np.uint64), np.zeros(32, np.uint64)
    for n in sizes:
        keys[floor.bucket_of(n)] += np.uint64(1)
        rows[floor.bucket_of(n)] += np.uint64(n)
    return {"keys": keys, "rows": rows, "max_rows": max(sizes, default=0), "n_keys": len(sizes)}


def test_all_rows_in_one_bucket():
    h = _hist([20] * 7)                                 # bucket 16: 17 .. 31
    for keep in (Fraction(1), Fraction(1, 2), Fraction(1, 140), 0.3):
        assert keycap.cap_for(h, keep) == 31
    assert keycap.cap_for(h, 0) == 1
    assert keycap.rows_kept(h, 16) == 0 and keycap.rows_kept(h, 19) == 0 and keycap.rows_kept(h, 30) == 140
    assert keycap.rows_kept(h, 20) == 140 and keycap.rows_kept(h, 31) == 140 and keycap.rows_kept(h, 0) == 140
    assert keycap.rows_kept(h["rows"], 20) == 0 and keycap.rows_kept(h["rows"], 31) == 140     # (no maximum known)


def test_keep_one_and_keep_zero_and_an_empty_histogram():
    h = _hist([1] * 10 + [3] * 5 + [16] * 2 + [100] + [5000])
    total = 10 + 15 + 32 + 100 + 5000
    assert keycap.cap_for(h, 1) == keycap.cap_for(h, Fraction(1)) == keycap.cap_for(h, 1.0) == 8191
    assert keycap.rows_kept(h, 8191) == total
    assert keycap.cap_for(h, 0) == 1 and keycap.rows_kept(h, 1) == 10
    assert [keycap.rows_kept(h, c) for c in (2, 3, 15, 16, 127, 4095)] == [10, 25, 25, 57, 157, 157]
    assert keycap.share_kept(h, 16) == Fraction(57, total)
    e = _hist([])
    assert keycap.cap_for(e, 1) == 0 and keycap.cap_for(e, 0) == 0 and keycap.cap_for(e, Fraction(1, 2)) == 0
    assert keycap.rows_kept(e, 5) == 0 and keycap.share_kept(e, 5) == 1
    for bad in (Fraction(-1, 10), Fraction(11, 10), 1.5):
        with pytest.raises(ValueError):
            keycap.cap_for(h, bad)
    with pytest.raises(ValueError):
        keycap.rows_kept(np.zeros(31), 1)


def test_a_keep_met_exactly_at_an_edge():
    h = _hist([1] * 10 + [2] * 20 + [40])              # 10 + 40 + 40 rows
    assert keycap.cap_for(h, Fraction(50, 90)) == 2     # the keys of at most 2 rows hold exactly 50 of 90
    assert keycap.cap_for(h, Fraction(50, 90) + Fraction(1, 10 ** 30)) == 63
    assert keycap.cap_for(h, Fraction(10, 90)) == 1 and keycap.cap_for(h, Fraction(11, 90)) == 2
    # a float is converted once and compared exactly: 0.1 as a binary fraction lies above 1/10
    h10 = _hist([1] * 1 + [2] * 0 + [9])
    assert keycap.cap_for(h10, Fraction(1, 10)) == 1 and keycap.cap_for(h10, 0.1) == 9
    # the open last bucket: its edge is the table's largest key
    big = _hist([4] * 3 + [1 << 20])
    assert keycap.cap_for(big, 1) == 1 << 20 and keycap.rows_kept(big, 1 << 20) == 12 + (1 << 20)
    assert keycap.rows_kept(big, (1 << 20) - 1) == 12 and keycap.cap_for(big["rows"], 1) == keycap.CAP_MAX
