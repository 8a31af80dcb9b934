"""The vote floor without a GPU: shz_vote_bucket against its Python restatement at every bucket edge, the twin of the two
histograms (tests/vote_floor_twin.py) against a brute-force count, the tail fit of shazam_amd.floor on inputs whose answer
is known in closed form, and the min_score filter of scan() on built arrays."""
import ctypes as C
import math

import numpy as np
import pytest

from vote_floor_twin import bucket_lo, bucket_of, floor_of


def _edge_counts():
    cs = {1, 16, 17, 31, 32, (1 << 32) - 1}
    for k in range(1, 33):
        cs.update(c for c in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 1 <= c < 1 << 32)
    return sorted(cs)


def test_vote_bucket_edges():
    from shazam_amd import _ffi, floor
    lib = _ffi.lib()
    b = C.c_uint32()
    for c in _edge_counts():
        assert lib.shz_vote_bucket(c, C.byref(b)) == _ffi.OK
        assert b.value == floor.bucket_of(c) == bucket_of(c), c
        assert floor.bucket_lo(b.value) <= c and (b.value == 31 or c < floor.bucket_lo(b.value + 1)), c
    for c, want in ((1, 0), (16, 15), (17, 16), (31, 16), (32, 17), (63, 17), (64, 18), ((1 << 19) - 1, 30), (1 << 19, 31),
                    ((1 << 32) - 1, 31)):
        assert floor.bucket_of(c) == want, c
    for bk in range(32):
        assert floor.bucket_of(floor.bucket_lo(bk)) == bk and floor.bucket_lo(bk) == bucket_lo(bk)
        assert bk == 0 or floor.bucket_of(floor.bucket_lo(bk) - 1) == bk - 1
    assert lib.shz_vote_bucket(0, C.byref(b)) == _ffi.E_INVALID
    assert lib.shz_vote_bucket(5, None) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        floor.bucket_of(0)


def _brute(matches, tol):
    """The definition, counted the slow way: every bin's multiplicity; per song the largest sum of tol + 1 neighbouring bins
    over the windows that start at an occupied bin."""
    song, bins = np.zeros(32, np.int64), np.zeros(32, np.int64)
    for s in {s for s, _ in matches}:
        ds = [d for t, d in matches if t == s]
        for d in set(ds):
            bins[bucket_of(ds.count(d))] += 1
        best = max(sum(1 for e in ds if d <= e <= d + tol) for d in set(ds))
        song[bucket_of(best)] += 1
    return song, bins


@pytest.mark.parametrize("tol", [0, 1, 31])
@pytest.mark.parametrize("seed", range(4))
def test_twin_against_brute_force(seed, tol):
    rng = np.random.default_rng(4100 + seed)
    n = int(rng.integers(0, 400))
    matches = list(zip(rng.integers(1, 6, n).tolist(), (rng.integers(-6, 7, n) * rng.integers(1, 4, n)).tolist()))
    if seed == 0:
        matches += [(9, 3)] * 40 + [(9, 4)] * 17 + [(8, -2)] * 16     # counts beyond the exact buckets
    song, bins = floor_of(matches, tol)
    bsong, bbins = _brute(matches, tol)
    assert song.tolist() == bsong.tolist() and bins.tolist() == bbins.tolist()
    assert int(song.sum()) == len({s for s, _ in matches}) and int(bins.sum()) == len(set(matches))


def test_fit_tail_geometric():
    """n_c = 2^(16 - c), c = 1 .. 16: ln n_c is a line exactly, so any correct weighted fit returns it; the bound covers
    float rounding only."""
    from shazam_amd import floor
    h = np.zeros(32, np.uint32)
    h[:16] = [1 << (16 - c) for c in range(1, 17)]
    alpha, beta = floor.fit_tail(h)
    assert abs(beta + math.log(2.0)) <= 1e-9 * math.log(2.0)
    assert abs(alpha - 16 * math.log(2.0)) <= 1e-9 * 16 * math.log(2.0)
    e = floor.expected_above(h, 20)
    assert abs(e - 0.125) <= 1e-9 * 0.125
    assert abs(floor.score(20, h) - (-math.log10(0.125))) <= 1e-9
    assert abs(floor.score(20, song_hist=h, bin_hist=np.zeros(32, np.uint32)) - floor.score(20, h)) == 0.0
    # the buckets beyond the exact ones take no part in the fit
    h2 = h.copy()
    h2[20] = 7
    assert floor.fit_tail(h2) == floor.fit_tail(h)
    assert floor.tail_counts(h).tolist()[:3] == [65535, 32767, 16383] and floor.tail_counts(h2)[20] == 7


def test_fit_tail_none():
    from shazam_amd import floor
    z = np.zeros(32, np.uint32)
    assert floor.fit_tail(z) is None and floor.expected_above(z, 5) is None and floor.score(5, z) is None
    one = z.copy()
    one[3] = 9
    assert floor.fit_tail(one) is None and floor.score(50, one) is None
    rising = z.copy()
    rising[:4] = [1, 2, 4, 8]
    assert floor.fit_tail(rising) is None
    flat = z.copy()
    flat[:4] = 5
    assert floor.fit_tail(flat) is None
    only_wide = z.copy()
    only_wide[16:20] = [8, 4, 2, 1]
    assert floor.fit_tail(only_wide) is None
    with pytest.raises(ValueError):
        floor.fit_tail(np.zeros(31, np.uint32))
    with pytest.raises(ValueError):
        floor.score(3, z, which="rows")


def test_min_score_filter_on_built_arrays():
    from shazam_amd import floor
    geo = np.zeros(32, np.uint32)
    geo[:16] = [1 << (16 - c) for c in range(1, 17)]       # score(a) = (a - 17) log10 2 + log10(1/2) ... rising with a
    hist = np.stack([geo, geo, np.zeros(32, np.uint32), geo, geo])
    aligned = np.array([[40, 3], [18, 2], [25, 0], [0, 0], [19, 19]], np.uint32)
    nres = np.array([2, 2, 1, 0, 2], np.uint32)
    s40, s18, s19 = (floor.score(a, geo) for a in (40, 18, 19))
    assert s18 < s19 < s40
    keep = floor.keep_windows(nres, aligned, hist, min_score=(s18 + s19) / 2)
    # window 1 falls below; window 2 has nothing to compare against (score None): it counts; window 3 had no result
    assert keep.tolist() == [2, 0, 1, 0, 2]
    assert nres.tolist() == [2, 2, 1, 0, 2]                 # a copy: the input stays
    assert floor.keep_windows(nres, aligned, hist, min_score=-1e9).tolist() == nres.tolist()
    assert floor.keep_windows(nres, aligned, hist, min_score=1e9).tolist() == [0, 0, 1, 0, 0]
