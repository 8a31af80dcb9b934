"""GPU: Table.match_songs_warps_extents (shz_match_songs_warps_extents) -- songs of the table warped on the device by the JOB
FORM of the row warp, one (song, t16, f16) a job, and handed to the extent pass with the moments -- against the plain-Python
definition (tests/rows_fit_twin.py) on Table.export().  Every comparison is exact, under the debug flags 0,
EXTENT_SMALL_TILES, CATALOG_SMALL_SLICES (a slice holds at most 2 jobs) and both.

The built table (a few thousand rows): song 1 (400 rows, frames 0 .. 299) and song 2, which holds the images under (67502,
65536) of song 1's rows of the frames LO .. HI shifted by DELTA; songs 11 .. 17 of 1, 63, 64, 65, 511, 512 and 513 rows (song
10 has none) -- they reach wave and RW_ITEMS block borders, and listed one behind the other they make waves that straddle
two and three jobs; song 30, which holds their images under WARP shifted by SHIFT; song 20, all frequencies above 1024 (at
f16 = 32768 every row leaves); song 21, rows with dt > 100 (at t16 = 131072 they leave by dt' > 200) beside rows that stay;
song 22, two rows that meet in one (key, t1') at t16 = 32768, and song 40, which holds that one image."""
import numpy as np
import pytest

from fit_twin import expected_moments, own_frames, warp_map
from rows_fit_twin import FIELDS, assert_same, match_songs_warps_extents as twin
from rows_warp_twin import warp_rows

pytestmark = pytest.mark.gpu

ONE = 65536
DELTA, LO, HI = 37, 120, 219
PLANT = (67502, ONE)
WARP, SHIFT = (66000, 65000), 50
SIZES = {11: 1, 12: 63, 13: 64, 14: 65, 15: 511, 16: 512, 17: 513}
MEET_KEY, MEET_SHIFT = (700 << 20) | (900 << 8) | 4, 11


def _rows(rng, n, f_lo=0, f_hi=2048, off_hi=300, dt_lo=1, dt_hi=100):
    """n distinct rows (key32 = f1 << 20 | f2 << 8 | dt, off)"""
    seen, ks, os_ = set(), [], []
    while len(ks) < n:
        f1, f2 = int(rng.integers(f_lo, f_hi + 1)), int(rng.integers(f_lo, f_hi + 1))
        k, o = (f1 << 20) | (f2 << 8) | int(rng.integers(dt_lo, dt_hi + 1)), int(rng.integers(0, off_hi))
        if (k, o) not in seen:
            seen.add((k, o))
            ks.append(k)
            os_.append(o)
    return np.asarray(ks, np.uint32), np.asarray(os_, np.uint32)


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def built(S, ctx):
    rng = np.random.default_rng(2024)
    t = S.Table(ctx)
    ka, oa = _rows(rng, 400)
    oa[:4] = (LO, HI, LO - 1, HI + 1)            # both ends of the stretch are occupied, and their neighbours outside it
    t.insert(ka, 1, oa)
    ins = (oa >= LO) & (oa <= HI)
    wk, wo, keep = warp_rows(ka[ins], oa[ins], *PLANT)
    assert keep.all()
    kb, ob = _rows(rng, 250, off_hi=600)
    t.insert(np.concatenate([wk, kb]), 2, np.concatenate([wo + DELTA, ob]))
    kc, oc = _rows(rng, 300)
    t.insert(kc, 3, oc)
    img_k, img_o = [], []
    for sid, n in SIZES.items():
        k, o = _rows(rng, n)
        t.insert(k, sid, o)
        wk, wo, _ = warp_rows(k, o, *WARP)
        img_k.append(wk)
        img_o.append(wo + SHIFT)
    t.insert(np.concatenate(img_k), 30, np.concatenate(img_o))
    kh, oh = _rows(rng, 100, f_lo=1100)
    t.insert(kh, 20, oh)
    k1, o1 = _rows(rng, 80, dt_lo=101, dt_hi=200)
    k2, o2 = _rows(rng, 40)
    t.insert(np.concatenate([k1, k2]), 21, np.concatenate([o1, o2]))
    k3, o3 = _rows(rng, 30)
    t.insert(np.concatenate([np.asarray([MEET_KEY, MEET_KEY], np.uint32), k3]), 22, np.concatenate([np.asarray([9, 10], np.uint32), o3]))
    mk, mo, _ = warp_rows([MEET_KEY], [9], 32768, ONE)
    t.insert(mk, 40, mo + MEET_SHIFT)
    t.finalize()
    yield t, t.export()
    t.close()


def _flags():
    from shazam_amd import _ffi
    return (0, _ffi.DEBUG_EXTENT_SMALL_TILES, _ffi.DEBUG_CATALOG_SMALL_SLICES, _ffi.DEBUG_EXTENT_SMALL_TILES | _ffi.DEBUG_CATALOG_SMALL_SLICES)


def _check(ctx, built, jobs, cs, lo, hi, cn=None, what="", hist=True):
    """the library under every debug flag against the twin (computed once); returns the library's dict"""
    t, (tk, ts, to) = built
    sid, t16, f16 = ([j[i] for j in jobs] for i in range(3))
    want = twin(tk, ts, to, sid, t16, f16, cs, lo, hi, cn, hist=hist)
    out = None
    for flag in _flags():
        ctx.set_debug(flag)
        try:
            out = t.match_songs_warps_extents(sid, t16, f16, np.asarray(cs, np.uint32), np.asarray(lo, np.int32), np.asarray(hi, np.int32),
                                              cand_n=cn, hist=hist)
        finally:
            ctx.set_debug(0)
        assert_same(out, want, (what, flag), hist=hist)
    return out


# one song in three jobs at three warps, listed between jobs of other songs; 1-, 1- and 63-row jobs share the first wave
JOBS = [(11, *WARP), (11, ONE, ONE), (12, *WARP), (10, ONE, ONE), (13, *WARP), (14, *WARP), (1, *PLANT), (15, *WARP), (1, 70000, 64000),
        (16, *WARP), (1, 60000, ONE), (17, *WARP), (20, ONE, 32768), (21, 131072, ONE), (22, 32768, ONE)]


def test_sizes_at_every_border_one_candidate(ctx, built):
    n = len(JOBS)
    r = _check(ctx, built, JOBS, [[30]] * n, [[SHIFT]] * n, [[SHIFT]] * n, what="ncand 1")
    t, (tk, ts, to) = built
    assert {s: int((ts == s).sum()) for s in SIZES} == SIZES
    for j, (sid, t16, f16) in enumerate(JOBS):
        if sid in SIZES and (t16, f16) == WARP:                             # every kept row has its image in song 30
            wk, wo, _ = warp_rows(tk[ts == sid], to[ts == sid], *WARP)
            assert int(r["kept"][j]) == len(wk) and int(r["count"][j, 0]) >= len(set(zip(wk.tolist(), wo.tolist())))
    assert int(r["count"][:, 0].sum()) > 1500
    assert int(r["kept"][3]) == 0 and int(r["shift"][3]) == 0                                       # the song without rows
    assert not any(int(r[f][3, 0]) for f in FIELDS if f not in ("kept", "shift"))


def test_three_candidates_and_slots_past_cand_n(ctx, built):
    n = len(JOBS)
    cs = [[30, 2, 30]] * n
    lo = [[SHIFT - 10, DELTA - 5, -300]] * n
    hi = [[SHIFT + 10, DELTA + 5, 600]] * n
    cn = [(j % 3) + 1 for j in range(n)]
    r = _check(ctx, built, JOBS, cs, lo, hi, cn, "ncand 3")
    assert int(r["count"][:, 2].sum()) > 0 and all(int(r["count"][j, 2]) == 0 for j in range(n) if cn[j] < 3)


def test_rows_that_leave_and_rows_that_meet(ctx, built):
    t, (tk, ts, to) = built
    jobs = [(20, ONE, 32768), (21, 131072, ONE), (22, 32768, ONE)]
    r = _check(ctx, built, jobs, [[20, 20], [21, 3], [40, 22]], [[-600, 0]] * 3, [[600, 3000]] * 3,
               what="leave / meet")
    assert int(r["kept"][0]) == 0 and not r["count"][0].any() and int(r["shift"][0]) == 0     # every frequency leaves: an empty query
    assert int(r["kept"][1]) == int(((tk[ts == 21] & 0xFF) <= 100).sum()) == 40                 # dt' = 2 dt > 200 leaves
    k22, o22 = tk[ts == 22], to[ts == 22]
    wk, wo, keep = warp_rows(k22, o22, 32768, ONE)
    assert keep.all() and int(r["kept"][2]) == len(k22)                                         # kept counts both rows that meet ...
    assert len(set(zip(wk.tolist(), wo.tolist()))) < len(k22)
    one = t.match_songs_warps_extents([22], [32768], [ONE], [[40]], [[MEET_SHIFT]], [[MEET_SHIFT]])
    assert int(one["count"][0, 0]) == 1 and int(one["kept"][0]) == len(k22)                     # ... the extent pass counts the set


def test_the_planted_stretch_in_warped_and_in_own_frames(ctx, built):
    r = _check(ctx, built, [(1, *PLANT)], [[2]], [[DELTA]], [[DELTA]], what="planted")
    assert (int(r["q_first"][0, 0]), int(r["q_last"][0, 0])) == (warp_map(LO, PLANT[0]), warp_map(HI, PLANT[0]))
    assert (int(r["t_first"][0, 0]), int(r["t_last"][0, 0])) == (warp_map(LO, PLANT[0]) + DELTA, warp_map(HI, PLANT[0]) + DELTA)
    from shazam_amd.extent import own_frames as lib_own
    assert lib_own(int(r["q_first"][0, 0]), int(r["q_last"][0, 0]), PLANT[0]) == (LO, HI) == own_frames(int(r["q_first"][0, 0]), int(r["q_last"][0, 0]), PLANT[0])
    # a widened candidate, d_hi - d_lo = 4095, is accepted
    _check(ctx, built, [(1, *PLANT), (1, ONE, ONE)], [[2], [2]], [[DELTA - 2000]] * 2, [[DELTA + 2095]] * 2, what="4095 wide", hist=False)


def test_identity_jobs_equal_the_catalogue_form_and_the_fit_on_gathered_rows(ctx, built):
    t, (tk, ts, to) = built
    sids = [15, 1, 10, 2, 3, 11]
    cs = [[30, 2], [2, 3], [1, 1], [1, 30], [3, 1], [30, 11]]
    lo = [[0, -50], [-40, -600], [0, 0], [-600, -600], [0, -600], [-100, 0]]
    hi = [[100, 50], [40, 600], [0, 0], [600, 600], [0, 600], [100, 0]]
    ro, qk, qo = t.song_hashes(sids)
    for flag in _flags():
        ctx.set_debug(flag)
        try:
            got = t.match_songs_warps_extents(sids, [ONE] * len(sids), [ONE] * len(sids), cs, lo, hi, hist=True)
            cat = t.match_songs_extents(sids, cs, lo, hi)
            fit = t.match_extents(qk, qo, ro, cs, lo, hi, fit=True)
        finally:
            ctx.set_debug(0)
        for f in ("count", "q_first", "q_last", "t_first", "t_last", "hist", "shift"):
            assert np.array_equal(got[f], cat[f]), (flag, f)
        for f in ("sum_q", "sum_u", "sum_qq", "sum_qu", "count", "shift"):
            assert np.array_equal(got[f], fit[f]), (flag, f)
        assert got["kept"].tolist() == np.diff(ro.astype(np.int64)).tolist()
    assert int(got["count"][4, 0]) == int((ts == 3).sum())                  # a song against itself at delta 0: its rows
    want = expected_moments(tk, ts, to, qk, qo, ro, cs, lo, hi)
    assert [int(x) for x in got["sum_qu"][1]] == [w["sum_qu"] for w in want[1]]


def _raw(ctx, t, sid, t16, f16, n_jobs, ncand, cs, lo, hi, cn, drop=(), kept=True):
    """the entry point as it is, on outputs filled with a pattern: (status, outputs untouched?)"""
    from shazam_amd import _ffi
    L, p = _ffi.lib(), _ffi.ptr
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint32)   # noqa: E731
    sid, t16, f16, cs, cn = u32(sid), u32(t16), u32(f16), u32(cs), u32(cn)
    lo, hi = np.ascontiguousarray(lo, np.int32), np.ascontiguousarray(hi, np.int32)
    cells = max(n_jobs * ncand, 1)
    o32 = {f: np.full(cells * (64 if f == "hist" else 1), 0xABABABAB, np.uint32) for f in ("count", "q_first", "q_last", "t_first", "t_last", "hist", "shift")}
    o64 = {f: np.full(cells, 0xCDCDCDCDCDCDCDCD, np.uint64) for f in ("sum_q", "sum_u", "sum_qq", "sum_qu", "kept")}
    args32 = [None if f in drop else p(o32[f]) for f in o32]
    args64 = [None if f in drop or (f == "kept" and not kept) else p(o64[f]) for f in o64]
    as_u32p = lambda a: None if a is None else a.ctypes.data_as(_ffi.u32p)      # noqa: E731
    rc = L.shz_match_songs_warps_extents(ctx.h, t.h, as_u32p(sid), as_u32p(t16), as_u32p(f16), n_jobs, ncand, p(cs), p(lo), p(hi), p(cn),
                                         *args32, *args64, None, None, None)
    clean = all((a == 0xABABABAB).all() for a in o32.values()) and all((a == 0xCDCDCDCDCDCDCDCD).all() for a in o64.values())
    return rc, clean


def test_refusals_leave_the_outputs_untouched(S, ctx, built):
    from shazam_amd import _ffi
    t, _ = built
    ok = dict(sid=[1, 2], t16=[ONE, 70000], f16=[ONE, ONE], n_jobs=2, ncand=1, cs=[2, 1], lo=[0, 0], hi=[5, 5], cn=[1, 1])

    def raw(**k):
        return _raw(ctx, t, **{**ok, **k})

    rc, clean = raw()
    assert rc == _ffi.OK and not clean                                                       # (the call as it is runs)
    assert raw(kept=False)[0] == _ffi.OK and raw(drop=("hist",))[0] == _ffi.OK               # out_kept and out_hist may be NULL
    assert raw(n_jobs=0) == (_ffi.OK, True)                                                  # nothing is written
    assert raw(n_jobs=0, sid=None, t16=None, f16=None) == (_ffi.OK, True)
    for bad in (dict(t16=[ONE, 32767]), dict(t16=[131073, ONE]), dict(f16=[32767, ONE]), dict(f16=[ONE, 131073]),   # a factor out of range
                dict(sid=None), dict(t16=None), dict(f16=None),                                                      # a NULL job array
                dict(ncand=0), dict(ncand=65, cs=[2] * 130, lo=[0] * 130, hi=[0] * 130),                             # ncand outside [1, 64]
                dict(lo=[6, 0]), dict(cn=[1, 2]),                                                                    # d_lo > d_hi; cand_n above ncand
                dict(drop=("count",)), dict(drop=("shift",)), dict(drop=("sum_qq",)), dict(cn=None), dict(cs=None)):  # NULL arrays
        assert raw(**bad) == (_ffi.E_INVALID, True), bad
    assert raw(lo=[0, -96], hi=[5, 4000]) == (_ffi.E_UNSUPPORTED, True)                      # a used candidate 4,096 bins wide
    assert raw(lo=[0, -95], hi=[5, 4000])[0] == _ffi.OK                                      # 4,095: accepted
    # the state of the table; a warped offset that reaches 2^20: offset 600,000 at t16 = 131072
    u = S.Table(ctx)
    u.insert(np.asarray([(5 << 20) | (6 << 8) | 6, (7 << 20) | (8 << 8) | 2], np.uint32), 1, np.asarray([5, 600000], np.uint32))
    u.insert(np.asarray([(5 << 20) | (6 << 8) | 3], np.uint32), 2, np.asarray([9], np.uint32))
    far = dict(sid=[2, 1], t16=[131072, 131072], f16=[ONE, ONE], n_jobs=2, ncand=1, cs=[1, 2], lo=[-20, 0], hi=[20, 0], cn=[1, 1])
    assert _raw(ctx, u, **far) == (_ffi.E_STATE, True)
    u.finalize()
    assert _raw(ctx, u, **far) == (_ffi.E_UNSUPPORTED, True)
    with pytest.raises(_ffi.ShzError) as e:
        u.match_songs_warps_extents([1], [131072], [ONE], [[2]], [[0]], [[0]])
    assert e.value.code == _ffi.E_UNSUPPORTED and "600000" in str(e.value) and "131072" in str(e.value)
    r = u.match_songs_warps_extents([2, 1], [131072, ONE], [ONE, ONE], [[1], [2]], [[-20], [0]], [[20], [4]])   # (at 1.0 the offset is fine)
    assert (int(r["count"][0, 0]), int(r["q_first"][0, 0]), int(r["t_first"][0, 0])) == (1, 18, 5)                # offset 9 -> 18, dt 3 -> 6
    u.close()
