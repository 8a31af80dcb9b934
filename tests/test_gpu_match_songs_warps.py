"""GPU: shz_match_songs_warps -- listed songs warped at a list of (tempo, pitch) pairs on the device and matched against the
rest of the table in one call -- against Table.match (full sort) on the rows tests/rows_warp_twin.py makes of
Table.song_hashes, with topn + 1 and the song itself stripped in numpy.  Every comparison is exact.

The table: eight songs of 300 to 1,200 random rows over a small key space (f in 1000..1015, dt < 32: 8,192 keys, so unrelated
songs share keys at every warp -- the warps below move f by about 8 bins and keep it inside the space), built once as one
segment and once as several, and the plants
  B   the twin's warp_rows(song A, warp 1) under another id: A at warp 1 lists B at delta 0, aligned = A's distinct warped rows;
  C   likewise at warp 2."""
import numpy as np
import pytest

import rows_warp_twin as RT

pytestmark = pytest.mark.gpu

ONE = 65536
TEMPOS = np.array([ONE, 65936, 65200], np.uint32)
PITCHES = np.array([ONE, 65036, 66060], np.uint32)
A, B, C = 3, 9, 10
LISTED = [B, 5, A, 1, 8, C, 2, 12, 7]                       # (12: an id without rows)
FIELDS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")


def make_rows(seed=31):
    rng = np.random.default_rng(seed)
    ks, ss, os_ = [], [], []
    for sid in range(1, 9):
        n = int(rng.integers(300, 1201))
        cell = rng.choice(8192 * 400, n, replace=False)     # distinct (key, offset) pairs
        kid, off = cell // 400, cell % 400
        key = ((1000 + (kid >> 9)) << 20) | ((1000 + ((kid >> 5) & 15)) << 8) | (kid & 31)
        ks.append(key); ss.append(np.full(n, sid)); os_.append(off)
    ak, ao = ks[A - 1], os_[A - 1]
    for sid, v in ((B, 1), (C, 2)):
        wk, wo, _ = RT.warp_rows(ak, ao, int(TEMPOS[v]), int(PITCHES[v]))
        rows = np.unique(np.stack([wk.astype(np.int64), wo.astype(np.int64)], 1), axis=0)
        ks.append(rows[:, 0]); ss.append(np.full(len(rows), sid)); os_.append(rows[:, 1])
    k, s, o = np.concatenate(ks), np.concatenate(ss), np.concatenate(os_)
    p = rng.permutation(len(k))
    return k[p].astype(np.uint32), s[p].astype(np.uint32), o[p].astype(np.uint32)


def build(ctx, k, s, o, parts):
    import shazam_amd as S
    t = S.Table(ctx)
    if parts > 1:
        t.set_segment_rows(max(16, (len(k) + parts - 1) // parts))
    for part in np.array_split(np.arange(len(k)), parts):
        t.insert(k[part], s[part], o[part])
        t.finalize()
    return t


def expected(t, listed, tempos, pitches, topn):
    """Table.match (full sort) on the twin's warped rows of every listed song, topn + 1, the song itself stripped"""
    ro, k, o = t.song_hashes(listed)
    wk, wo, wro = RT.warp_rows_batch(k, o, ro, tempos, pitches)
    w = t.match(wk, wo, wro, topn=topn + 1, full_sort=True)
    n, K = len(listed), len(tempos)
    out = {f: np.zeros((n, K, topn), np.int64) for f in FIELDS[:4]}
    out["nres"] = np.zeros((n, K), np.int64)
    for q, s in enumerate(listed):
        for v in range(K):
            e = q * K + v
            keep = [i for i in range(int(w["nres"][e])) if w["sid"][e, i] != s][:topn]
            for f in FIELDS[:4]:
                out[f][q, v, :len(keep)] = w[f][e, keep]
            out["nres"][q, v] = len(keep)
    out["nhash"] = w["nhash"].astype(np.int64).reshape(n, K)
    out["npairs"] = w["npairs"].astype(np.int64).reshape(n, K)
    out["rows"] = np.diff(ro.astype(np.int64))
    distinct = np.array([len(set(zip(wk[int(wro[e]):int(wro[e + 1])].tolist(), wo[int(wro[e]):int(wro[e + 1])].tolist())))
                         for e in range(n * K)]).reshape(n, K)
    return out, distinct


def compare(got, want, label):
    for f in FIELDS + ("rows",):
        assert np.array_equal(np.asarray(got[f], np.int64), want[f]), f"{label}: {f}\n{got[f]}\n{want[f]}"


@pytest.fixture(scope="module", params=(1, 4), ids=("one_segment", "segments"))
def case(request):
    import shazam_amd as S
    ctx = S.get_context(0)
    t = build(ctx, *make_rows(), request.param)
    assert (t.segments() == 1) == (request.param == 1)
    yield ctx, t
    t.close()


def test_the_identity_warp_alone_is_match_songs(case):
    ctx, t = case
    for topn in (1, 5):
        plain = t.match_songs(LISTED, topn=topn)
        got = t.match_songs_warps(LISTED, [ONE], [ONE], topn=topn)
        for f in FIELDS:
            assert got[f].shape == (len(LISTED), 1) + plain[f].shape[1:] and got[f].dtype == plain[f].dtype
            assert np.array_equal(got[f][:, 0], plain[f]), f
        assert np.array_equal(got["rows"], plain["rows"]) and plain["nres"].any()


def test_every_song_and_warp_equals_the_match_of_the_twins_rows(case):
    ctx, t = case
    topn = 5
    want, distinct = expected(t, LISTED, TEMPOS, PITCHES, topn)
    assert want["nres"][:, 1:].any() and (want["aligned"][:, 1:, 1] > 0).any()      # unrelated songs meet at the warps too
    got = t.match_songs_warps(LISTED, TEMPOS, PITCHES, topn=topn)
    compare(got, want, "top5")
    compare(t.match_songs_warps(LISTED, TEMPOS, PITCHES, topn=topn, full_sort=True), want, "top5 full_sort")
    assert np.array_equal(got["nhash"], distinct)
    # the plants: A at warp v lists its twin-warped copy first, at delta 0, with every distinct warped row aligned
    qa = LISTED.index(A)
    for sid, v in ((B, 1), (C, 2)):
        assert got["sid"][qa, v, 0] == sid and got["delta"][qa, v, 0] == 0
        assert got["aligned"][qa, v, 0] == distinct[qa, v] > 250
        assert got["aligned"][qa, 0, 0] < 50                                         # the plain match does not see it
    assert got["rows"][LISTED.index(12)] == 0 and not got["nres"][LISTED.index(12)].any()
    # the public form names the pairs; a speed ladder is the diagonal
    import shazam_amd as S
    pub = S.match_songs(t, LISTED, topn=topn, warps=(TEMPOS, PITCHES))
    compare(pub, want, "S.match_songs")
    assert np.array_equal(pub["tempo_q16"], TEMPOS) and np.array_equal(pub["pitch_q16"], PITCHES)
    sp = S.match_songs(t, [A, 5], topn=2, speeds=np.array([ONE, 65936], np.uint32))
    compare(sp, expected(t, [A, 5], [ONE, 65936], [ONE, 65936], 2)[0], "speeds=")


@pytest.mark.parametrize("topn", (1, 63))
def test_results_do_not_depend_on_the_slicing(case, topn):
    from shazam_amd import _ffi
    ctx, t = case
    whole = t.match_songs_warps(LISTED, TEMPOS, PITCHES, topn=topn)
    compare(whole, expected(t, LISTED, TEMPOS, PITCHES, topn)[0], f"top{topn}")
    ctx.set_debug(_ffi.DEBUG_CATALOG_SMALL_SLICES)
    try:
        small = t.match_songs_warps(LISTED, TEMPOS, PITCHES, topn=topn)
    finally:
        ctx.set_debug(0)
    for f in FIELDS + ("rows",):
        assert np.array_equal(small[f], whole[f]), f
    # the same songs in two calls, and the timings do not change the arrays
    two = [t.match_songs_warps(LISTED[:4], TEMPOS, PITCHES, topn=topn), t.match_songs_warps(LISTED[4:], TEMPOS, PITCHES, topn=topn)]
    for f in FIELDS + ("rows",):
        assert np.array_equal(np.concatenate([r[f] for r in two]), whole[f]), f
    timed = t.match_songs_warps(LISTED, TEMPOS, PITCHES, topn=topn, timings=True)
    assert all(np.array_equal(timed[f], whole[f]) for f in FIELDS) and len(timed["ms"]) == 3 and min(timed["ms"]) > 0


def test_refusals(case):
    import shazam_amd as S
    from shazam_amd import _ffi
    ctx, t = case
    with pytest.raises(S.ShzError) as e:
        t.match_songs_warps([A, 5, A], TEMPOS, PITCHES)
    assert e.value.code == _ffi.E_INVALID and "twice" in str(e.value)
    with pytest.raises(S.ShzError) as e:
        t.match_songs_warps(LISTED, [ONE, 131073], [ONE, ONE])
    assert e.value.code == _ffi.E_INVALID and "tempo 1" in str(e.value)
    with pytest.raises(S.ShzError) as e:
        t.match_songs_warps(LISTED, [ONE, ONE], [32767, ONE])
    assert e.value.code == _ffi.E_INVALID and "pitch 0" in str(e.value)
    with pytest.raises(S.ShzError) as e:
        t.match_songs_warps(LISTED, [], [])
    assert e.value.code == _ffi.E_INVALID and "n_warps" in str(e.value)
    for topn in (0, 64):
        with pytest.raises(S.ShzError) as e:
            t.match_songs_warps(LISTED, TEMPOS, PITCHES, topn=topn)
        assert e.value.code == _ffi.E_INVALID and "topn" in str(e.value)
    res = t.match_songs_warps(np.zeros(0, np.uint32), TEMPOS, PITCHES)
    assert res["sid"].shape == (0, 3, 5) and len(res["rows"]) == 0
    res = t.match_songs_warps([12, 1000], TEMPOS, PITCHES, topn=2)                   # no listed song has a row
    assert not res["nres"].any() and not res["rows"].any() and not res["sid"].any()


def test_a_warped_offset_that_reaches_2_pow_20_is_refused():
    """a listed song's WARPED offsets are query offsets: offset 600,000 stays below 2^20 at 1.0 and 1.5 and passes it at 2.0"""
    import shazam_amd as S
    from shazam_amd import _ffi
    ctx = S.get_context(0)
    k, s, o = make_rows(seed=4)
    k, s, o = np.append(k, np.uint32(1000 << 20 | 1000 << 8 | 3)), np.append(s, np.uint32(5)), np.append(o, np.uint32(600000))
    t = build(ctx, k, s, o, 1)
    try:
        ok = [ONE, 98304]
        compare(t.match_songs_warps([5, 2], ok, ok, topn=2), expected(t, [5, 2], ok, ok, 2)[0], "below 2^20")
        with pytest.raises(S.ShzError) as e:
            t.match_songs_warps([5, 2], [ONE, 131072], [ONE, ONE], topn=2)
        assert e.value.code == _ffi.E_UNSUPPORTED and "600000" in str(e.value) and "131072" in str(e.value)
        compare(t.match_songs_warps([2, 7], [ONE, 131072], [ONE, ONE], topn=2), expected(t, [2, 7], [ONE, 131072], [ONE, ONE], 2)[0],
                "beside the long song")
    finally:
        t.close()
