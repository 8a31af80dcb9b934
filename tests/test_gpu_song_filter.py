"""GPU: the song filter (Context.songs, Table.match(songs= / exclude= / song_sets=)) on tables and queries built by hand,
against its plain-Python definition (tests/song_filter_twin.py): a filtered match gives the arrays of the plain match on a
table of the allowed songs' rows.  Bitmap edges, vote counts at every border of the two filter kernels, query and sub-batch
borders, per-query sets, the case the feature exists for, the sub-table definition on a second table, and the state of the
setting.  Every case runs with and without SHZ_DEBUG_FILTER_SMALL, at delta_tol 0 and 2, with floor=True as well, and through
match and match_device.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from song_filter_twin import allowed_rows, expected_floor_sets, expected_match_sets
from test_gpu_vote_floor import ARRAYS, Built, _hist_eq, _same
from vote_tol_twin import assert_match

pytestmark = pytest.mark.gpu

SMALL = 2048   # SHZ_DEBUG_FILTER_SMALL


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _check(S, ctx, b, sets, set_of=None, exclude=False, tols=(0, 2), topn=3, debugs=(0, SMALL), what="", t=None):
    """match(floor=True) under the filter against the twin at every tolerance and debug setting; match without the floor,
    match_device with and without it against that result; the context is as it was afterwards.  sets: one list of ids (with
    set_of None: songs= / exclude=) or a list of lists with set_of (song_sets=)."""
    tk, ts, to, qk, qo, qoff = b.arrays() if isinstance(b, Built) else b
    own = t is None
    if own:
        t = S.Table(ctx)
        t.insert(tk, ts, to)
        t.finalize()
    if set_of is None:
        kw = dict(exclude=sets) if exclude else dict(songs=sets)
        tw = dict(sets=[sets], set_of=None, exclude=exclude)
    else:
        kw = dict(song_sets=sets, set_of=set_of, exclude=bool(exclude))
        tw = dict(sets=sets, set_of=set_of, exclude=exclude)
    out = {}
    try:
        for tol in tols:
            want = expected_match_sets(tk, ts, to, qk, qo, qoff, tol, topn, **tw)
            wantf = expected_floor_sets(tk, ts, to, qk, qo, qoff, tol, **tw)
            for dbg in debugs:
                ctx.set_debug(dbg)
                try:
                    res = t.match(qk, qo, qoff, topn, delta_tol=tol, floor=True, **kw)
                    plain = t.match(qk, qo, qoff, topn, delta_tol=tol, **kw)
                    dev = t.match_device(qk, qo, qoff, topn, delta_tol=tol, floor=True, **kw)
                    devb = t.match_device(qk, qo, qoff, topn, delta_tol=tol, bias_bound=int(qo.max()) if len(qo) else 0, **kw)
                finally:
                    ctx.set_debug(0)
                assert_match(res, want, (what, tol, dbg))
                _hist_eq(res, wantf, (what, tol, dbg))
                _same(plain, res, (what, "no floor", tol, dbg))
                _same(dev, res, (what, "device", tol, dbg))
                _hist_eq(dev, wantf, (what, "device", tol, dbg))
                _same(devb, res, (what, "device, bound", tol, dbg))
                assert ctx.song_filter is None and not ctx.vote_floor and ctx.vote_tolerance == 0 and ctx.floor_rows() == 0
                out[tol] = res
    finally:
        if own:
            t.close()
    return out


# ---- 1. bitmap edges -----------------------------------------------------------------------------------------------------
def _edge_table():
    """songs 0, 31, 32, 63, 64, 100 (the largest) and a few between, a few bins each, one query"""
    b = Built()
    for i, sid in enumerate((0, 1, 31, 32, 33, 63, 64, 65, 99, 100)):
        b.bins(0, sid, {3 * i - 9: 2 + i % 3, 3 * i - 8: 1})
    b.miss(0, 2)
    return b


@pytest.mark.parametrize("sid", [0, 31, 32, 63, 64, 100])
def test_bitmap_edges_one_song_alone_in_and_out(S, ctx, sid):
    b = _edge_table()
    r = _check(S, ctx, b, [sid], what=("alone in", sid))
    assert int(r[0]["nres"][0]) == 1 and int(r[0]["sid"][0, 0]) == sid
    r = _check(S, ctx, b, [sid], exclude=True, topn=12, what=("alone out", sid))
    assert int(r[0]["nres"][0]) == 9 and sid not in r[0]["sid"][0, :9].tolist()


def test_bitmap_edges_ids_beyond_table_and_bitmap_empty_and_full(S, ctx):
    b = _edge_table()
    every = [0, 1, 31, 32, 33, 63, 64, 65, 99, 100]
    r = _check(S, ctx, b, [64, 5000, 1 << 31], what="listed above the table's largest")
    assert r[0]["sid"][0, :int(r[0]["nres"][0])].tolist() == [64]
    # the bitmap ends with the word of id 40 (ids 32 .. 63): the table's songs 64 .. 100 lie above it -- barred under allow,
    # kept under exclude
    r = _check(S, ctx, b, [1, 40], topn=12, what="table above the bitmap, allow")
    assert r[0]["sid"][0, :int(r[0]["nres"][0])].tolist() == [1]
    r = _check(S, ctx, b, [1, 40], exclude=True, topn=12, what="table above the bitmap, exclude")
    assert sorted(r[0]["sid"][0, :int(r[0]["nres"][0])].tolist()) == [s for s in every if s != 1]
    r = _check(S, ctx, b, [], what="empty, allow")
    assert int(r[0]["nres"][0]) == 0 and int(r[0]["npairs"][0]) == 0 and int(r[0]["nhash"][0]) > 0
    r = _check(S, ctx, b, [], exclude=True, topn=12, what="empty, exclude")
    full = _check(S, ctx, b, every[::-1] + every, topn=12, what="every song, repeated and unordered")
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    plain = t.match(qk, qo, qoff, 12, delta_tol=2)
    t.close()
    _same(r[2], plain, "exclude nothing")
    _same(full[2], plain, "allow everything")


# ---- 2. vote counts of one query at the kernels' borders -------------------------------------------------------------------
def _masked(mask):
    """one query, one vote per entry of mask in key order: a kept vote belongs to song 1, a dropped one to song 2; the offset
    differences walk over 5 bins so that the runs and the bins hold several votes"""
    b = Built(q_base=8)
    for i, keep in enumerate(mask):
        b.vote(0, 1 if keep else 2, (i % 5) - 2)
    return b


def _pattern(n, way):
    i = np.arange(n)
    return {"first": i < (n + 1) // 2, "last": i >= n // 2, "alternating": i % 2 == 0}[way]


@pytest.mark.parametrize("way", ["first", "last", "alternating"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_vote_counts_at_the_borders(S, ctx, n, way):
    mask = _pattern(n, way)
    r = _check(S, ctx, _masked(mask), [1], what=(n, way))
    assert int(r[0]["npairs"][0]) == int(mask.sum()) and int(r[0]["nhash"][0]) == n


@pytest.mark.parametrize("way", ["first", "last", "alternating"])
def test_seventy_thousand_votes(S, ctx, way):
    mask = _pattern(70000, way)
    r = _check(S, ctx, _masked(mask), [1], tols=(0,), what=(70000, way))
    assert int(r[0]["npairs"][0]) == 35000
    r = _check(S, ctx, _masked(mask), [2], tols=(2,), debugs=(0,), what=(70000, way, "the other half"))
    assert int(r[2]["npairs"][0]) == 35000


@pytest.mark.parametrize("n,block,debugs", [(129, 64, (SMALL,)), (4097, 2048, (0,)), (4097, 512, (0,)), (129, 16, (SMALL,))])
def test_first_or_last_vote_of_a_block_alone(S, ctx, n, block, debugs):
    """the only kept vote, and the only dropped one, at the first and last place of a block (and of a wave's quarter of it)"""
    for at in (0, block - 1, block, 2 * block - 1, 2 * block, n - 1):
        for only_kept in (True, False):
            mask = np.zeros(n, bool) if only_kept else np.ones(n, bool)
            mask[at] = only_kept
            r = _check(S, ctx, _masked(mask), [1], tols=(0,), debugs=debugs, what=(n, at, only_kept))
            assert int(r[0]["npairs"][0]) == int(mask.sum())


# ---- 3. queries ------------------------------------------------------------------------------------------------------------
def _queries(nq, seed):
    """nq queries over 12 songs: query 1 votes for barred songs only (under the set below), query 2 for allowed ones only, query
    3 has no hashes, query 4 hashes that match nothing, query 5 about 300 votes over several blocks of 64; the others a
    few random votes"""
    rng = np.random.default_rng(seed)
    b = Built(n_queries=nq)
    for q in range(nq):
        if q == 1:
            for s in (7, 9, 11):
                b.bins(q, s, {1: 3, 2: 2})
        elif q == 2:
            for s in (2, 4, 6):
                b.bins(q, s, {-1: 2, 0: 4, 4: 1})
        elif q == 3:
            continue
        elif q == 4:
            b.miss(q, 4)
        elif q == 5:
            for i in range(300):
                b.vote(q, int(rng.integers(0, 12)), int(rng.integers(-4, 5)))
        else:
            for _ in range(int(rng.integers(2, 7))):
                b.vote(q, int(rng.integers(0, 12)), int(rng.integers(-3, 4)), int(rng.integers(1, 4)))
            b.miss(q)
    return b


ALLOWED = [0, 2, 4, 6, 8, 10]


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 7])
def test_queries_and_sub_batch_borders(S, ctx, nq):
    b = _queries(nq, 40 + nq)
    r = _check(S, ctx, b, ALLOWED, what=("queries", nq))
    _check(S, ctx, b, ALLOWED, exclude=True, what=("queries, exclude", nq))
    res = r[0]
    if nq > 2:
        assert int(res["npairs"][1]) == 0 and int(res["nres"][1]) == 0 and int(res["nhash"][1]) == 15     # all votes go
        assert int(res["npairs"][2]) == 21 and int(res["nres"][2]) == 3                                    # all votes stay
    if nq > 4:
        assert int(res["nhash"][3]) == 0 and int(res["nhash"][4]) == 4 and int(res["npairs"][4]) == 0


def test_single_query_takes_the_kept_total(S, ctx):
    """one query: npairs is the kept total, not the probed pairs; match_stats keeps counting the probed ones"""
    b = Built()
    b.bins(0, 3, {0: 5, 1: 2})
    b.bins(0, 4, {2: 9})
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        res = t.match(qk, qo, qoff, 2, songs=[3])
        assert int(res["npairs"][0]) == 7 and res["sid"][0].tolist() == [3, 0] and int(res["aligned"][0, 0]) == 5
        assert t.match_stats()["pairs"] == 16
        assert int(t.match(qk, qo, qoff, 2)["npairs"][0]) == 16
    finally:
        t.close()


def test_per_query_sets(S, ctx):
    """neighbouring queries with different sets, two queries sharing one, under both modes"""
    b = _queries(7, 91)
    sets = [ALLOWED, [7, 9, 11, 200], [], list(range(12))]
    set_of = [0, 1, 3, 2, 1, 0, 3]
    r = _check(S, ctx, b, sets, set_of, what="sets")
    assert int(r[0]["npairs"][1]) == 15 and int(r[0]["npairs"][2]) == 21
    _check(S, ctx, b, sets, set_of, exclude=True, what="sets, exclude")
    # one set through song_sets= is songs=
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        _same(t.match(qk, qo, qoff, 3, song_sets=[ALLOWED], set_of=[0] * 7), t.match(qk, qo, qoff, 3, songs=ALLOWED), "one set")
    finally:
        t.close()


def test_out_of_range_set_is_refused(S, ctx):
    from shazam_amd import _ffi
    b = _queries(4, 92)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        before = t.match(qk, qo, qoff, 3)
        stats = t.match_stats()
        for call in (t.match, t.match_device):
            with pytest.raises(_ffi.ShzError) as e:
                call(qk, qo, qoff, 3, song_sets=[[1], [2]], set_of=[0, 1, 2, 0])
            assert e.value.code == _ffi.E_INVALID and ctx.song_filter is None
        assert t.match_stats() == stats                                  # nothing ran
        with pytest.raises(ValueError):
            t.match(qk, qo, qoff, 3, song_sets=[[1]], set_of=[0, 0])    # one entry per query
        with pytest.raises(ValueError):
            t.match(qk, qo, qoff, 3, song_sets=[[1]])
        res = _ffi._match_result(4, 3)
        m = np.zeros(4, np.uint32)
        args = (ctx.h, t.h, _ffi.ptr(qk), _ffi.ptr(qo), qoff.ctypes.data_as(_ffi.u64p), 4, 3, 0, *(_ffi.ptr(res[k]) for k in ARRAYS))
        assert _ffi.lib().shz_match_batch_sets(*args, _ffi.ptr(m)) == _ffi.E_STATE     # no filter set
        with ctx.songs(only=[1]):
            assert _ffi.lib().shz_match_batch_sets(*args, None) == _ffi.E_INVALID
        _same(t.match(qk, qo, qoff, 3), before, "after the refusals")
    finally:
        t.close()


# ---- 4. the reason for the feature -----------------------------------------------------------------------------------------
def test_allowed_song_third_overall_comes_first(S, ctx):
    b = Built()
    b.bins(0, 5, {0: 30, 1: 3})
    b.bins(0, 6, {4: 20})
    b.bins(0, 7, {-2: 10, 9: 4})      # the operator's song: third
    b.bins(0, 8, {3: 2})
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        plain = t.match(qk, qo, qoff, 2)
        assert plain["sid"][0].tolist() == [5, 6]                       # a larger-topn-and-discard caller never sees song 7
        res = t.match(qk, qo, qoff, 2, songs=[7, 8])
        assert res["sid"][0].tolist() == [7, 8] and res["aligned"][0].tolist() == [10, 2] and int(res["delta"][0, 0]) == -2
        assert int(res["npairs"][0]) == 16 and int(plain["npairs"][0]) == 69
        res = t.match(qk, qo, qoff, 2, exclude=[5, 6])
        assert res["sid"][0].tolist() == [7, 8]
    finally:
        t.close()


# ---- 5. the sub-table definition ---------------------------------------------------------------------------------------------
def test_filtered_match_is_the_plain_match_on_the_sub_table(S, ctx):
    rng = np.random.default_rng(2024)
    keys = rng.choice(1 << 31, 48, replace=False).astype(np.uint32)
    n_rows, nq = 3000, 9
    t = S.Table(ctx)
    t.insert(keys[rng.integers(0, 48, n_rows)], rng.integers(1, 41, n_rows).astype(np.uint32), rng.integers(0, 200, n_rows).astype(np.uint32))
    t.finalize()
    qk = keys[rng.integers(0, 48, 40 * nq)]
    qo = rng.integers(0, 64, 40 * nq).astype(np.uint32)
    qoff = (np.arange(nq + 1) * 40).astype(np.uint64)
    tk, ts, to = t.export()
    try:
        for ids in ([3], [40, 1, 17, 22, 22, 5], list(range(2, 41, 2))):
            for exclude in (False, True):
                m = allowed_rows(ts, ids, exclude)
                sub = S.Table(ctx)
                sub.insert(tk[m], ts[m], to[m])
                sub.finalize()
                try:
                    for tol in (0, 2):
                        want = sub.match(qk, qo, qoff, 5, delta_tol=tol, floor=True)
                        for dbg in (0, SMALL):
                            ctx.set_debug(dbg)
                            try:
                                kw = dict(exclude=ids) if exclude else dict(songs=ids)
                                got = t.match(qk, qo, qoff, 5, delta_tol=tol, floor=True, **kw)
                            finally:
                                ctx.set_debug(0)
                            _same(got, want, (ids, exclude, tol, dbg))
                            _hist_eq(got, (want["song_hist"], want["bin_hist"]), (ids, exclude, tol, dbg))
                finally:
                    sub.close()
    finally:
        t.close()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------
def test_state_of_the_setting(S, ctx):
    from shazam_amd import _ffi
    from shazam_amd.shard import ShardedTable
    lib = _ffi.lib()
    b = _queries(7, 93)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        assert ctx.song_filter is None
        before = t.match(qk, qo, qoff, 3)
        in_set = t.match(qk, qo, qoff, 3, songs=ALLOWED)
        assert ctx.song_filter is None                                   # match(songs=) leaves no filter behind
        with pytest.raises(_ffi.ShzError):                                # ... nor after an exception inside
            t.match(qk, qo, qoff, 0, songs=ALLOWED)
        assert ctx.song_filter is None
        # songs() nests and restores
        with ctx.songs(only=ALLOWED):
            assert ctx.song_filter == {"n_sets": 1, "exclude": False, "n_ids": 6}
            _same(t.match(qk, qo, qoff, 3), in_set, "inside the block")
            with ctx.songs(exclude=[7, 7, 9]):
                assert ctx.song_filter == {"n_sets": 1, "exclude": True, "n_ids": 3}
                _same(t.match(qk, qo, qoff, 3), t.match(qk, qo, qoff, 3, exclude=[9, 7]), "nested")
                assert ctx.song_filter == {"n_sets": 1, "exclude": True, "n_ids": 3}
                with ctx.songs():
                    assert ctx.song_filter["n_ids"] == 3
            assert ctx.song_filter == {"n_sets": 1, "exclude": False, "n_ids": 6}
            _same(t.match(qk, qo, qoff, 3), in_set, "back in the outer block")
            with pytest.raises(ZeroDivisionError):
                with ctx.songs(sets=[[1], [2, 3]], exclude=True):
                    assert ctx.song_filter == {"n_sets": 2, "exclude": True, "n_ids": 3}
                    1 / 0
            assert ctx.song_filter == {"n_sets": 1, "exclude": False, "n_ids": 6}
            # the sharded match refuses while a filter is set
            n = C.c_uint64()
            assert lib.shz_match_pairs(ctx.h, t.h, _ffi.ptr(qk), _ffi.ptr(qo), qoff.ctypes.data_as(_ffi.u64p), 7, 0, 0, 1, 8, 12, 40,
                                       None, 0, C.byref(n), None, None) == _ffi.E_UNSUPPORTED
            out = _ffi._match_result(7, 3)
            assert lib.shz_pairs_vote(ctx.h, None, 0, 7, 8, 12, 40, 3, *(_ffi.ptr(out[k]) for k in ARRAYS[:5])) == _ffi.E_UNSUPPORTED
            st = ShardedTable(ctx, nshards=2)
            st.insert(tk, ts, to)
            st.finalize()
            try:
                with pytest.raises(NotImplementedError):
                    st.match(qk, qo, qoff, 3)
            finally:
                st.close()
        assert ctx.song_filter is None
        _same(t.match(qk, qo, qoff, 3), before, "plain match, afterwards")
        # refusals leave the previous setting in force
        ctx.set_song_filter(ALLOWED)
        ids, bad = np.array([1, 2], np.uint32), np.array([1, 2], np.uint64)
        assert lib.shz_set_song_filter(ctx.h, _ffi.ptr(ids), _ffi.ptr(bad), 1, 0) == _ffi.E_INVALID          # set_off[0] != 0
        assert lib.shz_set_song_filter(ctx.h, _ffi.ptr(ids), _ffi.ptr(np.array([0, 2, 1], np.uint64)), 2, 0) == _ffi.E_INVALID
        assert lib.shz_set_song_filter(ctx.h, None, _ffi.ptr(np.array([0, 2], np.uint64)), 1, 0) == _ffi.E_INVALID
        assert lib.shz_set_song_filter(ctx.h, _ffi.ptr(ids), None, 1, 0) == _ffi.E_INVALID
        top = np.array([(1 << 32) - 1, 5], np.uint32)                     # 2^27 words a set: five sets exceed 2^31 bytes
        assert lib.shz_set_song_filter(ctx.h, _ffi.ptr(top), _ffi.ptr(np.array([0, 2, 2, 2, 2, 2], np.uint64)), 5, 0) == _ffi.E_UNSUPPORTED
        assert ctx.song_filter == {"n_sets": 1, "exclude": False, "n_ids": 6}
        _same(t.match(qk, qo, qoff, 3), in_set, "after the refusals")
        # replace, then clear twice
        ctx.set_song_filter([[7], [9, 11]], exclude=True)
        assert ctx.song_filter == {"n_sets": 2, "exclude": True, "n_ids": 3}
        _same(t.match(qk, qo, qoff, 3), t.match(qk, qo, qoff, 3, exclude=[7]), "replaced: set 0")
        ctx.clear_song_filter()
        ctx.clear_song_filter()
        assert ctx.song_filter is None
        _same(t.match(qk, qo, qoff, 3), before, "cleared")
        # a filter set before the table existed, and a context of its own destroyed with a filter set
        c2 = _ffi.Context(0)
        c2.set_song_filter([1, 2, 3])
        c2.close()
    finally:
        ctx.clear_song_filter()
        t.close()
