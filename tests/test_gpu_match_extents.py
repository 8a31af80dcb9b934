"""GPU: Table.match_extents (shz_match_extents) on tables and queries built by hand, so that every pair is known, against its
plain-Python definition (tests/extent_twin.py): both inclusive ends of a range, the set semantics, the borders of a tile, of
the LDS descriptor table and of a sub-batch of queries, the walk over segments, and a random fuzz.  Every case runs with and
without SHZ_DEBUG_EXTENT_SMALL_TILES (tiles of 64 pairs, 4 descriptors, 3 queries a sub-batch); every comparison is exact,
the zeros past cand_n included."""
import numpy as np
import pytest

from extent_twin import SCALARS, assert_extents, expected_extents

pytestmark = pytest.mark.gpu

QMAX = (1 << 20) - 1


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _table(S, ctx, rows):
    t = S.Table(ctx)
    if rows:
        tk, ts, to = (np.asarray([r[i] for r in rows], np.uint32) for i in range(3))
        t.insert(tk, ts, to)
    t.finalize()
    return t


def _query_arrays(queries):
    qk = np.asarray([h[0] for hs in queries for h in hs], np.uint32)
    qo = np.asarray([h[1] for hs in queries for h in hs], np.uint32)
    qoff = np.cumsum([0] + [len(hs) for hs in queries]).astype(np.uint64)
    return qk, qo, qoff


def _cand_arrays(cands, ncand=None):
    """cands: per query a list of (sid, d_lo, d_hi) -> [n, ncand] arrays and cand_n; unused slots hold a filler that would
    match every pair of song 1 if it were read"""
    n = len(cands)
    ncand = ncand or max(1, max((len(c) for c in cands), default=1))
    cs, lo, hi = np.full((n, ncand), 1, np.uint32), np.full((n, ncand), -(1 << 30), np.int32), np.full((n, ncand), 1 << 30, np.int32)
    for q, c in enumerate(cands):
        for i, (s, a, b) in enumerate(c):
            cs[q, i], lo[q, i], hi[q, i] = s, a, b
    return cs, lo, hi, np.asarray([len(c) for c in cands], np.uint32)


def _check(S, ctx, t, queries, cands, what, ncand=None, flags=None):
    """match_extents of the queries against the twin on the table's export, switch off and on, with and without hist"""
    from shazam_amd import _ffi
    tk, ts, to = t.export()
    qk, qo, qoff = _query_arrays(queries)
    cs, lo, hi, cn = _cand_arrays(cands, ncand)
    want = expected_extents(tk, ts, to, qk, qo, qoff, cs.tolist(), lo.tolist(), hi.tolist(), cn)
    out = None
    for flag in ((0, _ffi.DEBUG_EXTENT_SMALL_TILES) if flags is None else flags):
        ctx.set_debug(flag)
        try:
            res = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn)
            bare = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn, hist=None)
        finally:
            ctx.set_debug(0)
        assert_extents(res, want, (what, flag))
        assert bare["hist"] is None
        for k in SCALARS + ("shift",):
            assert np.array_equal(bare[k], res[k]), (what, flag, k)
        assert np.array_equal(res["hist"].sum(axis=2), res["count"]), (what, flag)
        out = res
    return out


def _one(res, q=0, c=0):
    return tuple(int(res[k][q, c]) for k in SCALARS)


def test_one_pair_and_a_candidate_nothing_belongs_to(S, ctx):
    t = _table(S, ctx, [(5, 3, 17)])
    r = _check(S, ctx, t, [[(5, 4)]], [[(3, 13, 13), (3, 14, 14), (2, 13, 13)]], "one pair")
    assert _one(r, 0, 0) == (1, 4, 4, 17, 17) and _one(r, 0, 1) == (0, 0, 0, 0, 0) and _one(r, 0, 2) == (0, 0, 0, 0, 0)
    assert int(r["shift"][0]) == 0 and int(r["hist"][0, 0, 4]) == 1
    t.close()
    e = _table(S, ctx, [])                                   # the empty table: no pair at all
    r = _check(S, ctx, e, [[(5, 4)], []], [[(3, 13, 13)], [(1, 0, 0)]], "empty table")
    assert not r["count"].any()
    e.close()


def test_negative_deltas_and_a_range_across_zero_with_both_ends(S, ctx):
    rows, q = [], []
    for i, d in enumerate(range(-3, 5)):                     # one pair at every d from d_lo - 1 to d_hi + 1
        rows.append((100 + i, 1, 50 + d))
        q.append((100 + i, 50))
    rows += [(200, 2, 3), (201, 2, 10), (202, 1, 0)]
    q += [(200, 40), (201, 47), (202, 60)]                   # song 2 at delta -37 twice, song 1 at -60
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q], [[(1, -2, 3), (2, -37, -37), (1, -60, -60), (1, -3, -3), (1, 4, 4), (1, -61, -61)]], "across zero")
    assert _one(r, 0, 0) == (6, 50, 50, 48, 53)
    assert _one(r, 0, 1) == (2, 40, 47, 3, 10)
    assert _one(r, 0, 2) == (1, 60, 60, 0, 0)
    assert _one(r, 0, 3)[0] == 1 and _one(r, 0, 4)[0] == 1 and _one(r, 0, 5)[0] == 0
    t.close()


def test_query_offsets_0_and_top_and_duplicate_hashes(S, ctx):
    rows = [(1, 1, 0), (2, 1, QMAX), (3, 1, (1 << 31) - 1), (4, 1, 7)]
    q = [(1, 0), (2, QMAX), (3, QMAX), (3, QMAX), (4, 7), (4, 7), (4, 7)]       # (4, 7) three times: one pair
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q], [[(1, 0, 0), (1, (1 << 31) - 1 - QMAX, (1 << 31) - 1 - QMAX), (1, -QMAX, (1 << 31) - 1)]], "edges")
    assert _one(r, 0, 0) == (3, 0, QMAX, 0, QMAX)
    assert _one(r, 0, 1) == (1, QMAX, QMAX, (1 << 31) - 1, (1 << 31) - 1)
    assert _one(r, 0, 2)[0] == 4 and int(r["shift"][0]) == 14
    t.close()


def test_two_candidates_of_one_song(S, ctx):
    rows = [(10 + i, 1, 100 + i) for i in range(6)] + [(20 + i, 1, 500 + i) for i in range(4)]
    q = [(10 + i, 90) for i in range(6)] + [(20 + i, 90) for i in range(4)]    # deltas 10..15 and 410..413
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q], [[(1, 10, 12), (1, 410, 413), (1, 11, 14), (1, 13, 411), (1, 10, 12)]], "one song twice")
    assert [_one(r, 0, c)[0] for c in range(5)] == [3, 4, 4, 5, 3]
    t.close()


def test_64_candidates_and_cand_n_0_1_64(S, ctx):
    rows = [(1000 + d, 1 + d % 3, 200 + d) for d in range(64)]
    q = [(1000 + d, 200) for d in range(64)]
    full = [(1 + d % 3, d, d) for d in range(64)]
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q, q, q], [[], [(1, 0, 63)], full], "64 candidates", ncand=64)
    assert not r["count"][0].any() and r["count"][1].tolist() == [22] + [0] * 63 and r["count"][2].tolist() == [1] * 64
    t.close()


def test_an_empty_query_between_two_others(S, ctx):
    t = _table(S, ctx, [(1, 1, 10), (2, 1, 20), (3, 2, 30)])
    r = _check(S, ctx, t, [[(1, 5), (2, 15)], [], [(3, 1), (1, 5)]], [[(1, 5, 5)], [(1, 5, 5)], [(2, 29, 29), (1, 5, 5)]], "empty between")
    assert _one(r, 0, 0) == (2, 5, 15, 10, 20) and _one(r, 1, 0) == (0, 0, 0, 0, 0)
    assert _one(r, 2, 0) == (1, 1, 1, 30, 30) and _one(r, 2, 1) == (1, 5, 5, 10, 10)
    t.close()


def test_one_key_with_300_rows_spans_several_tiles(S, ctx):
    rows = [(77, 1, 3 * i) for i in range(300)] + [(77, 2, i) for i in range(50)]
    q = [(77, 0), (77, 3), (77, 600)]
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q], [[(1, 0, 897), (1, 300, 300), (1, -600, -1), (2, 0, 49)]], "one key")
    assert _one(r, 0, 0)[0] == 300 + 299 + 100 and _one(r, 0, 1) == (2, 0, 3, 300, 303)
    assert _one(r, 0, 2)[0] == 1 + 200 and _one(r, 0, 3)[0] == 50 + 47
    t.close()


def test_300_keys_with_one_row_each_overflow_the_descriptor_table(S, ctx):
    rows = [(5000 + 7 * i, 1 + (i % 2), 10 + i) for i in range(300)]
    q = [(5000 + 7 * i, i % 9) for i in range(300)] + [(4999, 0), (9999, 3)]    # (two keys without rows)
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q], [[(1, 0, 400), (2, 0, 400), (2, 100, 150)]], "300 keys")
    assert _one(r, 0, 0)[0] == 150 and _one(r, 0, 1)[0] == 150
    t.close()


def test_two_queries_share_a_tile_with_one_song_at_different_deltas(S, ctx):
    rows = [(300 + i, 9, 40 + i) for i in range(10)] + [(300 + i, 9, 70 + i) for i in range(10)]
    qa = [(300 + i, i) for i in range(10)]                   # deltas 40 and 70
    qb = [(300 + i, 30 + i) for i in range(10)]              # deltas 10 and 40
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [qa, qb], [[(9, 70, 70)], [(9, 10, 10)]], "shared tile")
    assert _one(r, 0, 0) == (10, 0, 9, 70, 79) and _one(r, 1, 0) == (10, 30, 39, 40, 49)
    r = _check(S, ctx, t, [qa, qb, qa, qb, qa, qb], [[(9, 40, 40)]] * 6, "more queries than the LDS cache in one tile")
    assert r["count"][:, 0].tolist() == [10] * 6
    t.close()


def test_three_segments_with_one_keys_rows_in_two(S, ctx):
    t = S.Table(ctx)
    t.set_segment_rows(16)
    rng = np.random.default_rng(5)
    for part in range(4):
        k = np.concatenate([rng.integers(0, 1 << 32, 14, dtype=np.uint64).astype(np.uint32), np.full(6, 4242, np.uint32)])
        s = np.concatenate([np.full(14, 10 + part, np.uint32), np.full(6, 1, np.uint32)])
        o = np.concatenate([rng.integers(0, 99, 14).astype(np.uint32), (100 * part + np.arange(6)).astype(np.uint32)])
        t.insert(k, s, o)
        t.finalize()
    assert t.segments() >= 3
    tk, ts, to = t.export()
    assert (tk == 4242).sum() == 24
    q = [(4242, 0), (4242, 2)] + [(int(k), 1) for k in tk[::5] if k != 4242]
    r = _check(S, ctx, t, [q, q[:1]], [[(1, 0, 400), (1, 100, 105), (10, -50, 99), (13, -50, 99)], [(1, 298, 305)]], "segments")
    assert _one(r, 0, 0)[0] == 24 + 22 and _one(r, 0, 1)[0] == 6 + 4 and _one(r, 1, 0) == (6, 0, 0, 300, 305)
    t.close()


def test_a_table_built_through_sealed_runs(S, ctx):
    t = S.Table(ctx)
    rng = np.random.default_rng(6)
    for run in range(3):
        k = rng.integers(0, 40, 200).astype(np.uint32)
        t.insert(k, np.full(200, 1 + run, np.uint32), rng.integers(0, 60, 200).astype(np.uint32))
        t.seal_run()
    t.finalize()
    q = [(int(k), int(o)) for k, o in zip(rng.integers(0, 40, 120), rng.integers(0, 30, 120))]
    _check(S, ctx, t, [q, q[:40]], [[(1, 0, 5), (2, -5, 0), (3, 10, 10)], [(2, 0, 60), (3, -30, 0)]], "runs")
    t.close()


def test_the_sub_batch_cut(S, ctx):
    from shazam_amd import _ffi
    rows = [(i, 1 + i % 2, i % 50) for i in range(4100)]
    t = _table(S, ctx, rows)
    many = [[(i, 3)] for i in range(4097)]                   # 4,097 queries of one hash each: the 4,096 cut, without the switch
    r = _check(S, ctx, t, many, [[(1 + i % 2, -3, 46)] for i in range(4097)], "4097 queries", flags=(0,))
    assert r["count"][:, 0].tolist() == [1] * 4097
    few = [[(i, 3), (i + 1, 4)] for i in range(7)]           # 7 queries: sub-batches of 3, 3, 1 under the switch
    r = _check(S, ctx, t, few, [[(1, -3, 46), (2, -3, 46)]] * 7, "7 queries", flags=(_ffi.DEBUG_EXTENT_SMALL_TILES,))
    assert r["count"].tolist() == [[1, 1]] * 7
    t.close()


@pytest.mark.parametrize("shift", [0, 3])
def test_hist_on_both_sides_of_every_bucket_edge(S, ctx, shift):
    w = 1 << shift
    offs = sorted(set([0] + [b * w - 1 for b in range(1, 64)] + [b * w for b in range(1, 64)] + [64 * w - 1]))
    rows = [(i, 1, o + 11) for i, o in enumerate(offs)] + [(900, 1, 12)]
    q = [(i, o) for i, o in enumerate(offs)] + [(900, 1), (900, 1)]
    t = _table(S, ctx, rows)
    r = _check(S, ctx, t, [q], [[(1, 11, 11)]], ("bucket edges", shift))
    assert int(r["shift"][0]) == shift
    want = np.bincount(np.asarray(offs + [1]) >> shift, minlength=64)      # ((900, 1) twice in the query: one pair)
    assert r["hist"][0, 0].tolist() == want.tolist() and want.min() >= 1
    t.close()


def _random_table(rng, n_rows=2000, n_keys=50, n_songs=6, n_off=41):
    return [(int(k), int(s), int(o)) for k, s, o in zip(rng.integers(0, n_keys, n_rows), rng.integers(1, n_songs + 1, n_rows),
                                                         rng.integers(0, n_off, n_rows))]


@pytest.mark.parametrize("topn", [1, 2, 5])
def test_count_is_the_aligned_of_the_match(S, ctx, topn):
    from shazam_amd import _ffi
    from shazam_amd.extent import extents_of
    rng = np.random.default_rng(40 + topn)
    t = _table(S, ctx, _random_table(rng))
    queries = [[(int(k), int(o)) for k, o in zip(rng.integers(0, 50, n), rng.integers(0, 41, n))] for n in (150, 0, 7, 200)]
    qk, qo, qoff = _query_arrays(queries)
    res = t.match(qk, qo, qoff, topn, delta_tol=0)
    assert int(res["nres"].max()) == topn
    for flag in (0, _ffi.DEBUG_EXTENT_SMALL_TILES):
        ctx.set_debug(flag)
        try:
            ext = extents_of(t, qk, qo, qoff, res, tol=0)
            wide = extents_of(t, qk, qo, qoff, res, tol=2)
        finally:
            ctx.set_debug(0)
        assert np.array_equal(ext["count"], res["aligned"]), flag          # (both are zero past nres)
        assert np.array_equal(ext["hist"].sum(axis=2), res["aligned"])
        assert (wide["count"] >= ext["count"]).all()
    t.close()


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_against_the_twin(S, ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    t = _table(S, ctx, _random_table(rng))
    queries = [[(int(k), int(o)) for k, o in zip(rng.integers(0, 50, n), rng.integers(0, 41, n))]
               for n in rng.integers(0, 201, 5)]
    qk, qo, qoff = _query_arrays(queries)
    res = t.match(qk, qo, qoff, 3, delta_tol=0)
    cands = []
    for q in range(5):
        c = [(int(res["sid"][q, i]), int(res["delta"][q, i]) - int(rng.integers(0, 3)), int(res["delta"][q, i]) + int(rng.integers(0, 3)))
             for i in range(int(res["nres"][q]))]
        for _ in range(int(rng.integers(0, 5))):
            lo = int(rng.integers(-45, 45))
            c.append((int(rng.integers(1, 8)), lo, lo + int(rng.integers(0, 30))))
        cands.append(c)
    _check(S, ctx, t, queries, cands, ("fuzz", seed))
    t.close()


# ---- refusals: the status, and the outputs as they were -----------------------------------------------------------------
def _raw(ctx, t, qk, qo, qoff, n, ncand, cs, lo, hi, cn, null=None, ctx_h="ctx", t_h="t"):
    """shz_match_extents as it is, on outputs filled with a pattern: (status, outputs untouched?)"""
    from shazam_amd import _ffi
    L, ptr = _ffi.lib(), _ffi.ptr
    cells = max(n, 1) * max(min(ncand, 64), 1)
    outs = {k: np.full(cells, 0xABABABAB, np.uint32) for k in SCALARS}
    outs["hist"] = np.full(cells * 64, 0xABABABAB, np.uint32)
    outs["shift"] = np.full(max(n, 1), 0xABABABAB, np.uint32)
    a = {"key32": qk, "q_off": qo, "query_off": qoff, "cand_sid": cs, "cand_dlo": lo, "cand_dhi": hi, "cand_n": cn, **outs}
    if null:
        a[null] = None
    rc = L.shz_match_extents(ctx.h if ctx_h == "ctx" else None, t.h if t_h == "t" else None, ptr(a["key32"]), ptr(a["q_off"]),
                             None if a["query_off"] is None else a["query_off"].ctypes.data_as(_ffi.u64p), n, ncand,
                             ptr(a["cand_sid"]), ptr(a["cand_dlo"]), ptr(a["cand_dhi"]), ptr(a["cand_n"]), ptr(a["count"]),
                             ptr(a["q_first"]), ptr(a["q_last"]), ptr(a["t_first"]), ptr(a["t_last"]), ptr(a["hist"]), ptr(a["shift"]))
    return rc, all((v == 0xABABABAB).all() for v in outs.values())


def test_refusals_leave_the_outputs_untouched(S, ctx):
    from shazam_amd import _ffi
    t = _table(S, ctx, [(1, 1, 10), (2, 1, 20)])
    qk, qo, qoff = _query_arrays([[(1, 5)], [(2, 15)]])
    cs, lo, hi, cn = _cand_arrays([[(1, 5, 5)], [(1, 5, 5)]], ncand=2)
    base = (qk, qo, qoff, 2, 2, cs, lo, hi, cn)
    rc, same = _raw(ctx, t, *base)
    assert rc == _ffi.OK and not same
    assert _raw(ctx, t, *base, ctx_h=None) == (_ffi.E_INVALID, True)
    assert _raw(ctx, t, *base, t_h=None) == (_ffi.E_INVALID, True)
    for name in ("key32", "q_off", "query_off", "cand_sid", "cand_dlo", "cand_dhi", "cand_n") + SCALARS + ("shift",):
        assert _raw(ctx, t, *base, null=name) == (_ffi.E_INVALID, True), name
    rc, same = _raw(ctx, t, *base, null="hist")               # (the histogram may be NULL)
    assert rc == _ffi.OK
    for ncand in (0, 65):
        assert _raw(ctx, t, qk, qo, qoff, 2, ncand, cs, lo, hi, cn) == (_ffi.E_INVALID, True)
    assert _raw(ctx, t, qk, qo, qoff, 2, 2, cs, lo, hi, np.asarray([1, 3], np.uint32)) == (_ffi.E_INVALID, True)
    bad_lo = lo.copy()
    bad_lo[1, 0] = 6                                          # a used candidate with d_lo > d_hi
    assert _raw(ctx, t, qk, qo, qoff, 2, 2, cs, bad_lo, hi, cn) == (_ffi.E_INVALID, True)
    bad_lo = lo.copy()
    bad_lo[1, 1], bad_hi = 9, hi.copy()
    bad_hi[1, 1] = 8                                          # ... an unused one is never read
    rc, same = _raw(ctx, t, qk, qo, qoff, 2, 2, cs, bad_lo, bad_hi, cn)
    assert rc == _ffi.OK
    wide = qo.copy()
    wide[1] = 1 << 20
    assert _raw(ctx, t, qk, wide, qoff, 2, 2, cs, lo, hi, cn) == (_ffi.E_UNSUPPORTED, True)
    assert _raw(ctx, t, qk, qo, qoff, 0, 2, cs, lo, hi, cn) == (_ffi.OK, True)     # no query: nothing is written
    # the state of the table
    t.insert(np.asarray([3], np.uint32), 1, np.asarray([5], np.uint32))
    assert _raw(ctx, t, *base) == (_ffi.E_STATE, True)        # staged rows
    t.seal_run()                                              # a sealed run that waits for its merge is refused like staged rows;
    waiting = t.rows()[1] > 0                                 # (a table that holds no runs merges a small one at once)
    rc, same = _raw(ctx, t, *base)
    assert (rc, same) == (_ffi.E_STATE, True) if waiting else rc == _ffi.OK
    t.finalize()
    assert _raw(ctx, t, *base)[0] == _ffi.OK
    t.insert(np.asarray([4], np.uint32), 1, np.asarray([1 << 31], np.uint32))
    t.finalize()
    assert _raw(ctx, t, *base) == (_ffi.E_UNSUPPORTED, True)  # a table offset >= 2^31
    t.close()
    fresh = S.Table(ctx)
    assert _raw(ctx, fresh, *base) == (_ffi.E_STATE, True)    # never finalized
    fresh.close()
    with pytest.raises(_ffi.ShzError):
        _table(S, ctx, [(1, 1, 1)]).match_extents(qk, qo, qoff, cs, hi + 1, hi)
