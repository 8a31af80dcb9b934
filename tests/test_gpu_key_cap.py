"""GPU: the key cap (Context.key_cap, Table.match(max_key_rows=)) on tables and queries built by hand, against its
plain-Python definition (tests/key_cap_twin.py): a capped match gives the arrays of the plain match on a table lacking the rows
of every key that holds more than the cap.  Thresholds, several offsets a key, keys spread over segments, group counts at
the borders of the cap kernel and of the two heads, queries, the counters, a song filter on top, the sub-table definition on
a second table, the sharded table and the state of the setting.  Every case runs at delta_tol 0 and 2, with and without
floor=True, through match and match_device, and checks the context unchanged afterwards.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

from key_cap_twin import (dropped, expected_floor_cap, expected_floor_cap_sets, expected_match_cap, expected_match_cap_sets,
                          kept_rows, key_sizes)
from test_gpu_vote_floor import ARRAYS, Built, _hist_eq, _same
from vote_tol_twin import assert_match

pytestmark = pytest.mark.gpu

CAP_MAX = (1 << 64) - 1


def _mh_max():
    """MH_MAX of csrc/shz_table.hip: the most hashes of a sub-batch whose head runs in one workgroup"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shazam_amd", "csrc", "shz_table.hip")).read()
    threads, rows = (int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("MH_THREADS", "MH_ROWS"))
    assert re.search(r"#define MH_MAX \(MH_THREADS \* MH_ROWS\)", src)
    return threads * rows


MH_MAX = _mh_max()


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


class Keyed(Built):
    """Built with keys that hold several rows: group(queries, rows, q_offs) adds ONE new key with `rows` distinct table rows
    (songs 1 .. 5 in turn, a new offset every five rows) that every listed query hashes at every listed offset."""

    def group(self, queries, rows, q_offs=(None,), song=None):
        self.key += 1
        for r in range(rows):
            self.rows.append((self.key, 1 + r % 5 if song is None else song, 60 + r // 5 + self.key % 3))
        for q in queries:
            for o in q_offs:
                self.hashes[q].append((self.key, self.q_base if o is None else o))
        return self.key


def _table_of(S, ctx, rows):
    tk, ts, to = rows
    t = S.Table(ctx)
    t.insert(tk, ts, to)
    t.finalize()
    return t


def _check(S, ctx, b, cap, tols=(0, 2), topn=3, what="", t=None, songs=None):
    """match(floor=True, max_key_rows=cap) against the twin at every tolerance; match without the floor, match_device with
    and without it against that result; the counters of the last call; the context as it was afterwards.  b: a Built, or
    (tk, ts, to, qk, qo, qoff) -- with t given, the table rows are those t.export() shows.  songs: a song filter on top."""
    tk, ts, to, qk, qo, qoff = b.arrays() if isinstance(b, Built) else b
    own = t is None
    if own:
        t = _table_of(S, ctx, (tk, ts, to))
    kw = dict(max_key_rows=cap) if songs is None else dict(max_key_rows=cap, songs=songs)
    out = {}
    try:
        for tol in tols:
            if songs is None:
                want = expected_match_cap(tk, ts, to, qk, qo, qoff, tol, topn, cap)
                wantf = expected_floor_cap(tk, ts, to, qk, qo, qoff, tol, cap)
            else:
                want = expected_match_cap_sets(tk, ts, to, qk, qo, qoff, tol, topn, cap, [songs])
                wantf = expected_floor_cap_sets(tk, ts, to, qk, qo, qoff, tol, cap, [songs])
            res = t.match(qk, qo, qoff, topn, delta_tol=tol, floor=True, **kw)
            plain = t.match(qk, qo, qoff, topn, delta_tol=tol, **kw)
            stats, mstats = ctx.key_cap_stats(), t.match_stats()
            dev = t.match_device(qk, qo, qoff, topn, delta_tol=tol, floor=True, **kw)
            devb = t.match_device(qk, qo, qoff, topn, delta_tol=tol, bias_bound=int(qo.max()) if len(qo) else 0, **kw)
            assert_match(res, want, (what, tol))
            _hist_eq(res, wantf, (what, tol))
            _same(plain, res, (what, "no floor", tol))
            _same(dev, res, (what, "device", tol))
            _hist_eq(dev, wantf, (what, "device", tol))
            _same(devb, res, (what, "device, bound", tol))
            g, p = dropped(tk, ts, to, qk, qo, qoff, cap)
            assert stats == {"groups": g, "pairs": p}, (what, tol, stats, g, p)
            if songs is None:          # (under a song filter npairs counts what the filter left of the expanded pairs)
                assert mstats["pairs"] == int(plain["npairs"].sum()), (what, tol)
            assert ctx.key_cap == 0 and ctx.song_filter is None and not ctx.vote_floor and ctx.vote_tolerance == 0
            assert ctx.floor_rows() == 0
            out[tol] = res
    finally:
        if own:
            t.close()
    return out


# ---- 1. thresholds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 16, 17, 64])
def test_a_key_with_1_c_and_c_plus_1_rows(S, ctx, c):
    b = Keyed()
    for rows in (1, c, c + 1):
        b.group([0], rows)
    b.miss(0)
    r = _check(S, ctx, b, c, topn=6, what=("threshold", c))
    assert int(r[0]["npairs"][0]) == 1 + c and int(r[0]["nhash"][0]) == 4
    t = b.table(S, ctx)
    tk, ts, to, qk, qo, qoff = b.arrays()
    try:
        plain = t.match(qk, qo, qoff, 6, delta_tol=2)
        for cap in (c + 1, c + 2, 1 << 32, CAP_MAX, 0):       # at or above the largest key: the plain match array for array
            _same(t.match(qk, qo, qoff, 6, delta_tol=2, max_key_rows=cap), plain, ("no key above", c, cap))
            assert ctx.key_cap_stats() == {"groups": 0, "pairs": 0}
        assert int(plain["npairs"][0]) == 2 * c + 2
    finally:
        t.close()
    _check(S, ctx, b, CAP_MAX, tols=(0,), what=("2^64 - 1", c))
    if c > 1:
        r = _check(S, ctx, b, c - 1, tols=(0,), what=("below", c))
        assert int(r[0]["npairs"][0]) == 1


# ---- 2. several offsets per key ------------------------------------------------------------------------------------------------
def test_a_group_of_several_elements_goes_together(S, ctx):
    b = Keyed(n_queries=2)
    b.group([0], 3, q_offs=(4, 9, 20, 31))          # 3 rows x 4 offsets = 12 pairs
    b.group([0, 1], 2, q_offs=(4, 5))               # 2 rows x 2 offsets in both queries
    b.group([1], 4, q_offs=(7,))
    b.vote(0, 2, 3)
    for cap, pairs in ((1, [1, 0]), (2, [5, 4]), (3, [17, 4]), (4, [17, 8])):
        r = _check(S, ctx, b, cap, topn=5, what=("offsets", cap))
        assert r[0]["npairs"].tolist() == pairs and r[0]["nhash"].tolist() == [7, 3]
    tk, ts, to, qk, qo, qoff = b.arrays()
    assert dropped(tk, ts, to, qk, qo, qoff, 2) == (2, 12 + 4)


# ---- 3. segments ---------------------------------------------------------------------------------------------------------------
def _segmented(S, ctx, n_batches, c, seed):
    """n_batches batches finalized one by one into segments of at most 64 rows: 50 random rows under keys 1 .. 40 each, key
    500 with 3 new rows a batch, key 600 with c rows in all, dealt out over the batches"""
    rng = np.random.default_rng(seed)
    t = S.Table(ctx)
    t.set_segment_rows(64)
    share = np.array_split(np.arange(c), n_batches)
    for part in range(n_batches):
        k = np.concatenate([rng.integers(1, 41, 50), np.full(3, 500), np.full(len(share[part]), 600)]).astype(np.uint32)
        s = np.concatenate([rng.integers(1, 7, 50), np.full(3, 2), np.full(len(share[part]), 3)]).astype(np.uint32)
        o = np.concatenate([rng.integers(0, 300, 50), 100 + 3 * part + np.arange(3), 200 + share[part]]).astype(np.uint32)
        t.insert(k, s, o)
        t.finalize()
    return t


def _per_segment(tk, key):
    """rows of `key` in every segment of an export: a segment's keys never decrease, so a descent starts the next one"""
    cuts = np.flatnonzero(np.diff(tk.astype(np.int64)) < 0) + 1
    return [int((seg == key).sum()) for seg in np.split(tk, cuts)]


def _seg_queries(rng, tk):
    """3 queries over the table's keys, 500 and 600 among them (500 at two offsets in query 0), and a miss each"""
    keys = np.unique(tk)
    qs = []
    for q in range(3):
        ks = np.concatenate([rng.choice(keys[keys < 100], 12, replace=False), [500, 600, 7000 + q]])
        os_ = rng.integers(0, 50, len(ks))
        if q == 0:
            ks, os_ = np.concatenate([ks, [500]]), np.concatenate([os_, [55]])
        qs.append((ks, os_))
    qk = np.concatenate([a for a, _ in qs]).astype(np.uint32)
    qo = np.concatenate([b for _, b in qs]).astype(np.uint32)
    return qk, qo, np.cumsum([0] + [len(a) for a, _ in qs]).astype(np.uint64)


@pytest.mark.parametrize("n_batches", [1, 3, 5])
def test_a_key_spread_over_segments_counts_once_with_all_its_rows(S, ctx, n_batches):
    c = 3 * n_batches - 1                           # key 500: 3 n rows in all, c + 1; key 600: c rows in all
    t = _segmented(S, ctx, n_batches, c, 90 + n_batches)
    try:
        tk, ts, to = t.export()
        assert t.segments() == 1 if n_batches == 1 else t.segments() >= min(n_batches, 4)
        sizes = key_sizes(tk, ts, to)
        assert sizes[500] == c + 1 and sizes[600] == c
        if n_batches > 1:
            assert t.segments() >= 3 and max(_per_segment(tk, 500)) <= c and len([n for n in _per_segment(tk, 500) if n]) > 1
            assert len([n for n in _per_segment(tk, 600) if n]) > 1
        qk, qo, qoff = _seg_queries(np.random.default_rng(5), tk)
        r = _check(S, ctx, (tk, ts, to, qk, qo, qoff), c, topn=6, what=("segments", n_batches), t=t)
        kept = kept_rows(tk, c, ts, to)
        assert not kept[tk == 500].any() and kept[tk == 600].all()
        g, p = dropped(tk, ts, to, qk, qo, qoff, c)
        assert g >= 3 and p >= 4 * (c + 1)
        _check(S, ctx, (tk, ts, to, qk, qo, qoff), 4, tols=(0,), topn=6, what=("segments, cap 4", n_batches), t=t)
        full = t.match(qk, qo, qoff, 6, max_key_rows=c + 1)
        assert int(full["npairs"].sum()) > int(r[0]["npairs"].sum())
    finally:
        t.close()


def test_key_range_segments_of_one_bulk_finalize(S, ctx):
    rng = np.random.default_rng(17)
    t = S.Table(ctx)
    t.set_segment_rows(256)
    for run in range(2):                            # two sealed runs, one merge: segments by key range
        k = rng.integers(0, 120, 700).astype(np.uint32) * np.uint32(37)
        t.insert(k, rng.integers(1 + 50 * run, 51 + 50 * run, 700).astype(np.uint32), rng.integers(0, 4000, 700).astype(np.uint32))
        if run == 0:
            t.seal_run()
    t.finalize()
    try:
        assert t.segments() >= 4
        tk, ts, to = t.export()
        sizes = np.array(sorted(key_sizes(tk, ts, to).values()))
        keys = np.unique(tk)
        qk = np.concatenate([keys[::2], keys[1::2], [5]]).astype(np.uint32)       # every key in one of two queries, and a miss
        qo = np.concatenate([np.full(len(keys[::2]), 3), np.full(len(keys[1::2]), 9), [0]]).astype(np.uint32)
        qoff = np.array([0, len(keys[::2]), len(qk)], np.uint64)
        for cap in (int(sizes[len(sizes) // 2]), int(sizes[-1]) - 1):
            r = _check(S, ctx, (tk, ts, to, qk, qo, qoff), cap, topn=4, what=("key ranges", cap), t=t)
            assert ctx.key_cap_stats()["groups"] > 0 and int(r[0]["npairs"].sum()) > 0
    finally:
        t.close()


# ---- 4. group counts of a sub-batch -------------------------------------------------------------------------------------------
def _groups(n, way):
    """one query of n keys: a kept key holds one row, a dropped one two (cap 1)"""
    i = np.arange(n)
    drop = {"first": i < (n + 1) // 2, "last": i >= n // 2, "alternating": i % 2 == 0}[way]
    tk = np.concatenate([np.arange(1, n + 1), np.arange(1, n + 1)[drop]]).astype(np.uint32)
    ts = np.concatenate([1 + i % 4, (5 + i % 3)[drop]]).astype(np.uint32)
    to = np.concatenate([50 + i % 3, (90 + i % 2)[drop]]).astype(np.uint32)
    qk, qo = np.arange(1, n + 1, dtype=np.uint32), np.full(n, 20, np.uint32)
    return (tk, ts, to, qk, qo, np.array([0, n], np.uint64)), int(drop.sum())


@pytest.mark.parametrize("way", ["first", "last", "alternating"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_group_counts_at_the_kernel_borders(S, ctx, n, way):
    arrays, nd = _groups(n, way)
    r = _check(S, ctx, arrays, 1, what=(n, way))
    assert int(r[0]["npairs"][0]) == n - nd and int(r[0]["nhash"][0]) == n
    assert ctx.key_cap_stats() == {"groups": nd, "pairs": 2 * nd}


@pytest.mark.parametrize("way", ["first", "last", "alternating"])
@pytest.mark.parametrize("n", [MH_MAX - 1, MH_MAX, MH_MAX + 1])
def test_group_counts_around_the_one_workgroup_head(S, ctx, n, way):
    """up to MH_MAX hashes the head runs in one workgroup, above it head_sorted composes, sorts and compacts: both feed the
    probe and the cap kernel the same tables"""
    arrays, nd = _groups(n, way)
    r = _check(S, ctx, arrays, 1, tols=(0,), what=(n, way))
    assert int(r[0]["npairs"][0]) == n - nd
    two, _ = _groups(n, way)                        # the same keys as two queries: a sub-batch of two, the same groups twice
    tk, ts, to, qk, qo, _ = two
    r = _check(S, ctx, (tk, ts, to, np.concatenate([qk, qk]), np.concatenate([qo, qo]), np.array([0, n, 2 * n], np.uint64)), 1,
               tols=(2,), what=(n, way, "twice"))
    assert r[2]["npairs"].tolist() == [n - nd, n - nd]


# ---- 5. queries ----------------------------------------------------------------------------------------------------------------
def _queries(nq):
    """query 0 and 1 share a dropped and a kept key; query 2's hashes are all dropped; query 3 has none; query 4 matches
    nothing; the others hash a kept key of their own and the shared dropped one"""
    b = Keyed(n_queries=nq)
    shared = [q for q in range(nq) if q not in (3, 4)]
    b.group(shared, 9, q_offs=(3, 8))               # dropped under cap 4 in every query that hashes it
    b.group([q for q in (0, 1) if q < nq], 4)       # at the cap
    for q in range(nq):
        if q == 2:
            b.group([2], 5)
            b.group([2], 40)
        elif q == 3:
            continue
        elif q == 4:
            b.miss(q, 3)
        else:
            b.group([q], 1 + q % 4)
            b.vote(q, 2, q - 3)
            b.miss(q)
    return b


@pytest.mark.parametrize("nq", [1, 2, 3, 7])
def test_queries(S, ctx, nq):
    b = _queries(nq)
    r = _check(S, ctx, b, 4, topn=4, what=("queries", nq))[0]
    tk, ts, to, qk, qo, qoff = b.arrays()
    plain = expected_match_cap(tk, ts, to, qk, qo, qoff, 0, 4, 0)
    for q in range(nq):
        if q not in (3, 4):
            assert int(r["npairs"][q]) == plain[q][1] - 18 - (45 if q == 2 else 0), q      # the shared key in every query
    if nq > 2:
        assert int(r["nres"][2]) == 0 and int(r["npairs"][2]) == 0 and int(r["nhash"][2]) == 4
    if nq > 4:
        assert int(r["nhash"][3]) == 0 and int(r["nres"][3]) == 0
        assert int(r["nhash"][4]) == 3 and int(r["nres"][4]) == 0 and int(r["npairs"][4]) == 0


def test_one_small_host_query_takes_the_queued_fold_on_the_capped_counts(S, ctx):
    b = Keyed()
    for i in range(40):
        b.group([0], 1 + i % 6)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        for cap in (1, 3, 5, 6):
            queued, used = ctx.spec_stats()
            res = t.match(qk, qo, qoff, 4, max_key_rows=cap)
            assert ctx.spec_stats() == (queued + 1, used + 1), cap          # votes queued ahead of the count, and taken
            assert_match(res, expected_match_cap(tk, ts, to, qk, qo, qoff, 0, 4, cap), ("queued", cap))
            assert ctx.key_cap_stats() == dict(zip(("groups", "pairs"), dropped(tk, ts, to, qk, qo, qoff, cap)))
    finally:
        t.close()
    _check(S, ctx, b, 3, what="queued, all routes")


# ---- 6. counters ---------------------------------------------------------------------------------------------------------------
def test_counters_follow_the_last_call(S, ctx):
    b = _queries(7)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        off = t.match(qk, qo, qoff, 3)
        assert ctx.key_cap_stats() == {"groups": 0, "pairs": 0}
        assert t.match_stats()["pairs"] == int(off["npairs"].sum())
        rows_off = t.match_stats()["rows_scanned"]
        on = t.match(qk, qo, qoff, 3, max_key_rows=4)
        g, p = dropped(tk, ts, to, qk, qo, qoff, 4)
        assert ctx.key_cap_stats() == {"groups": g, "pairs": p} and g == 7 and p > 0
        st = t.match_stats()
        assert st["pairs"] == int(on["npairs"].sum()) == int(off["npairs"].sum()) - p
        assert st["rows_scanned"] == rows_off                  # rows scanned stay as probed
        t.match(qk, qo, qoff, 3)
        assert ctx.key_cap_stats() == {"groups": 0, "pairs": 0}
    finally:
        t.close()


# ---- 7. with a song filter on top ----------------------------------------------------------------------------------------------
def test_a_song_filter_on_top(S, ctx):
    b = _queries(5)
    for songs in ([1, 3], [2], []):
        _check(S, ctx, b, 4, topn=4, songs=songs, what=("filter", songs))
    _check(S, ctx, b, CAP_MAX, tols=(2,), topn=4, songs=[1, 2, 5], what="filter, cap above all")


# ---- 8. the sub-table definition -----------------------------------------------------------------------------------------------
def test_the_capped_match_is_the_plain_match_on_the_table_of_the_kept_rows(S, ctx):
    rng = np.random.default_rng(314)
    sizes = np.minimum(1 + (rng.pareto(0.9, 48) * 20).astype(np.int64), 400)     # skewed: most keys small, a few in the hundreds
    sizes[:3] = (1, 2, 3)
    tk = np.repeat(1 + 11 * np.arange(48), sizes).astype(np.uint32)
    pick = np.concatenate([rng.choice(40 * 600, n, replace=False) for n in sizes])        # distinct (song, offset) under a key
    ts, to = (1 + pick // 600).astype(np.uint32), (pick % 600).astype(np.uint32)
    assert 2500 <= len(tk) <= 3500                  # about 3,000 rows
    keys = np.unique(tk)
    qs = [rng.choice(keys, int(rng.integers(5, 30)), replace=False) for _ in range(9)]
    qk = np.concatenate(qs).astype(np.uint32)
    qo = rng.integers(0, 200, len(qk)).astype(np.uint32)
    qoff = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint64)
    t = _table_of(S, ctx, (tk, ts, to))
    try:
        hist = t.key_hist()
        assert hist["max_rows"] == int(sizes.max()) and hist["n_keys"] == 48
        for cap in (1, 3, int(np.median(sizes)), int(sizes.max()) - 1, int(sizes.max())):
            m = kept_rows(tk, cap)
            assert m.any() and (cap == sizes.max()) == bool(m.all())
            sub = _table_of(S, ctx, (tk[m], ts[m], to[m]))
            try:
                for tol in (0, 2):
                    got = t.match(qk, qo, qoff, 5, delta_tol=tol, floor=True, max_key_rows=cap)
                    want = sub.match(qk, qo, qoff, 5, delta_tol=tol, floor=True)
                    _same(got, want, ("sub-table", cap, tol))
                    assert np.array_equal(got["song_hist"], want["song_hist"]) and np.array_equal(got["bin_hist"], want["bin_hist"])
                    _same(t.match_device(qk, qo, qoff, 5, delta_tol=tol, max_key_rows=cap), want, ("sub-table, device", cap, tol))
            finally:
                sub.close()
        _check(S, ctx, (tk, ts, to, qk, qo, qoff), int(np.median(sizes)), topn=5, what="sub-table, twin", t=t)
    finally:
        t.close()


# ---- 9. sharded ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nshards", [1, 2, 3])
def test_sharded_table_gives_the_unsharded_result(S, ctx, nshards):
    from shazam_amd.shard import ShardedTable
    b = _queries(7)
    for i in range(30):
        b.group([i % 7], 1 + i % 9, q_offs=(2, 6) if i % 4 == 0 else (None,))
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    st = ShardedTable(ctx, nshards=nshards)
    st.insert(tk, ts, to)
    st.finalize()
    try:
        for cap in (1, 4, 8, CAP_MAX):
            for tol in (0, 2):
                want = t.match(qk, qo, qoff, 3, delta_tol=tol, floor=True, max_key_rows=cap)
                got = st.match(qk, qo, qoff, 3, delta_tol=tol, floor=True, max_key_rows=cap)
                _same(got, want, ("sharded", nshards, cap, tol))
                _hist_eq(got, (want["song_hist"], want["bin_hist"]), ("sharded", nshards, cap, tol))
            assert_match(st.match(qk, qo, qoff, 3, max_key_rows=cap), expected_match_cap(tk, ts, to, qk, qo, qoff, 0, 3, cap),
                         ("sharded, twin", nshards, cap))
            assert ctx.key_cap == 0
        h, hs = t.key_hist(), st.key_hist()
        assert np.array_equal(h["keys"], hs["keys"]) and np.array_equal(h["rows"], hs["rows"])
        assert (h["max_rows"], h["n_keys"]) == (hs["max_rows"], hs["n_keys"])
    finally:
        st.close()
        t.close()


# ---- 10. the state of the setting ----------------------------------------------------------------------------------------------
def test_state_of_the_setting(S, ctx):
    from shazam_amd import _ffi
    b = _queries(3)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    try:
        plain = t.match(qk, qo, qoff, 3)
        capped = t.match(qk, qo, qoff, 3, max_key_rows=4)
        assert ctx.key_cap == 0 and isinstance(ctx.key_cap, int)
        assert int(capped["npairs"].sum()) < int(plain["npairs"].sum())
        with ctx.key_cap(4) as c:
            assert c is ctx and ctx.key_cap == 4
            _same(t.match(qk, qo, qoff, 3), capped, "inside the block")
            with ctx.key_cap(None):
                assert ctx.key_cap == 4
            with ctx.key_cap(40):                   # (the largest key holds 40 rows)
                assert ctx.key_cap == 40
                _same(t.match(qk, qo, qoff, 3), plain, "nested, cap 40")
                _same(t.match(qk, qo, qoff, 3, max_key_rows=4), capped, "the keyword inside a block")
                assert ctx.key_cap == 40
                with ctx.key_cap(0):
                    assert ctx.key_cap == 0
                    _same(t.match(qk, qo, qoff, 3), plain, "nested, off")
                assert ctx.key_cap == 40
            assert ctx.key_cap == 4
        assert ctx.key_cap == 0
        with pytest.raises(RuntimeError, match="boom"):
            with ctx.key_cap(2):
                with ctx.key_cap(CAP_MAX):
                    assert ctx.key_cap == CAP_MAX
                    raise RuntimeError("boom")
        assert ctx.key_cap == 0
        with pytest.raises(_ffi.ShzError):          # a refused call inside max_key_rows= leaves nothing behind
            t.match(qk, qo, qoff, 65, max_key_rows=4)
        assert ctx.key_cap == 0
        for bad in (-1, 1 << 64):
            with pytest.raises(_ffi.ShzError):
                ctx.set_key_cap(bad)
        ctx.set_key_cap(4)
        try:
            assert ctx.key_cap == 4
            _same(t.match(qk, qo, qoff, 3), capped, "set by hand")
            _same(t.match(qk, qo, qoff, 3, max_key_rows=0), plain, "the keyword switches it off for a call")
            assert ctx.key_cap == 4
        finally:
            ctx.set_key_cap(0)
        _same(t.match(qk, qo, qoff, 3), plain, "off again")
        c2 = _ffi.Context(0)                       # a context of its own destroyed with a cap set
        c2.set_key_cap(7)
        assert c2.key_cap == 7 and c2.key_cap_stats() == {"groups": 0, "pairs": 0}
        c2.close()
    finally:
        ctx.set_key_cap(0)
        t.close()
