"""GPU: the table build AT its run limit -- the most rows one sorted run, or one segment cut from runs, may hold
(SHZ_RUN_ROWS_MAX = 2^32 - 4096, inclusive).  SHZ_DEBUG_RUN_LIMIT_SMALL lowers that limit to L = 65,536 rows for one
context, so that the cuts at the limit are reached with few rows: the run cut of seal_run, set_run_rows' clamp,
finalize_runs' blocks, the segment cut of a table that is not reserved for gathering, and the size check of an
exchange round.  Every case compares the table with np.unique over (key, sid, off) rows: INSERT IGNORE across the cuts
(mysql_database.py:54-55, 62-68).  The real limit is tested in test_gpu_table_4g.py."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from shazam_amd import _ffi
    ctx = _ffi.Context(0)   # a context of its own: the switch holds for every table of the context
    ctx.set_debug(_ffi.DEBUG_RUN_LIMIT_SMALL)
    yield _ffi, ctx, _ffi.RUN_ROWS_MAX_SMALL
    ctx.close()


def _rows(rng, n, L, ordered, sid_lo=1, sid_hi=300):
    """n rows, duplicates on both sides of every multiple of L (rows c-2 .. c+2 are row c-1) and inside the first run.
    ordered: by (sid, off), the order the stable key-only sort of seal_rows takes (the duplicates keep that order)."""
    k = (rng.integers(0, 1 << 22, n).astype(np.uint32) << np.uint32(8)) | rng.integers(0, 6, n).astype(np.uint32)
    s = rng.integers(sid_lo, sid_hi, n).astype(np.uint32)
    o = rng.integers(0, 4000, n).astype(np.uint32)
    if ordered:
        idx = np.lexsort((o, s))
        k, s, o = k[idx], s[idx], o[idx]
    for a in (k, s, o):
        if n > 12:
            a[6:12] = a[5]
        for c in range(L, n, L):
            a[c - 2:c + 3] = a[c - 1]
    return k, s, o


def _want(*parts):
    return np.unique(np.concatenate([np.stack(p, 1) for p in parts]).astype(np.uint64), axis=0)


def _table_rows(tbl):
    return np.stack(tbl.export(), 1).astype(np.uint64)


def _by_key(k, s, o):
    """lookup() rows with each key's group ordered by (sid, off): a segmented table lists a key's rows segment by segment"""
    g = np.cumsum(np.r_[0, k[1:] != k[:-1]])[:len(k)]
    idx = np.lexsort((o, s, g))
    return k[idx], s[idx], o[idx]


def _assert_table(tbl, want):
    rows = _table_rows(tbl)
    assert tbl.rows() == (len(want), 0)
    assert len(rows) == len(want) and np.array_equal(np.unique(rows, axis=0), want)


@pytest.mark.parametrize("ordered", [False, True], ids=["random", "sid_off_ordered"])
@pytest.mark.parametrize("m", [(1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 17)], ids=lambda m: f"{m[0]}L{m[1]:+d}")
def test_seal_run_cuts_sub_runs_at_the_limit(env, m, ordered):
    F, ctx, L = env
    n = m[0] * L + m[1]
    rng = np.random.default_rng(n * 2 + ordered)
    k, s, o = _rows(rng, n, L, ordered)
    tbl = F.Table(ctx)
    try:
        tbl.reserve(n, n, gather=True)   # (the batch hint is clamped to the limit)
        tbl.insert(k, s, o)
        tbl.seal_run()
        assert tbl.exchange_stats()["runs_held"] == -(-n // L)
        tbl.finalize()
        _assert_table(tbl, _want((k, s, o)))
        assert tbl.segments() >= -(-tbl.rows()[0] // L)   # (a segment cut from runs holds at most L rows)
    finally:
        tbl.close()


@pytest.mark.parametrize("run_rows", ["L", "L+1"])
def test_set_run_rows_at_and_above_the_limit(env, run_rows):
    F, ctx, L = env
    n = 2 * L + 5
    rng = np.random.default_rng(7 + len(run_rows))
    k, s, o = _rows(rng, n, L, False)
    tbl = F.Table(ctx)
    try:
        tbl.reserve(0, 0, gather=True)
        tbl.set_run_rows(L if run_rows == "L" else L + 1)   # L + 1 is clamped to L
        tbl.insert(k, s, o)
        tbl.seal_run()
        assert tbl.exchange_stats()["runs_held"] == 3
        tbl.finalize()
        _assert_table(tbl, _want((k, s, o)))
    finally:
        tbl.close()


@pytest.mark.parametrize("blocks", [["L"], ["L+1"], ["L", "0", "1", "L"]], ids=lambda b: "_".join(b))
def test_finalize_runs_blocks_at_the_limit(env, blocks):
    F, ctx, L = env
    sizes = [{"L": L, "L+1": L + 1, "0": 0, "1": 1}[b] for b in blocks]
    n = sum(sizes)
    rng = np.random.default_rng(n + len(blocks))
    k, s, o = _rows(rng, n, L, False)
    # the first row of every block is also the last row of the one before it (duplicates across the runs)
    at = np.cumsum(sizes)[:-1]
    for a in (k, s, o):
        for c in at:
            if 0 < c < n:
                a[c] = a[c - 1]
    tbl = F.Table(ctx)
    try:
        tbl.insert(k, s, o)
        tbl.finalize_runs(sizes)
        _assert_table(tbl, _want((k, s, o)))
    finally:
        tbl.close()


def test_segment_cut_at_the_limit_equals_unsegmented_build(env):
    """A table not reserved for gathering cuts full segments (min(segment rows, limit) = L rows at most) on seal_run;
    lookups and a match give what one unsegmented table of the same rows gives (a context without the switch)."""
    F, ctx, L = env
    rng = np.random.default_rng(2024)
    batches = [_rows(rng, n, L, False) for n in (L - 3, L + 1, L, 2 * L + 9, 17)]
    # rows of the first batch again in the later ones: duplicates across segments
    for b in batches[1:]:
        m = min(40, len(b[0]))
        for a, src in zip(b, batches[0]):
            a[-m:] = src[1000:1000 + m]
    want = _want(*batches)
    seg = F.Table(ctx)
    plain_ctx = F.Context(0)
    plain = F.Table(plain_ctx)
    try:
        seg.set_segment_rows(3 * L)   # above the limit: the limit cuts
        for b in batches:
            seg.insert(*b)
            seg.seal_run()
            plain.insert(*b)
        seg.finalize()
        plain.finalize()
        assert plain.segments() == 1
        assert seg.segments() >= -(-len(want) // L) and seg.segments() >= 4
        _assert_table(seg, want)
        _assert_table(plain, want)
        # every key of the table (the first and last rows of every segment among them) and keys that are absent
        rows = _table_rows(seg)
        v = (rows[:, 0] << np.uint64(21)) | (rows[:, 1] << np.uint64(12)) | rows[:, 2]   # (sid < 2^9, off < 2^12)
        # where a segment of a later flush restarts the order (the pieces of one flush follow each other in key order,
        # their edges are among the keys looked up below)
        starts = np.flatnonzero(v[1:] < v[:-1]) + 1
        assert len(starts) >= 1
        edge = rows[np.r_[0, starts - 1, starts, len(rows) - 1], 0].astype(np.uint32)
        present = set(want[:, 0].tolist())
        absent = np.array([x for x in rng.integers(0, 1 << 30, 4000).astype(np.uint32).tolist() if x not in present][:2000], np.uint32)
        for keys in (edge, np.unique(want[:, 0]).astype(np.uint32), absent, np.r_[absent[:50], edge[:50], absent[50:100]]):
            got, exp = seg.lookup(keys), plain.lookup(keys)
            assert np.array_equal(got[0], exp[0])   # rows grouped in key-list order; inside a key, segment order
            for g, e in zip(_by_key(*got), _by_key(*exp)):
                assert np.array_equal(g, e)
        assert len(seg.lookup(absent)[0]) == 0
        k_all, s_all, o_all = want[:, 0].astype(np.uint32), want[:, 1].astype(np.uint32), want[:, 2].astype(np.uint32)
        for sid in (int(want[0, 1]), int(want[-1, 1]), 150):
            sel = s_all == sid
            assert seg.song_rows(sid) == plain.song_rows(sid) == int(sel.sum())
        # a match: queries made of rows of a few songs, shifted
        qk, qo, qoff = [], [], [0]
        for sid in (3, 150, 299):
            sel = np.flatnonzero(s_all == sid)[:300]
            qk.append(k_all[sel])
            qo.append((o_all[sel].astype(np.int64) + 5) % 4000)
            qoff.append(qoff[-1] + len(sel))
        qk, qo = np.concatenate(qk), np.concatenate(qo).astype(np.uint32)
        ra = seg.match(qk, qo, np.array(qoff, np.uint64), 3)
        rb = plain.match(qk, qo, np.array(qoff, np.uint64), 3)
        for name in rb:
            assert np.array_equal(ra[name], rb[name]), name
        assert list(ra["sid"][:, 0]) == [3, 150, 299]
    finally:
        seg.close()
        plain.close()
        plain_ctx.close()


def _run_ranks(world, fn):
    """fn(rank) on `world` threads; re-raises the first failure."""
    errs, outs = [None] * world, [None] * world

    def go(r):
        try:
            outs[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    ths = [threading.Thread(target=go, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(600)
    for e in errs:
        if e is not None:
            raise e
    return outs


@pytest.mark.parametrize("world", [2, 3])
def test_gathered_build_at_the_limit_over_thread_ranks(env, world):
    """Ranks (threads, one context each, all with the switch) stage L + 1, exactly L and 0 rows: every rank's table
    equals the one-rank build of all rows, and answers a match alike."""
    F, ctx, L = env
    sizes = [L + 1, L, 0][:world]
    rng = np.random.default_rng(90 + world)
    parts = [_rows(rng, n, L, False, 1 + 100 * r, 250 + 100 * r) for r, n in enumerate(sizes)]
    for a, src in zip(parts[1], parts[0]):   # rows both ranks stage (the ranks' song ids overlap as well)
        a[L - 40:L] = src[L - 40:L]
        a[:40] = src[:40]
    want = _want(*[p for p in parts if len(p[0])])
    one = F.Table(ctx)
    try:
        for p in parts:
            if len(p[0]):
                one.insert(*p)
        one.finalize()
        _assert_table(one, want)
        qk = np.concatenate([p[0][:: 97][:200] for p in parts if len(p[0])])
        qo = np.concatenate([p[2][:: 97][:200] for p in parts if len(p[0])])
        qoff = np.arange(0, len(qk) + 1, 200).astype(np.uint64)
        res_one = one.match(qk, qo, qoff, 3)
    finally:
        one.close()
    gid = 7700 + world

    def rank_fn(r):
        c = F.Context(0)
        c.set_debug(F.DEBUG_RUN_LIMIT_SMALL)
        comm = F.Comm.local(c, gid, r, world)
        tbl = F.Table(c)
        try:
            tbl.reserve(0, 0, gather=True)
            if sizes[r]:
                tbl.insert(*parts[r])
            tbl.allgather(comm)
            return _table_rows(tbl), tbl.rows(), tbl.match(qk, qo, qoff, 3)
        finally:
            tbl.close()
            comm.close()
            c.close()

    for r, (rows, nrows, res) in enumerate(_run_ranks(world, rank_fn)):
        assert nrows == (len(want), 0), r
        assert len(rows) == len(want) and np.array_equal(np.unique(rows, axis=0), want), r
        for name in res_one:
            assert np.array_equal(res[name], res_one[name]), (r, name)
