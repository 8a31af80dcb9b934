"""GPU: the match on query columns that already lie on the device (shz_match_device: the fused recognise and scan calls and
the listeners), reached through the tests / tools entry shz_match_device_host with a CHOSEN bound of the query offsets.
Every case is compared two ways: with oracle/cpu_ref.py (return_matches + vote: sid, delta, aligned, dedup, nhash, npairs)
and, element by element, with Table.match on the same arrays in host memory.  Where the route matters the counters of
shz_match_spec_stats are asserted too: (queued, used) = the one-workgroup fold was queued ahead of the vote count on the
layout the BOUND gives / its results were the answer.

What is expected of the route comes from include/shz.h (shz_match_batch: sb = bits(largest song id), dbits = bits(largest
table offset + bias); shz_match_device_host: the fold takes 1 + sb + dbits <= 32, dbits <= 20, topn <= 8, a bound < 2^20, one
query of at most 8,192 hashes, at most 32,768 votes) -- restated in _fits() below from the table's own numbers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("sid", "delta", "aligned", "dedup")


def _table(rng, n_songs, rows, hot_rows=0):
    """rows random (key, song, offset) rows over a small key alphabet + hot_rows rows under one popular key"""
    key = ((rng.integers(0, 600, rows) << 20) | (rng.integers(0, 40, rows) << 8) | rng.integers(0, 4, rows)).astype(np.uint32)
    sid = rng.integers(1, n_songs + 1, rows).astype(np.uint32)
    off = rng.integers(0, 900, rows).astype(np.uint32)
    hot = np.uint32((700 << 20) | (5 << 8) | 1)
    if hot_rows:
        key = np.concatenate([key, np.full(hot_rows, hot)])
        sid = np.concatenate([sid, rng.integers(1, n_songs + 1, hot_rows).astype(np.uint32)])
        off = np.concatenate([off, rng.integers(0, 900, hot_rows).astype(np.uint32)])
    return key, sid, off, hot


def _oracle_db(key, sid, off, n_songs):
    from oracle import cpu_ref as O
    odb = O.DictDB()
    for s in range(1, n_songs + 1):
        odb.insert_song(str(s), "00", 1)
    by_song = {}
    for k, s, o in zip(key.tolist(), sid.tolist(), off.tolist()):
        by_song.setdefault(s, []).append((k, o))
    for s, hs in by_song.items():
        odb.insert_hashes(s, hs)
    return odb


def _check(res, q, qk, qo, odb, topn):
    from oracle import cpu_ref as O
    hs = set(zip(qk.tolist(), qo.tolist()))
    m, dd = O.return_matches(hs, odb)
    want = O.vote(m, topn)
    got = [(int(res["sid"][q, i]), int(res["delta"][q, i]), int(res["aligned"][q, i])) for i in range(int(res["nres"][q]))]
    assert got == [tuple(w) for w in want]
    assert [int(res["dedup"][q, i]) for i in range(len(got))] == [dd[w[0]] for w in want]
    assert int(res["npairs"][q]) == len(m) and int(res["nhash"][q]) == len(hs)
    return len(m)


def _same(a, b, qa=0, qb=0):
    n = int(a["nres"][qa])
    assert n == int(b["nres"][qb])
    for f in FIELDS:
        assert np.array_equal(a[f][qa, :n], b[f][qb, :n]), f
    assert int(a["npairs"][qa]) == int(b["npairs"][qb]) and int(a["nhash"][qa]) == int(b["nhash"][qb])


def _same_all(a, b):
    """every query of two results: counters whole, the result rows up to nres"""
    for f in ("nres", "nhash", "npairs"):
        assert np.array_equal(a[f], b[f]), f
    valid = np.arange(a["sid"].shape[1])[None, :] < a["nres"][:, None]
    for f in FIELDS:
        assert a[f].shape == b[f].shape and np.array_equal(a[f][valid], b[f][valid]), f


def _bits(v):
    return max(int(v).bit_length(), 1)


def _fits(max_sid, max_off, bound, topn):
    """include/shz.h at shz_match_device_host: the layout of the bound is one the one-workgroup fold takes"""
    dbits = _bits(max_off + bound)
    return bound < (1 << 20) and topn <= 8 and dbits <= 20 and 1 + _bits(max_sid) + dbits <= 32


class _Stats:
    """the (queued, used) counters since the last look"""

    def __init__(self, ctx):
        self.ctx, self.last = ctx, ctx.spec_stats()

    def delta(self):
        now = self.ctx.spec_stats()
        d = (now[0] - self.last[0], now[1] - self.last[1])
        self.last = now
        return d


@pytest.fixture(scope="module")
def env():
    """a 40,000-row table, its oracle, and ONE query of 1,200 hashes: 500 of song 18's rows moved by 40 frames (the true
    match) + 700 random hashes.  M: its largest offset."""
    import shazam_amd as S
    ctx = S.get_context(0)
    rng = np.random.default_rng(4242)
    n_songs = 300
    key, sid, off, _ = _table(rng, n_songs, 40000)
    t = S.Table(ctx)
    t.insert(key, sid, off)
    t.finalize()
    odb = _oracle_db(key, sid, off, n_songs)
    own = np.flatnonzero((sid == 18) & (off >= 40))[:500]
    qk = np.concatenate([key[own], key[rng.integers(0, len(key), 700)]])
    qo = np.concatenate([off[own] - 40, rng.integers(0, 300, 700).astype(np.uint32)]).astype(np.uint32)
    e = {"S": S, "ctx": ctx, "t": t, "odb": odb, "key": key, "sid": sid, "off": off, "qk": qk, "qo": qo,
         "qoff": np.array([0, len(qk)], np.uint64), "M": int(qo.max()), "max_sid": int(sid.max()), "max_off": int(off.max()),
         "rng": rng, "host": {}}
    for topn in (1, 3, 8):   # the host-memory reference of every single-query case, computed once
        e["host"][topn] = t.match(qk, qo, e["qoff"], topn)
    yield e
    t.close()


def _bounds(e):
    """-1, M, M + 1, either side of the next bit of max_off + bound, either side of dbits = 20 | 21, 2^20 - 1, 2^20,
    2^32 - 1, 2^32"""
    M, mo = e["M"], e["max_off"]
    nxt = 1 << _bits(mo + M + 1)                  # the first power of two above max_off + M + 1
    out = [-1, M, M + 1, nxt - 1 - mo, nxt - mo, (1 << 20) - 1 - mo, (1 << 20) - mo, (1 << 20) - 1, 1 << 20, (1 << 32) - 1,
           1 << 32]
    assert _bits(mo + out[3]) + 1 == _bits(mo + out[4]) and out[3] >= M + 1
    assert _bits(mo + out[5]) == 20 and _bits(mo + out[6]) == 21
    return out


def test_the_host_reference_equals_the_oracle(env):
    e = env
    for topn in (1, 3, 8):
        votes = _check(e["host"][topn], 0, e["qk"], e["qo"], e["odb"], topn)
        assert 0 < votes <= 32768
    assert int(e["host"][3]["sid"][0, 0]) == 18 and int(e["host"][3]["delta"][0, 0]) == 40


def test_one_query_over_a_sweep_of_bounds(env):
    """the same arrays for every bound; queued and used exactly where the header says"""
    e = env
    st = _Stats(e["ctx"])
    topn = 3
    seen = set()
    for b in _bounds(e):
        res = e["t"].match_device(e["qk"], e["qo"], e["qoff"], topn, bias_bound=b)
        d = st.delta()
        no_bound = b < 0 or b >= (1 << 32)
        want = (1, 1) if not no_bound and _fits(e["max_sid"], e["max_off"], b, topn) else (0, 0)
        assert d == want, (b, d, want)
        seen.add(want)
        _check(res, 0, e["qk"], e["qo"], e["odb"], topn)
        _same_all(res, e["host"][topn])
    assert seen == {(0, 0), (1, 1)}


@pytest.mark.parametrize("topn", [1, 3, 8])
def test_topn_and_the_full_sort(env, topn):
    e = env
    st = _Stats(e["ctx"])
    for b, full, want in ((e["M"], False, (1, 1)), (e["M"] + 7, False, (1, 1)), (-1, False, (0, 0)), (e["M"], True, (0, 0))):
        res = e["t"].match_device(e["qk"], e["qo"], e["qoff"], topn, full_sort=full, bias_bound=b)
        assert st.delta() == want, (b, full)
        _check(res, 0, e["qk"], e["qo"], e["odb"], topn)
        _same_all(res, e["host"][topn])
    # more results than the fold ranks: never queued, same answer as the host's
    res9 = e["t"].match_device(e["qk"], e["qo"], e["qoff"], 9, bias_bound=e["M"])
    assert st.delta() == (0, 0)
    _check(res9, 0, e["qk"], e["qo"], e["odb"], 9)
    _same_all(res9, e["t"].match(e["qk"], e["qo"], e["qoff"], 9))


def test_more_votes_than_the_queued_fold_takes(env):
    """the hot-key table of test_gpu_single_query.py: queued on the bound, the kernels do nothing, the passes answer"""
    S, ctx = env["S"], env["ctx"]
    rng = np.random.default_rng(7)
    n_songs = 2000
    key, sid, off, hot = _table(rng, n_songs, 60000, hot_rows=50000)
    t = S.Table(ctx)
    t.insert(key, sid, off)
    t.finalize()
    odb = _oracle_db(key, sid, off, n_songs)
    qk = np.concatenate([np.array([hot, hot], np.uint32), key[rng.integers(0, 60000, 300)]])
    qo = np.concatenate([np.array([3, 11], np.uint32), rng.integers(0, 200, 300).astype(np.uint32)])
    qoff = np.array([0, len(qk)], np.uint64)
    b = int(qo.max()) + 1
    assert _fits(int(sid.max()), int(off.max()), b, 5)
    st = _Stats(ctx)
    res = t.match_device(qk, qo, qoff, 5, bias_bound=b)   # (the table's first match: no vote estimate yet keeps it from queueing)
    assert st.delta() == (1, 0)
    assert _check(res, 0, qk, qo, odb, 5) > 32768
    _same_all(res, t.match(qk, qo, qoff, 5))
    t.close()


@pytest.mark.parametrize("m", [8192, 8193])
def test_either_side_of_the_one_workgroup_head(env, m):
    """8,192 hashes is the most the one-workgroup head and with it the queued fold take.  A fresh table: no earlier match
    has left a vote estimate that would keep the call from queueing."""
    S, ctx = env["S"], env["ctx"]
    rng = np.random.default_rng(8000 + m)
    n_songs = 300
    key, sid, off, _ = _table(rng, n_songs, 40000)
    t = S.Table(ctx)
    t.insert(key, sid, off)
    t.finalize()
    odb = _oracle_db(key, sid, off, n_songs)
    pick = rng.integers(0, len(key), m)
    qk, qo = key[pick], (off[pick] % 300).astype(np.uint32)
    qoff = np.array([0, m], np.uint64)
    st = _Stats(ctx)
    res = t.match_device(qk, qo, qoff, 4, bias_bound=299)
    d = st.delta()
    votes = _check(res, 0, qk, qo, odb, 4)
    assert d == ((1, 1 if votes <= 32768 else 0) if m <= 8192 else (0, 0)), (d, votes)
    _same_all(res, t.match(qk, qo, qoff, 4))
    t.close()


def test_every_hash_twice(env):
    """two identical channels of a listener: every (key, offset) appears twice; nhash counts the distinct ones"""
    e = env
    qk, qo = np.concatenate([e["qk"], e["qk"]]), np.concatenate([e["qo"], e["qo"]])
    qoff = np.array([0, len(qk)], np.uint64)
    st = _Stats(e["ctx"])
    for b, want in ((e["M"], (1, 1)), (-1, (0, 0))):
        res = e["t"].match_device(qk, qo, qoff, 3, bias_bound=b)
        assert st.delta() == want
        _check(res, 0, qk, qo, e["odb"], 3)
        assert int(res["nhash"][0]) == len(set(zip(e["qk"].tolist(), e["qo"].tolist()))) <= len(e["qk"])
        _same_all(res, e["host"][3])          # ... and the same as the query given once
    # interleaved instead of appended
    res = e["t"].match_device(np.repeat(e["qk"], 2), np.repeat(e["qo"], 2), qoff, 3, bias_bound=e["M"])
    _same_all(res, e["host"][3])


def _batch(e, rng, nq):
    """nq queries of 0 to 3 hashes (half of them keys of the table), empty ones first, in the middle and last, and the
    module's real query in one place"""
    sizes = rng.integers(0, 4, nq)
    sizes[[0, nq // 2, nq - 1]] = 0
    real = nq // 3 if nq > 2 else 1
    ks, os_ = [], []
    for q in range(nq):
        if q == real:
            ks.append(e["qk"])
            os_.append(e["qo"])
            continue
        n = int(sizes[q])
        k = e["key"][rng.integers(0, len(e["key"]), n)].copy()
        absent = rng.random(n) < 0.5
        k[absent] = ((900 + rng.integers(0, 50, int(absent.sum()))) << 20).astype(np.uint32) | np.uint32(1 << 8)
        ks.append(k)
        os_.append(rng.integers(0, 500, n).astype(np.uint32))
    lens = np.array([len(k) for k in ks])
    qoff = np.zeros(nq + 1, np.uint64)
    qoff[1:] = np.cumsum(lens)
    return ks, os_, np.concatenate(ks).astype(np.uint32), np.concatenate(os_).astype(np.uint32), qoff, real


@pytest.mark.parametrize("nq", [2, 65, 4097])
def test_batches(env, nq):
    """more than one query never queues; 4,097 is one more than a sub-batch holds"""
    e = env
    rng = np.random.default_rng(600 + nq)
    ks, os_, qk, qo, qoff, real = _batch(e, rng, nq)
    host = e["t"].match(qk, qo, qoff, 2)
    st = _Stats(e["ctx"])
    sample = set(rng.choice(nq, min(nq, 32), replace=False).tolist()) | {0, nq // 2, nq - 1, real}
    sample |= set(np.flatnonzero(host["nres"]).tolist())
    for q in sorted(sample):
        _check(host, q, ks[q], os_[q], e["odb"], 2)
    assert int(host["sid"][real, 0]) == 18 and int(host["delta"][real, 0]) == 40
    for q in {0, nq // 2, nq - 1} - {real}:
        assert int(host["nres"][q]) == 0 and int(host["nhash"][q]) == 0
    for b in (int(qo.max()), -1):
        res = e["t"].match_device(qk, qo, qoff, 2, bias_bound=b)
        assert st.delta() == (0, 0)
        _same_all(res, host)


def test_the_unpacked_upload(env):
    """524,300 queries: segment descriptors + query_off + control block pass 4 MiB, so they travel apart and every
    sub-batch uploads its own query offsets.  Against the host match only."""
    e = env
    nq = 524300
    assert 256 + ((nq + 1) * 8 + 255) // 256 * 256 + 256 > 4 << 20     # (one segment: 256 bytes of descriptors at the least)
    rng = np.random.default_rng(52)
    lens = np.zeros(nq, np.int64)
    some = rng.choice(nq, 600, replace=False)
    lens[some] = rng.integers(1, 4, len(some))
    lens[[0, nq - 1]] = 0
    real = 4096 * 100 + 17
    lens[real] = len(e["qk"])
    qoff = np.zeros(nq + 1, np.uint64)
    qoff[1:] = np.cumsum(lens)
    n = int(qoff[-1])
    qk = e["key"][rng.integers(0, len(e["key"]), n)].copy()
    qo = rng.integers(0, 500, n).astype(np.uint32)
    a = int(qoff[real])
    qk[a:a + len(e["qk"])] = e["qk"]
    qo[a:a + len(e["qk"])] = e["qo"]
    host = e["t"].match(qk, qo, qoff, 2)
    assert int(host["sid"][real, 0]) == 18 and int(host["delta"][real, 0]) == 40
    assert np.count_nonzero(host["nres"]) > 300
    _same(host, e["t"].match(e["qk"], e["qo"], e["qoff"], 2), real, 0)
    for b in (int(qo.max()), -1):
        _same_all(e["t"].match_device(qk, qo, qoff, 2, bias_bound=b), host)


def test_edges_and_refusals(env):
    from shazam_amd import _ffi
    e, S, ctx, t = env, env["S"], env["ctx"], env["t"]
    none = np.zeros(0, np.uint32)
    st = _Stats(ctx)
    # no query at all; one query without hashes
    for b in (5, -1):
        res = t.match_device(none, none, np.array([0], np.uint64), 3, bias_bound=b)
        assert res["nres"].shape == (0,) and res["sid"].shape == (0, 3)
        res = t.match_device(none, none, np.array([0, 0], np.uint64), 3, bias_bound=b)
        assert (int(res["nres"][0]), int(res["nhash"][0]), int(res["npairs"][0])) == (0, 0, 0)
    assert st.delta() == (0, 0)
    # an empty finalised table
    empty = S.Table(ctx)
    empty.finalize()
    for b in (e["M"], -1):
        res = empty.match_device(e["qk"], e["qo"], e["qoff"], 3, bias_bound=b)
        assert (int(res["nres"][0]), int(res["npairs"][0])) == (0, 0)
        assert int(res["nhash"][0]) == len(set(zip(e["qk"].tolist(), e["qo"].tolist())))
        _same_all(res, empty.match(e["qk"], e["qo"], e["qoff"], 3))
    empty.close()
    # a query offset of 2^20 in the device column: as for host input, with a (true) bound and without
    qo = e["qo"].copy()
    qo[77] = 1 << 20
    with pytest.raises(_ffi.ShzError) as err:
        t.match(e["qk"], qo, e["qoff"], 3)
    assert err.value.code == _ffi.E_UNSUPPORTED
    for b in (1 << 20, -1):
        with pytest.raises(_ffi.ShzError) as err:
            t.match_device(e["qk"], qo, e["qoff"], 3, bias_bound=b)
        assert err.value.code == _ffi.E_UNSUPPORTED
    # ... in the second of two queries, and 2^20 - 1 is taken
    two = np.array([0, 5, len(qo)], np.uint64)
    with pytest.raises(_ffi.ShzError) as err:
        t.match_device(e["qk"], qo, two, 3, bias_bound=1 << 20)
    assert err.value.code == _ffi.E_UNSUPPORTED
    qo[77] = (1 << 20) - 1
    res = t.match_device(e["qk"], qo, e["qoff"], 3, bias_bound=(1 << 20) - 1)
    _check(res, 0, e["qk"], qo, e["odb"], 3)
    _same_all(res, t.match(e["qk"], qo, e["qoff"], 3))
    # topn outside [1, 64]
    for topn in (0, 65):
        with pytest.raises(_ffi.ShzError) as err:
            t.match_device(e["qk"], e["qo"], e["qoff"], topn, bias_bound=e["M"])
        assert err.value.code == _ffi.E_INVALID
    # a table that is not finalised: never, and with rows waiting
    raw = S.Table(ctx)
    for rows in (False, True):
        if rows:
            raw.insert(e["key"][:100], e["sid"][:100], e["off"][:100])
        with pytest.raises(_ffi.ShzError) as err:
            raw.match_device(e["qk"], e["qo"], e["qoff"], 3, bias_bound=e["M"])
        assert err.value.code == _ffi.E_STATE
    raw.close()
    # and the table answers as before
    _same_all(t.match_device(e["qk"], e["qo"], e["qoff"], 3, bias_bound=e["M"]), e["host"][3])


def test_host_and_device_matches_in_turn_share_the_workspace(env):
    """the device path keeps its packed upload in another workspace slot than the host path keeps its own: calls of the
    two kinds in any order give the arrays they gave before"""
    e = env
    rng = np.random.default_rng(99)
    _, _, bk, bo, boff, _ = _batch(e, rng, 65)
    one_h = e["host"][3]
    many_h = e["t"].match(bk, bo, boff, 3)
    for _ in range(2):
        _same_all(e["t"].match_device(e["qk"], e["qo"], e["qoff"], 3, bias_bound=e["M"]), one_h)
        _same_all(e["t"].match(bk, bo, boff, 3), many_h)
        _same_all(e["t"].match_device(bk, bo, boff, 3, bias_bound=int(bo.max())), many_h)
        _same_all(e["t"].match(e["qk"], e["qo"], e["qoff"], 3), one_h)
        _same_all(e["t"].match_device(bk, bo, boff, 3), many_h)
        _same_all(e["t"].match_device(e["qk"], e["qo"], e["qoff"], 3), one_h)


def test_a_bound_that_does_not_hold(env):
    """bias_bound below the largest offset: the fold is queued on the bound's layout, the read-back shows an offset above
    it, its results are dropped and the vote passes answer.  (Safe to run: in m_expand_chunk / m_vote the wrapped
    off + bias - q_off only enters the vote's key bits -- every index there comes from the pair number and the prefix
    sums -- and vt_fold_kernel / vt_rank_kernel reach their tables through hashes masked to the table size and write
    results by rank, never by a field of the vote.)"""
    e = env
    assert e["M"] > 1 and int(e["qo"].min()) < e["M"]
    st = _Stats(e["ctx"])
    for b in (e["M"] - 1, 0):
        for topn in (3, 8):
            res = e["t"].match_device(e["qk"], e["qo"], e["qoff"], topn, bias_bound=b)
            assert st.delta() == (1, 0), b
            _check(res, 0, e["qk"], e["qo"], e["odb"], topn)
            _same_all(res, e["host"][topn])
