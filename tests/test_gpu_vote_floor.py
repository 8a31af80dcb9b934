"""GPU: the vote floor (Context.floor, Table.match(floor=True)) -- per query the exact histograms of how many single bins and
how many songs reached which count -- on tables and queries built by hand, against its plain-Python definition
(tests/vote_floor_twin.py): bucket edges, runs and blocks of every quantum of the kernels, query borders with and without
SHZ_DEBUG_FLOOR_SMALL, the identities of the definition, that no result array changes, the state of the row store, and every
door the rows come through.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from vote_floor_twin import bucket_of, expected_floor
from vote_tol_twin import assert_match, expected_match

pytestmark = pytest.mark.gpu

N_SONGS = 32
ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
SR = 44100


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


class Built:
    """A table and queries from single votes: vote(q, sid, delta, n) adds n votes of query q for song sid at offset difference
    delta, each through a key of its own (one row, one query hash)."""

    def __init__(self, n_queries=1, q_base=40):
        self.rows, self.hashes, self.key, self.q_base = [], [[] for _ in range(n_queries)], 0, q_base

    def vote(self, q, sid, delta, n=1, q_off=None):
        for _ in range(n):
            self.key += 1
            qo = self.q_base if q_off is None else q_off
            assert qo + delta >= 0
            self.rows.append((self.key, sid, qo + delta))
            self.hashes[q].append((self.key, qo))

    def bins(self, q, sid, bins):
        for d, n in bins.items():
            self.vote(q, sid, d, n)

    def miss(self, q, n=1):
        """n hashes of query q that match nothing"""
        for _ in range(n):
            self.key += 1
            self.hashes[q].append((self.key, self.q_base))

    def arrays(self):
        tk, ts, to = (np.asarray([r[i] for r in self.rows], np.uint32) for i in range(3))
        qk = np.asarray([h[0] for hs in self.hashes for h in hs], np.uint32)
        qo = np.asarray([h[1] for hs in self.hashes for h in hs], np.uint32)
        qoff = np.cumsum([0] + [len(hs) for hs in self.hashes]).astype(np.uint64)
        return tk, ts, to, qk, qo, qoff

    def table(self, S, ctx):
        tk, ts, to, *_ = self.arrays()
        t = S.Table(ctx)
        t.insert(tk, ts, to)
        t.finalize()
        return t


def _same(a, b, what=""):
    for name in ARRAYS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


def _hist_eq(res, want, what=""):
    sh, bh = want
    assert res["song_hist"].dtype == np.uint32 and res["song_hist"].shape == sh.shape == res["bin_hist"].shape, what
    bad = np.flatnonzero((res["song_hist"] != sh).any(axis=1) | (res["bin_hist"] != bh).any(axis=1))
    assert bad.size == 0, (what, "query", int(bad[0]), res["song_hist"][bad[0]].tolist(), sh[bad[0]].tolist(),
                           res["bin_hist"][bad[0]].tolist(), bh[bad[0]].tolist())


def _check(S, ctx, b, tols=(0,), topn=3, debugs=(0,), what="", t=None):
    """Table.match(floor=True) against the twin at every tolerance, under every debug setting; the other arrays against the
    floor=False call's.  Returns the results by tolerance."""
    tk, ts, to, qk, qo, qoff = b.arrays()
    own = t is None
    t = b.table(S, ctx) if own else t
    out = {}
    try:
        for tol in tols:
            want = expected_floor(tk, ts, to, qk, qo, qoff, tol)
            plain = t.match(qk, qo, qoff, topn, delta_tol=tol)
            for dbg in debugs:
                ctx.set_debug(dbg)
                try:
                    res = t.match(qk, qo, qoff, topn, delta_tol=tol, floor=True)
                finally:
                    ctx.set_debug(0)
                _hist_eq(res, want, (what, tol, dbg))
                _same(res, plain, (what, tol, dbg))
                assert ctx.floor_rows() == 0 and not ctx.vote_floor and ctx.vote_tolerance == 0
                out[tol] = res
    finally:
        if own:
            t.close()
    return out


# ---- 1. bucket edges ---------------------------------------------------------------------------------------------------
def test_bucket_edges(S, ctx):
    counts = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 4095, 4096)
    b = Built()
    for i, c in enumerate(counts):
        b.vote(0, 1 + i, 3 * i - 7, c)
    b.bins(0, 20, {10: 16, 11: 1})       # best count 16 at tolerance 0 (bucket 15), window sum 17 at tolerance 1 (bucket 16)
    b.bins(0, 21, {5: 31, 6: 1})         # 31 (bucket 16) and 32 (bucket 17)
    r = _check(S, ctx, b, (0, 1, 31), what="edges")
    sh0, sh1 = r[0]["song_hist"][0], r[1]["song_hist"][0]
    assert sh0[15] == 2 and sh0[16] == 3 and sh0[17] == 3 and sh0[18] == 1 and sh0[23] == 1 and sh0[24] == 1
    assert sh1[15] == 1 and sh1[16] == 3 and sh1[17] == 4
    assert np.array_equal(r[0]["bin_hist"], r[1]["bin_hist"]) and np.array_equal(r[0]["bin_hist"], r[31]["bin_hist"])
    assert r[0]["bin_hist"][0, 0] == 3   # the bins of one vote: count 1, and the two neighbours


# ---- 2. run and block borders --------------------------------------------------------------------------------------------
def test_run_starts_at_every_quantum(S, ctx):
    """One query, one song, bins in ascending delta: run i starts at the sum of the counts before it.  Runs start at the
    sorted-vote indices 7, 8, 9, 511, 512, 513, 2047, 2048, 2049 (the fold's thread, wave and workgroup quanta); the
    histogram kernels go by RUNS, 256 a workgroup: 600 more runs of one vote put the run indices 255, 256, 257, 511, 512,
    513 on borders too, then a run of 40,000 votes between runs of one, and the call ends where a block ends: 768 runs
    in all, 49,152 votes (a multiple of 2,048)."""
    counts = [7, 1, 1, 502, 1, 1, 1534, 1, 1]
    starts = np.cumsum([0] + counts)
    assert starts[1:].tolist() == [7, 8, 9, 511, 512, 513, 2047, 2048, 2049]
    counts += [1] * 600 + [40000] + [1] * 100
    counts += [1] * (768 - len(counts) - 1)
    counts.append(49152 - sum(counts))
    assert len(counts) == 768 and sum(counts) % 2048 == 0 and counts[-1] > 1
    b = Built(q_base=0)
    for i, c in enumerate(counts):
        b.vote(0, 5, 2 * i, c)
    r = _check(S, ctx, b, (0, 1, 2), debugs=(0, 1024), what="quanta")
    assert int(r[0]["bin_hist"][0].sum()) == 768 and int(r[0]["song_hist"][0].sum()) == 1
    assert r[0]["song_hist"][0, bucket_of(40000)] == 1


def test_large_runs_and_one_key_group(S, ctx):
    """Runs of 40,000 votes flanked by runs of one; one key with 200 rows x 200 query offsets: 399 bins with the counts
    1 .. 200 .. 1, a group of 399 runs over two workgroups of the histogram kernels."""
    b = Built(q_base=300)
    b.vote(0, 1, 5)
    b.bins(0, 2, {50: 1, 51: 40000, 52: 1})
    b.vote(0, 3, -8, 40000)
    b.vote(0, 4, -2)
    b.rows.extend(((1 << 30), 5, 1000 + i) for i in range(200))
    b.hashes[0].extend(((1 << 30), 50 + j) for j in range(200))
    b.vote(0, 9, 0)
    r = _check(S, ctx, b, (0, 1, 31), topn=8, debugs=(0, 1024), what="large")
    bh = r[0]["bin_hist"][0]
    assert bh[bucket_of(40000)] == 2 and bh[bucket_of(200)] == 1 + 2 * (199 - 127)
    assert int(bh.sum()) == 1 + 3 + 1 + 1 + 399 + 1
    assert int(r[0]["npairs"][0]) == 40002 + 40000 + 40000 + 3


# ---- 3. query borders ----------------------------------------------------------------------------------------------------
def _many_queries(nq, seed):
    """nq queries: most with a few votes; every 5th without hashes, every 7th with hashes that match nothing; query 2's last
    bin and query 3's first bin are the same (song 5, delta 3) -- they must not join; query 9 has 700 bins and about 2,000 votes,
    several workgroups of the fold and of the histogram kernels, between one-vote queries."""
    rng = np.random.default_rng(seed)
    b = Built(n_queries=nq)
    for q in range(nq):
        if q == 2:
            b.vote(q, 1, 0)
            b.vote(q, 5, 3, 2)
        elif q == 3:
            b.vote(q, 5, 3, 3)
            b.vote(q, 7, -1)
        elif q in (8, 10):
            b.vote(q, 2, 11)
        elif q == 9:
            for i in range(700):
                b.vote(q, 1 + i // 350, 5 * (i % 350) - 40, 1 + (i % 50 == 0) * 87 + (i % 7 == 0))
        elif q % 5 == 4:
            continue
        elif q % 7 == 6:
            b.miss(q, 3)
        else:
            for _ in range(int(rng.integers(1, 4))):
                b.vote(q, int(rng.integers(1, 9)), int(rng.integers(-3, 4)), int(rng.integers(1, 4)))
            b.miss(q)
    return b


@pytest.mark.parametrize("nq", [17, 300])
def test_query_borders(S, ctx, nq):
    b = _many_queries(nq, 70 + nq)
    tk, ts, to, qk, qo, qoff = b.arrays()
    r = _check(S, ctx, b, (0, 2), debugs=(0, 1024), what=("queries", nq))
    for tol in (0, 2):
        sh, bh = r[tol]["song_hist"], r[tol]["bin_hist"]
        assert sh.shape == (nq, 32)
        assert bh[2, 1] == 1 and bh[2, 0] == 1 and bh[3, 2] == 1 and not bh[2:4, 4].any()     # 2 and 3 votes, never 5
        for q in range(nq):
            if q not in (2, 3, 8, 9, 10) and (q % 5 == 4 or q % 7 == 6):
                assert not sh[q].any() and not bh[q].any(), q
        assert int(bh[9].sum()) == 700 and int(sh[9].sum()) == 2 and int(sh[8].sum()) == 1 == int(sh[10].sum())


# ---- 4. identities, and no side effect ---------------------------------------------------------------------------------------
def _crowded(rng, nq):
    keys = rng.choice(1 << 31, 32, replace=False).astype(np.uint32)
    n_rows = 700
    tk, ts, to = keys[rng.integers(0, 32, n_rows)], rng.integers(1, 9, n_rows).astype(np.uint32), rng.integers(0, 64, n_rows).astype(np.uint32)
    qk = keys[rng.integers(0, 32, 500 * nq)]
    qo = rng.integers(0, 64, 500 * nq).astype(np.uint32)
    return tk, ts, to, qk, qo, (np.arange(nq + 1) * 500).astype(np.uint64)


def test_identities_and_unchanged_results(S, ctx):
    b = _many_queries(17, 5)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    vb = np.vectorize(bucket_of)
    for tol in (0, 3):
        with ctx.tolerance(tol):
            plain = t.match(qk, qo, qoff, 16)
            res = t.match(qk, qo, qoff, 16, floor=True)
            _same(res, plain, ("floor", tol))
            for name, other in (("full_sort", t.match(qk, qo, qoff, 16, full_sort=True, floor=True)),
                                ("device", t.match_device(qk, qo, qoff, 16, floor=True)),
                                ("device, bound", t.match_device(qk, qo, qoff, 16, bias_bound=40, floor=True))):
                _same(other, plain, (name, tol))
                assert np.array_equal(other["song_hist"], res["song_hist"]) and np.array_equal(other["bin_hist"], res["bin_hist"]), name
            _same(t.match(qk, qo, qoff, 16, full_sort=True), plain, ("full_sort plain", tol))
            _same(t.match_device(qk, qo, qoff, 16, bias_bound=40), plain, ("device plain", tol))
            assert ctx.vote_tolerance == tol and not ctx.vote_floor and ctx.floor_rows() == 0
        sh, bh = res["song_hist"], res["bin_hist"]
        for q in range(17):
            n = int(res["nres"][q])
            assert n < 16 and int(sh[q].sum()) == n                      # topn above the songs with a vote: all are listed
            col = np.bincount(vb(res["aligned"][q, :n]), minlength=32) if n else np.zeros(32, np.int64)
            assert col.tolist() == sh[q].tolist(), (tol, q)
            if q != 9:                                                     # every bin count <= 16
                assert not bh[q, 16:].any()
                assert int((np.arange(1, 33) * bh[q].astype(np.int64)).sum()) == int(res["npairs"][q]), (tol, q)
    assert ctx.vote_tolerance == 0
    # a single query, the route the queued one-workgroup fold would take with the floor off
    one = np.array([0, int(qoff[1])], np.uint64)
    a, e = t.match(qk[:int(qoff[1])], qo[:int(qoff[1])], one, 4), t.match(qk[:int(qoff[1])], qo[:int(qoff[1])], one, 4, floor=True)
    _same(e, a, "one query")
    _hist_eq(e, expected_floor(tk, ts, to, qk[:int(qoff[1])], qo[:int(qoff[1])], one, 0), "one query")
    t.close()


# ---- 5. fuzz -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 17])
@pytest.mark.parametrize("seed", range(2))
def test_random_fuzz_with_crowded_bins(S, ctx, seed, nq):
    """8 songs, 32 distinct keys, offsets below 64, queries of 500 hashes: every (query, song) group fills most of its bins"""
    tk, ts, to, qk, qo, qoff = _crowded(np.random.default_rng(1900 + 10 * seed + nq), nq)
    t = S.Table(ctx)
    t.insert(tk, ts, to)
    t.finalize()
    for tol in (0, 1, 5, 31):
        res = t.match(qk, qo, qoff, 5, delta_tol=tol, floor=True)
        _hist_eq(res, expected_floor(tk, ts, to, qk, qo, qoff, tol), (seed, nq, tol))
        assert_match(res, expected_match(tk, ts, to, qk, qo, qoff, tol, 5), (seed, nq, tol))
    t.close()


# ---- 6. state --------------------------------------------------------------------------------------------------------------
def test_state_of_the_row_store(S, ctx):
    from shazam_amd import _ffi
    lib = _ffi.lib()
    b = _many_queries(17, 6)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    want = expected_floor(tk, ts, to, qk, qo, qoff, 0)
    assert not ctx.vote_floor
    t.match(qk, qo, qoff, 2)
    assert ctx.floor_rows() == 0                                        # off: nothing recorded
    ctx.set_vote_floor(True)
    try:
        assert ctx.vote_floor
        t.match(qk, qo, qoff, 2)
        assert ctx.floor_rows() == 17
        half = np.array(qoff[:6] - qoff[0], np.uint64)                   # the first 5 queries again
        t.match(qk[:int(qoff[5])], qo[:int(qoff[5])], half, 2)
        assert ctx.floor_rows() == 22                                   # two calls: the rows accumulate, in order
        sh, bh, n = np.full((4, 32), 9, np.uint32), np.full((4, 32), 9, np.uint32), C.c_uint64()
        rc = lib.shz_vote_floor_take(ctx.h, _ffi.ptr(sh), _ffi.ptr(bh), 4, C.byref(n))
        assert rc == _ffi.E_CAPACITY and n.value == 22 and (sh == 9).all() and (bh == 9).all() and ctx.floor_rows() == 22
        with pytest.raises(_ffi.ShzError):                                # a refused match records nothing, changes nothing
            t.match(qk, qo, qoff, 0)
        assert ctx.floor_rows() == 22 and ctx.vote_floor
        sh, bh = ctx.take_floor()
        assert sh.shape == (22, 32) and ctx.floor_rows() == 0
        assert np.array_equal(sh[:17], want[0]) and np.array_equal(bh[:17], want[1])
        assert np.array_equal(sh[17:], want[0][:5]) and np.array_equal(bh[17:], want[1][:5])
        t.match(qk, qo, qoff, 2)
        assert ctx.floor_rows() == 17
        ctx.set_vote_floor(False)                                        # off: the rows are dropped
        assert ctx.floor_rows() == 0 and not ctx.vote_floor
        # floor(): the previous state comes back and nothing is left over, after an exception too
        ctx.set_vote_floor(True)
        with pytest.raises(ZeroDivisionError):
            with ctx.floor():
                t.match(qk, qo, qoff, 2)
                1 / 0
        assert ctx.vote_floor and ctx.floor_rows() == 0
    finally:
        ctx.set_vote_floor(False)
        t.close()


# ---- 7. doors --------------------------------------------------------------------------------------------------------------
def test_sharded_table_gives_the_unsharded_histograms(S, ctx):
    from shazam_amd.shard import ShardedTable
    b = _many_queries(17, 7)
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    st = ShardedTable(ctx, nshards=3)
    st.insert(tk, ts, to)
    st.finalize()
    try:
        for tol in (0, 2):
            one = t.match(qk, qo, qoff, 3, delta_tol=tol, floor=True)
            got = st.match(qk, qo, qoff, 3, delta_tol=tol, floor=True)
            _same(got, one, ("sharded", tol))
            _hist_eq(got, (one["song_hist"], one["bin_hist"]), ("sharded", tol))
            _same(st.match(qk, qo, qoff, 3, delta_tol=tol), one, ("sharded plain", tol))
            assert not ctx.vote_floor and ctx.floor_rows() == 0 and ctx.vote_tolerance == 0
    finally:
        st.close()
        t.close()


@pytest.fixture(scope="module")
def music(S, ctx):
    """32 music-like songs of 6 s in a database (ids 1..32), and the clips: enough songs that a query's song histogram has a
    tail to fit."""
    from oracle import synth
    songs = [synth.music_clip(11, c, 6 * SR) for c in range(N_SONGS)]
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    for c in range(N_SONGS):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        d.set_song_fingerprinted(sid)
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    yield d, songs
    d.close()


def _floor_eq(a, b):
    return (a.keys() == b.keys() and np.array_equal(a["song_hist"], b["song_hist"]) and np.array_equal(a["bin_hist"], b["bin_hist"])
            and a["expected_above"] == b["expected_above"] and a["score"] == b["score"])


def test_recognize_batch_both_paths(S, ctx, music):
    from oracle import synth
    from shazam_amd import floor
    db, songs = music
    noise = synth.traffic_noise(5, 3, 4 * SR)
    queries = [songs[1][SR:5 * SR], [songs[2][2 * SR:6 * SR], synth.mix_query(songs[2][2 * SR:6 * SR], noise, 6.0)],
               songs[0][0:3 * SR]]
    for tol in (None, 2):
        plain, _ = S.recognize_batch(queries, db, topn=3, delta_tol=tol)
        two, _ = S.recognize_batch(queries, db, topn=3, floor=True, delta_tol=tol)
        fused, _ = S.recognize_batch(queries, db, topn=3, fused=True, floor=True, delta_tol=tol)
        chans = [queries[0], queries[1][0], queries[1][1], queries[2]]
        k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
        res = db.table.match(k, t1, ho[[0, 1, 3, 4]], 3, delta_tol=tol, floor=True)
        for q in range(3):
            assert two[q] and "floor" in two[q][0] and all("floor" not in d for d in two[q][1:])
            f = two[q][0]["floor"]
            assert _floor_eq(f, fused[q][0]["floor"]), q
            assert np.array_equal(f["song_hist"], res["song_hist"][q]) and np.array_equal(f["bin_hist"], res["bin_hist"][q]), q
            assert f["score"] == floor.score(int(res["aligned"][q, 0]), res["song_hist"][q])
            strip = lambda ds: [{k_: v for k_, v in d.items() if k_ != "floor"} for d in ds]   # noqa: E731
            assert strip(two[q]) == plain[q] == strip(fused[q]), q
        assert not ctx.vote_floor and ctx.floor_rows() == 0
    got, *_ = S.recognize(queries[0], db=db, topn=3, floor=True, delta_tol=2)
    assert _floor_eq(got[0]["floor"], two[0][0]["floor"]) and got[0]["song_id"] == 2


def _host_windows(ctx, chans, first, k, t1, ho, window, step):
    """tests/test_gpu_scan.py's contract, on the host: per recording and window the (key32, t1 - s) of the hashes with
    s <= t1 < s + window over all channels."""
    count = lambda frames: 0 if frames == 0 else 1 if frames <= window else -(-(frames - window) // step) + 1   # noqa: E731
    keys, qoffs, query_off = [], [], [0]
    t1 = t1.astype(np.int64)
    for r in range(len(first) - 1):
        cs = range(int(first[r]), int(first[r + 1]))
        frames = max((ctx.frames_of(len(chans[c])) for c in cs), default=0)
        for w in range(count(frames)):
            s, n = w * step, 0
            for c in cs:
                a, b = int(ho[c]), int(ho[c + 1])
                m = (t1[a:b] >= s) & (t1[a:b] < s + window)
                keys.append(k[a:b][m])
                qoffs.append((t1[a:b][m] - s).astype(np.uint32))
                n += int(m.sum())
            query_off.append(query_off[-1] + n)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint32)   # noqa: E731
    return cat(keys).astype(np.uint32), cat(qoffs).astype(np.uint32), np.asarray(query_off, np.uint64)


def test_scan_windows_floor_under_small_groups(S, ctx, music):
    from oracle import synth
    from shazam_amd import _ffi
    db, songs = music
    recs = [np.concatenate([synth.traffic_noise(5, 0, 2 * SR), songs[1][SR:5 * SR]]),
            [songs[3][0:4 * SR], songs[3][SR // 2:4 * SR + SR // 2]], synth.traffic_noise(5, 1, SR // 8)]
    chans = [recs[0], recs[1][0], recs[1][1], recs[2]]
    first = np.array([0, 1, 3, 4], np.uint32)
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    plain = S.scan_windows(recs, db, window_seconds=3, step_seconds=1)
    hk, hq, hqo = _host_windows(ctx, [S._as_pcm(c) for c in chans], first, k, t1, ho, plain["window_frames"], plain["step_frames"])
    want = db.table.match(hk, hq, hqo, 2, floor=True)
    for dbg in (0, _ffi.DEBUG_SCAN_SMALL_GROUPS, _ffi.DEBUG_SCAN_SMALL_GROUPS | _ffi.DEBUG_FLOOR_SMALL):
        ctx.set_debug(dbg)
        try:
            w = S.scan_windows(recs, db, window_seconds=3, step_seconds=1, floor=True)
        finally:
            ctx.set_debug(0)
        _same(w, plain, ("scan", dbg))
        _same(w, want, ("scan against match", dbg))
        _hist_eq(w, (want["song_hist"], want["bin_hist"]), ("scan", dbg))
        assert len(w["nres"]) == int(w["win_off"][-1]) > 3
    for kw in (dict(speeds=True), dict(tempos=[65536]), dict(pitches=[65536]), dict(warps=([65536], [65536]))):
        with pytest.raises(ValueError):
            S.scan_windows(recs, db, floor=True, **kw)
    assert not ctx.vote_floor and ctx.floor_rows() == 0


def test_scan_min_score_drops_the_foreign_stretch(S, ctx, music):
    """A recording of one catalogue song and a stretch of a song that is not in the table.  With min_aligned low enough that
    chance alone makes segments of the foreign stretch, a min_score between the two groups' scores leaves the catalogue
    song's segment only."""
    from oracle import synth
    from shazam_amd import floor
    db, songs = music
    foreign = synth.music_clip(11, N_SONGS + 7, 8 * SR)
    rec = np.concatenate([songs[1][0:6 * SR], foreign[SR:7 * SR]])
    w = S.scan_windows([rec], db, window_seconds=3, step_seconds=1, floor=True)
    n = len(w["nres"])
    split = int(6 * SR / w["hop"])                                        # the frame where the foreign stretch begins
    start = np.arange(n) * w["step_frames"]
    ours = np.flatnonzero((start + w["window_frames"] <= split) & (w["nres"] > 0) & (w["sid"][:, 0] == 2))
    theirs = np.flatnonzero((start >= split) & (w["nres"] > 0))
    sc = lambda i: floor.score(int(w["aligned"][i, 0]), w["song_hist"][i])   # noqa: E731
    s_ours = [sc(i) for i in ours]
    s_theirs = [s for s in (sc(i) for i in theirs) if s is not None]
    msg = f"catalogue windows {s_ours}, foreign windows {s_theirs}"
    assert len(ours) >= 2 and len(theirs) >= 2 and s_theirs, msg
    assert all(s is not None for s in s_ours) and min(s_ours) > max(s_theirs), msg
    min_score = (min(s_ours) + max(s_theirs)) / 2
    loose = S.scan([rec], db, window_seconds=3, step_seconds=1, min_aligned=1)
    tight = S.scan([rec], db, window_seconds=3, step_seconds=1, min_aligned=1, min_score=min_score)
    foreign_secs = split * w["hop"] / w["fs"]
    assert any(s["start_seconds"] >= foreign_secs - 1e-6 for s in loose[0]), (msg, loose)
    assert any(s["song_id"] == 2 and s["start_seconds"] < 1.5 for s in tight[0]), (msg, tight)
    assert not any(s["start_seconds"] >= foreign_secs - 1e-6 for s in tight[0]), (msg, tight)
    assert S.scan([rec], db, window_seconds=3, step_seconds=1, min_aligned=1, min_score=None) == loose
    # the same with extents=True: the timeline of that call is folded inside the library, behind a keep mask of the windows
    ext_loose = S.scan([rec], db, window_seconds=3, step_seconds=1, min_aligned=1, extents=True)
    ext_tight = S.scan([rec], db, window_seconds=3, step_seconds=1, min_aligned=1, extents=True, min_score=min_score)
    base = lambda segs: [{k: d[k] for k in loose[0][0]} for d in segs]   # noqa: E731  (the keys of the plain timeline)
    assert base(ext_loose[0]) == loose[0] and base(ext_tight[0]) == tight[0], (msg, ext_tight)
    assert not any(s["start_seconds"] >= foreign_secs - 1e-6 for s in ext_tight[0]), (msg, ext_tight)
    kept = {(d["song_id"], d["start_seconds"]): d for d in ext_loose[0]}
    for d in ext_tight[0]:                       # a segment that no cleared window touched keeps its zones
        o = kept.get((d["song_id"], d["start_seconds"]))
        if o is not None and o["end_seconds"] == d["end_seconds"]:
            assert d["pairs"] == o["pairs"] and d["play_start_seconds"] == o["play_start_seconds"], (d, o)
    assert all("pairs" in d and "play_end_seconds" in d for d in ext_tight[0]) and ext_tight[0]
    with pytest.raises(ValueError):
        S.scan([rec], db, speeds=True, min_score=1.0)


def test_listeners_and_speed_ladder_record_their_rows(S, ctx, music):
    db, songs = music
    ctx.set_vote_floor(True)
    try:
        rec = S.StreamRecognizer(db, 3, device=True, window_seconds=3, topn=2)
        rec.push([songs[0][:4 * 8192], songs[1][8192:5 * 8192], None])
        assert ctx.floor_rows() == 3
        rec.push([songs[0][4 * 8192:8 * 8192], None, None], end=True)
        assert ctx.floor_rows() == 6
        rec.close()
        ctx.take_floor()
        ladder = S.speed_ladder(0.96, 1.04, 0.04)
        assert len(ladder) == 3
        S.recognize_speeds([songs[2][SR:4 * SR], songs[3][0:3 * SR]], db, speeds=ladder)
        assert ctx.floor_rows() == 2 * len(ladder)
    finally:
        ctx.set_vote_floor(False)
    assert ctx.floor_rows() == 0
