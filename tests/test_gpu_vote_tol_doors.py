"""GPU: the vote tolerance gives one answer through every door of the library, at delta_tol 1 and 3 -- the sharded match,
the fused recognition, recognition over a speed ladder and over warp pairs (against the CPU twins with the vote replaced by
tests/vote_tol_twin.py's), the catalogue's match_songs, the windowed scan and the device-resident listeners -- and it is worth
having: a plain 10 s query cut between two frames gets 1.65 times the aligned count at a tolerance of one bin, the wrong songs
nothing.  The setting is a context's: it is restored after an exception, refused above 31, and keeps the single small query
out of the queue ahead of its vote count.  Every comparison is exact."""
import numpy as np
import pytest

import rows_warp_twin as RW
import speed_twin as T
import warp_twin as W
from test_gpu_scan import _flatten, _host_windows
from vote_tol_twin import vote_tol

pytestmark = pytest.mark.gpu

SR = 44100
ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
TOLS = (1, 3)
TOPN = 3


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def songs():
    from oracle import synth
    return [synth.music_clip(7, c, 30 * SR) for c in range(4)]


@pytest.fixture(scope="module")
def env(S, ctx, songs):
    """Songs 1..4 in a database; their rows (key32, sid, t1) as the extraction gave them; key32 -> [(sid, offset)] for the
    CPU vote."""
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    per_song = []
    for c in range(len(songs)):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        assert sid == c + 1
        d.set_song_fingerprinted(sid)
        per_song.append((k[int(ho[c]):int(ho[c + 1])], t1[int(ho[c]):int(ho[c + 1])]))
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    sid = np.repeat(np.arange(1, len(songs) + 1, dtype=np.uint32), np.diff(ho).astype(np.int64))
    yield d, (k, sid, t1), T.table_of(per_song)
    d.close()


@pytest.fixture(scope="module")
def queries(songs):
    """the plain 10 s query of DESIGN 3.7j (cut between two frames: sample 8 * 44100 is frame 172.27), a noisy one, a short one"""
    from oracle import synth
    a = songs[0][8 * SR:18 * SR]
    b = synth.mix_query(songs[2][5 * SR + 700:13 * SR + 700], synth.synth_clip(5, 9, 8 * SR, 0, 8000), 6.0)
    return [a, b, songs[3][20 * SR + 1024:23 * SR + 1024]]


@pytest.fixture(scope="module")
def query_hashes(S, ctx, queries):
    return S.fingerprint_batch(queries, ctx=ctx)


@pytest.fixture()
def tolerant_vote(monkeypatch):
    """the CPU twins' vote (oracle.cpu_ref.vote, looked up at call time by speed_twin.aligned_votes) replaced by vote_tol"""
    from oracle import cpu_ref as O

    def at(tol):
        monkeypatch.setattr(O, "vote", lambda matches, topn=2: vote_tol(matches, tol, topn))
    return at


def _same(a, b, what, names=ARRAYS):
    for name in names:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


@pytest.mark.parametrize("tol", TOLS)
def test_sharded_match_equals_table_match(S, ctx, env, query_hashes, tol):
    from shazam_amd.shard import ShardedTable
    d, (rk, rs, ro), _ = env
    k, t1, ho = query_hashes
    st = ShardedTable(ctx, nshards=3)
    st.insert(rk, rs, ro)
    st.finalize()
    want = d.table.match(k, t1, ho, TOPN, delta_tol=tol)
    _same(st.match(k, t1, ho, TOPN, delta_tol=tol), want, ("sharded", tol))
    _same(d.match(k, t1, ho, TOPN, delta_tol=tol), want, ("db", tol))
    assert int(want["aligned"][0, 0]) > int(d.table.match(k, t1, ho, TOPN)["aligned"][0, 0])   # (the tolerance is at work)
    assert ctx.vote_tolerance == 0
    st.close()


@pytest.mark.parametrize("tol", TOLS)
def test_fused_recognition_equals_fingerprint_then_match(S, ctx, env, queries, query_hashes, tol):
    d, _, _ = env
    k, t1, ho = query_hashes
    want = d.table.match(k, t1, ho, TOPN, delta_tol=tol)
    chans, pcm, off, first = _flatten(S, queries)
    with ctx.tolerance(tol):
        res, _, _ = ctx.recognize_batch(d.table, pcm, off, first, topn=TOPN)
    _same(res, want, ("fused", tol))
    fused, _ = S.recognize_batch(queries, d, topn=TOPN, fused=True, delta_tol=tol)
    plain, _ = S.recognize_batch(queries, d, topn=TOPN, delta_tol=tol)
    assert fused == plain and [r["song_id"] for r in fused[0]] == want["sid"][0, :int(want["nres"][0])].tolist()
    assert [r["offset"] for r in fused[1]] == want["delta"][1, :int(want["nres"][1])].tolist()
    assert ctx.vote_tolerance == 0


def _cpu_ladder(peaks, table, pairs, warp_pair, best_variant):
    """per query and variant: the twin's hashes and the vote (as tests/test_gpu_speed_recognize.py's expected)"""
    nq, K = len(peaks), len(pairs)
    exp = {n: np.zeros((nq, K, TOPN), np.int64) for n in ("sid", "delta", "aligned", "dedup")}
    exp["nres"], exp["nhash"] = np.zeros((nq, K), np.int64), np.zeros((nq, K), np.int64)
    for q, (f, t) in enumerate(peaks):
        for v, pair in enumerate(pairs):
            hk, ht = warp_pair(f, t, *pair)
            ranked, dedup, nhash = T.aligned_votes(hk, ht, table, TOPN)
            exp["nres"][q, v], exp["nhash"][q, v] = len(ranked), nhash
            for n, (sid, delta, aligned) in enumerate(ranked):
                exp["sid"][q, v, n], exp["delta"][q, v, n], exp["aligned"][q, v, n], exp["dedup"][q, v, n] = sid, delta, aligned, dedup[sid]
    exp["profile"] = np.where(exp["nres"] > 0, exp["aligned"][:, :, 0], 0)
    exp["best"] = np.asarray([best_variant(exp["profile"][q]) for q in range(nq)])
    return exp


def _assert_ladder(res, exp, what):
    assert np.array_equal(res["profile"], exp["profile"]), (what, res["profile"].tolist(), exp["profile"].tolist())
    assert np.array_equal(res["best"], exp["best"]), what
    for q in range(len(exp["best"])):
        b = int(exp["best"][q])
        n = int(exp["nres"][q, b])
        assert int(res["nres"][q]) == n and int(res["nhash"][q]) == int(exp["nhash"][q, b]), (what, q)
        for name in ("sid", "delta", "aligned", "dedup"):
            assert np.array_equal(res[name][q, :n], exp[name][q, b, :n]), (what, name, q)


@pytest.fixture(scope="module")
def sped(songs):
    """song 2 played at 0.97, 10 s from second 8 (DESIGN 3.7j's second table), and the plain query"""
    return [T.speed_up(songs[1][8 * SR:8 * SR + int(10 * SR * 0.97) + 2], 0.97)[:10 * SR], songs[0][8 * SR:18 * SR]]


@pytest.fixture(scope="module")
def sped_peaks(sped):
    from oracle import cpu_ref as O
    return [O.fingerprint_keys(x)[2:] for x in sped]


@pytest.mark.parametrize("tol", TOLS)
def test_speed_ladder_equals_the_twin(S, ctx, env, sped, sped_peaks, tolerant_vote, tol):
    d, _, table = env
    lad = np.asarray([T.q16(0.97), 65536, T.q16(1.03)], np.uint32)
    tolerant_vote(tol)
    exp = _cpu_ladder(sped_peaks, table, [(int(s),) for s in lad], T.warp_pair, lambda p: T.best_variant(p, lad))
    chans, pcm, off, first = _flatten(S, sped)
    with ctx.tolerance(tol):
        res, _ = ctx.recognize_speeds(d.table, pcm, off, first, lad, topn=TOPN)
    _assert_ladder(res, exp, ("speeds", tol))
    results, tm = S.recognize_speeds(sped, d, speeds=lad, topn=TOPN, delta_tol=tol)
    assert np.array_equal(tm["speed_profile"], exp["profile"]) and results[0][0]["song_id"] == 2 and results[1][0]["song_id"] == 1
    assert ctx.vote_tolerance == 0


@pytest.mark.parametrize("tol", TOLS)
def test_warp_pairs_equal_the_twin(S, ctx, env, sped, sped_peaks, tolerant_vote, tol):
    d, _, table = env
    t16 = np.asarray([T.q16(0.97), 65536, T.q16(0.97)], np.uint32)
    f16 = np.asarray([T.q16(0.97), 65536, 65536], np.uint32)
    tolerant_vote(tol)
    exp = _cpu_ladder(sped_peaks, table, list(zip(t16.tolist(), f16.tolist())), W.warp_pair_tf,
                      lambda p: W.best_variant_tf(p, t16, f16))
    chans, pcm, off, first = _flatten(S, sped)
    with ctx.tolerance(tol):
        res, _ = ctx.recognize_warps(d.table, pcm, off, first, t16, f16, topn=TOPN)
    _assert_ladder(res, exp, ("warps", tol))
    results, tm = S.recognize_warps(sped, d, warps=(t16, f16), topn=TOPN, delta_tol=tol)
    assert np.array_equal(tm["warp_profile"], exp["profile"])
    assert ctx.vote_tolerance == 0


@pytest.mark.parametrize("tol", TOLS)
def test_match_songs_equals_the_twin(S, ctx, tolerant_vote, tol):
    """a small catalogue with copies that drift: song 5 is song 1 with every second row one frame late, song 6 an excerpt of
    song 2 at +9 -- the plain and the warped call against rows_warp_twin's composition"""
    rng = np.random.default_rng(61)
    pool = np.unique(rng.integers(0, 1 << 31, 400, dtype=np.int64))
    ks, ss, os_ = [], [], []
    for sid in range(1, 5):
        cell = rng.choice(len(pool) * 300, 250, replace=False)
        ks.append(pool[cell // 300]); ss.append(np.full(250, sid, np.int64)); os_.append(cell % 300)
    ks.append(ks[0]); ss.append(np.full(250, 5, np.int64)); os_.append(os_[0] + 4 + (np.arange(250) & 1))
    ks.append(ks[1][:90]); ss.append(np.full(90, 6, np.int64)); os_.append(os_[1][:90] + 9 + (np.arange(90) % 3 == 0))
    rk, rs, ro = (np.concatenate(x) for x in (ks, ss, os_))
    t = S.Table(ctx)
    t.insert(rk.astype(np.uint32), rs.astype(np.uint32), ro.astype(np.uint32))
    t.finalize()
    table = RW.table_of_rows(rk, rs, ro)
    songs_rows = {s: (rk[rs == s], ro[rs == s]) for s in range(1, 7)}
    listed = [5, 1, 6, 2, 3]
    t16, f16 = [65536, 65536 + 300], [65536, 65536]
    tolerant_vote(tol)
    want = RW.match_songs_warps(table, songs_rows, listed, t16, f16, TOPN)
    got_w = S.match_songs(t, listed, topn=TOPN, warps=(t16, f16), delta_tol=tol)
    got_p = S.match_songs(t, listed, topn=TOPN, delta_tol=tol)
    for q in range(len(listed)):
        for v in range(2):
            ranked, nhash = want[q][v]
            n = int(got_w["nres"][q, v])
            assert [(int(got_w["sid"][q, v, i]), int(got_w["delta"][q, v, i]), int(got_w["aligned"][q, v, i])) for i in range(n)] == ranked, (tol, q, v)
            assert int(got_w["nhash"][q, v]) == nhash
        # the plain call: the song's rows as they are (the identity WARP drops rows whose random key is no pair of peaks)
        ranked = [r for r in T.aligned_votes(*songs_rows[listed[q]], table, TOPN + 1)[0] if r[0] != listed[q]][:TOPN]
        n = int(got_p["nres"][q])
        assert [(int(got_p["sid"][q, i]), int(got_p["delta"][q, i]), int(got_p["aligned"][q, i])) for i in range(n)] == ranked, (tol, q)
    assert int(got_p["aligned"][0, 0]) >= 248 and int(got_p["sid"][0, 0]) == 1     # both halves of the drifting copy ...
    assert int(S.match_songs(t, listed, topn=TOPN)["aligned"][0, 0]) <= 130          # ... one of them without the tolerance
    dup = S.find_duplicates(t, topn=TOPN, delta_tol=tol)
    assert [1, 5] in [sorted(c) for c in dup["clusters"]]
    assert ctx.vote_tolerance == 0
    t.close()


def test_scan_windows_and_listeners_equal_table_match(S, ctx, env, songs):
    from oracle import synth
    d, _, _ = env
    # the windowed scan: every window's hashes, cut on the host, through Table.match(delta_tol=1)
    rec = np.concatenate([synth.traffic_noise(5, 0, 2 * SR), songs[1][3 * SR + 500:11 * SR + 500], songs[3][SR:6 * SR]])
    w = S.scan_windows([rec], d, window_seconds=5, step_seconds=1, topn=TOPN, delta_tol=1)
    chans, pcm, off, first = _flatten(S, [rec])
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    hk, hq, hqo, hwo = _host_windows(ctx, chans, first, k, t1, ho, w["window_frames"], w["step_frames"])
    want = d.table.match(hk, hq, hqo, TOPN, delta_tol=1)
    _same(w, want, "scan_windows")
    assert np.array_equal(w["win_off"], hwo)
    assert (want["aligned"][:, 0] > d.table.match(hk, hq, hqo, TOPN)["aligned"][:, 0]).any()
    # the listeners: one push of a device-resident recogniser under ctx.tolerance(1) against its windows' hashes, kept by a
    # host recogniser beside it
    sig = [songs[0][8 * SR:14 * SR], songs[2][4 * SR + 900:10 * SR + 900]]
    host = S.StreamRecognizer(d, 2, window_seconds=5, topn=TOPN, device=False)
    dev = S.StreamRecognizer(d, 2, window_seconds=5, topn=TOPN, device=True)
    seen = {}
    inner = dev.listeners.push

    def spy(*a, **kw):
        seen["last"] = inner(*a, **kw)
        return seen["last"]
    dev.listeners.push = spy
    for a in range(0, 5 * SR, SR):
        host.push([s[a:a + SR] for s in sig])
        dev.push([s[a:a + SR] for s in sig])
    hres = host.push([s[5 * SR:] for s in sig], end=True)
    with ctx.tolerance(1):
        dres = dev.push([s[5 * SR:] for s in sig], end=True)
    res, w0 = seen["last"]
    qo = np.cumsum([0] + [len(x) for x in host._k]).astype(np.uint64)
    qk = np.concatenate(host._k)
    qt = np.concatenate([host._t[l] - np.uint32(hres[l][1]) for l in range(2)]).astype(np.uint32)
    want = d.table.match(qk, qt, qo, TOPN, delta_tol=1)
    _same(res, want, "listeners")
    assert [x[1] for x in dres] == [x[1] for x in hres] == w0.tolist()
    assert [r["song_id"] for r in dres[0][0]] == want["sid"][0, :int(want["nres"][0])].tolist()
    lifetime = S.StreamRecognizer(d, 2, window_seconds=5, topn=TOPN, device=True, delta_tol=1)
    lres = lifetime.push(sig, end=True)
    hall = S.StreamRecognizer(d, 2, window_seconds=5, topn=TOPN, device=False, delta_tol=1).push(sig, end=True)
    assert lres == hall and ctx.vote_tolerance == 0
    for r in (host, dev, lifetime):
        r.close()


def test_the_setting(S, ctx, env, query_hashes):
    from shazam_amd import _ffi
    d, _, _ = env
    k, t1, ho = query_hashes
    assert ctx.vote_tolerance == 0
    with pytest.raises(RuntimeError, match="boom"):
        with ctx.tolerance(5):
            assert ctx.vote_tolerance == 5
            with ctx.tolerance(None):
                assert ctx.vote_tolerance == 5
            raise RuntimeError("boom")
    assert ctx.vote_tolerance == 0
    ctx.set_vote_tolerance(31)
    try:
        assert _ffi.lib().shz_set_vote_tolerance(ctx.h, 32) == _ffi.E_INVALID and ctx.vote_tolerance == 31
        with pytest.raises(S.ShzError) as e:
            ctx.set_vote_tolerance(32)
        assert e.value.code == _ffi.E_INVALID and ctx.vote_tolerance == 31
        with pytest.raises(S.ShzError):
            d.table.match(k, t1, ho, TOPN, delta_tol=40)
        assert ctx.vote_tolerance == 31
    finally:
        ctx.set_vote_tolerance(0)
    # the single small host-fed query: queued ahead of its count without a tolerance, never with one
    a, b = int(ho[2]), int(ho[3])
    one = np.array([0, b - a], np.uint64)
    d.table.match(k[a:b], t1[a:b], one, 2)
    q0 = ctx.spec_stats()[0]
    d.table.match(k[a:b], t1[a:b], one, 2)
    assert ctx.spec_stats()[0] == q0 + 1
    for tol in (1, 3, 31):
        d.table.match(k[a:b], t1[a:b], one, 2, delta_tol=tol)
        with ctx.tolerance(tol):
            d.table.match_device(k[a:b], t1[a:b], one, 2, bias_bound=int(t1[a:b].max()))
    assert ctx.spec_stats()[0] == q0 + 1


def test_the_point_of_it(S, ctx, env, songs):
    """music_clip(7, 0..3), 30 s each, as songs 1..4; the query is 10 s of clip 0 from sample 8 * 44100 (frame 172.27: the
    cut falls between two frames and splits the right song's votes over the bins 172 and 173).  One bin: 821 aligned hashes;
    bins d .. d + 1: 1353, 1.65 times as many; the best wrong song: 12 either way (measured with the CPU oracle and the twin)."""
    from oracle import cpu_ref as O
    d, _, table = env
    q = songs[0][8 * SR:18 * SR]
    k, t1, _, _ = O.fingerprint_keys(q)
    pairs = sorted(set(zip(k.tolist(), t1.tolist())))
    matches = [(sid, off - qo) for kk, qo in pairs for sid, off in table.get(kk, ())]
    plain, tol1 = vote_tol(matches, 0, 2), vote_tol(matches, 1, 2)
    assert plain == [tuple(x) for x in O.vote(matches, 2)]
    print("one bin:", plain, "bins d .. d + 1:", tol1)
    assert plain[0][0] == 1 and plain[0][2] == 821 and tol1[0][0] == 1 and tol1[0][2] == 1353
    assert plain[1][2] == 12 and tol1[1][2] == 12
    res, _, _, _ = S.recognize(q, db=d, topn=2, delta_tol=1)
    raw = d.table.match(k, t1, np.array([0, len(k)], np.uint64), 2, delta_tol=1)
    assert [r["song_id"] for r in res] == [tol1[0][0], tol1[1][0]] == raw["sid"][0].tolist()
    assert [r["offset"] for r in res] == [tol1[0][1], tol1[1][1]] == raw["delta"][0].tolist()
    assert int(raw["aligned"][0, 0]) == tol1[0][2] and int(raw["aligned"][0, 1]) == tol1[1][2]
    assert int(raw["aligned"][0, 0]) >= 1.5 * plain[0][2]
    res0, _, _, _ = S.recognize(q, db=d, topn=2)
    raw0 = d.table.match(k, t1, np.array([0, len(k)], np.uint64), 2)
    assert res0[0]["song_id"] == 1 and int(raw0["aligned"][0, 0]) == 821 and raw0["delta"][0, 0] == plain[0][1]
