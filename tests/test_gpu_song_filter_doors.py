"""GPU: the song filter gives one answer through every door of the library.  One small fixture -- 8 synthetic songs of 10 s in
a database -- and one check everywhere: the call with the filter on the full table equals the same call without it on the
sub-table, a second database that knows the same songs and holds only the allowed songs' rows.  Doors: recognize_batch (two
calls and fused), scan_windows and scan, the device-resident listeners, and -- inside `with ctx.songs(...)` -- recognition
over a speed ladder and the catalogue's match_songs.  Every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 44100
N_SONGS = 8
ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
ONLY = [2, 5, 3, 8]


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
    return [synth.music_clip(23, c, 10 * SR) for c in range(N_SONGS)]


@pytest.fixture(scope="module")
def env(S, ctx, songs):
    """the full database (songs 1 .. 8), and sub(ids, exclude): a database with the same song records whose table holds only
    the rows of the songs that pass"""
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    sid = np.repeat(np.arange(1, N_SONGS + 1, dtype=np.uint32), np.diff(ho).astype(np.int64))
    made = []

    def make(mask):
        d = S.get_database("hip")(ctx=ctx)
        for c in range(N_SONGS):
            assert d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c])) == c + 1
            d.set_song_fingerprinted(c + 1)
        d.table.insert(k[mask], sid[mask], t1[mask])
        d.table.finalize()
        made.append(d)
        return d

    full = make(np.ones(len(k), bool))
    yield full, lambda ids, exclude=False: make(np.isin(sid, np.asarray(ids, np.uint32)) != exclude)
    for d in made:
        d.close()


@pytest.fixture(scope="module")
def queries(songs):
    """song 1 (barred by ONLY), song 2 (allowed), a stereo query of song 5 with noise on one channel, song 7 (barred)"""
    from oracle import synth
    noisy = synth.mix_query(songs[4][3 * SR:8 * SR], synth.synth_clip(5, 9, 5 * SR, 0, 8000), 6.0)
    return [songs[0][2 * SR:7 * SR], songs[1][SR + 500:6 * SR + 500], [songs[4][3 * SR:8 * SR], noisy], songs[6][4 * SR:9 * SR]]


def _same(a, b, what, names=ARRAYS):
    for name in names:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


@pytest.mark.parametrize("fused", [False, True])
def test_recognize_batch(S, ctx, env, queries, fused):
    full, sub = env
    for kw, d in ((dict(songs=ONLY), sub(ONLY)), (dict(exclude=[1, 7]), sub([1, 7], True))):
        got, tm = S.recognize_batch(queries, full, topn=3, fused=fused, **kw)
        want, tw = S.recognize_batch(queries, d, topn=3, fused=fused)
        assert got == want, kw
        assert np.array_equal(tm["n_matches"], tw["n_matches"]) and np.array_equal(tm["n_hashes"], tw["n_hashes"])
        assert ctx.song_filter is None
    plain, _ = S.recognize_batch(queries, full, topn=3, fused=fused)
    got, _ = S.recognize_batch(queries, full, topn=3, fused=fused, songs=ONLY)
    assert plain[0][0]["song_id"] == 1 and all(r["song_id"] in ONLY for q in got for r in q)
    assert got[1][0]["song_id"] == 2 and got[2][0]["song_id"] == 5 and got[1][0] == plain[1][0]
    one, *_ = S.recognize(queries[1], db=full, topn=3, fused=fused, songs=ONLY)
    assert one == got[1]
    with pytest.raises(ValueError):
        S.recognize_batch(queries, full, songs=[1], exclude=[2])


def test_scan_windows_and_scan(S, ctx, env, songs):
    from oracle import synth
    full, sub = env
    recs = [np.concatenate([songs[0][0:6 * SR], songs[1][2 * SR:8 * SR]]),
            [songs[4][SR:7 * SR], synth.mix_query(songs[4][SR:7 * SR], synth.synth_clip(5, 3, 6 * SR, 0, 8000), 10.0)]]
    got = S.scan_windows(recs, full, window_seconds=3, step_seconds=1, topn=3, songs=ONLY)
    want = S.scan_windows(recs, sub(ONLY), window_seconds=3, step_seconds=1, topn=3)
    _same(got, want, "scan_windows")
    assert np.array_equal(got["win_off"], want["win_off"]) and len(got["nres"]) > 6
    # the song that plays first is barred: its segment leaves the timeline, the rest stays
    loose = S.scan(recs, full, window_seconds=3, step_seconds=1, min_aligned=5)
    tight = S.scan(recs, full, window_seconds=3, step_seconds=1, min_aligned=5, exclude=[1])
    assert tight == S.scan(recs, sub([1], True), window_seconds=3, step_seconds=1, min_aligned=5)
    assert any(s["song_id"] == 1 for s in loose[0]) and not any(s["song_id"] == 1 for s in tight[0])
    assert any(s["song_id"] == 2 for s in tight[0]) and any(s["song_id"] == 5 for s in tight[1])
    assert ctx.song_filter is None


@pytest.mark.parametrize("device", [True, False])
def test_stream_recognizer(S, ctx, env, songs, device):
    full, sub = env
    a = S.StreamRecognizer(full, 3, device=device, window_seconds=3, topn=2, songs=ONLY)
    b = S.StreamRecognizer(sub(ONLY), 3, device=device, window_seconds=3, topn=2)
    try:
        chunk = 3 * 8192
        for i in range(4):
            chunks = [songs[0][i * chunk:(i + 1) * chunk], songs[1][SR + i * chunk:SR + (i + 1) * chunk],
                      songs[7][i * chunk:(i + 1) * chunk] if i != 2 else None]
            got, want = a.push(chunks, end=True if i == 3 else None), b.push(chunks, end=True if i == 3 else None)
            assert got == want, (device, i)
            assert ctx.song_filter is None
        assert got[1][0] and got[1][0][0]["song_id"] == 2 and got[2][0] and got[2][0][0]["song_id"] == 8
        assert all(r["song_id"] != 1 for r in got[0][0])
    finally:
        a.close()
        b.close()
    with pytest.raises(ValueError):
        S.StreamRecognizer(full, 1, songs=[1], exclude=[2])


def test_speed_ladder_and_match_songs_inside_the_block(S, ctx, env, queries, songs):
    full, sub = env
    d = sub(ONLY)
    ladder = S.speed_ladder(0.96, 1.04, 0.04)
    qs = [queries[0], queries[1], queries[3]]
    with ctx.songs(only=ONLY):
        got, tm = S.recognize_speeds(qs, full, speeds=ladder, topn=3)
        pairs = S.match_songs(full, ONLY, topn=3)
    want, tw = S.recognize_speeds(qs, d, speeds=ladder, topn=3)
    assert got == want and np.array_equal(tm["speed_profile"], tw["speed_profile"]) and np.array_equal(tm["speed_best"], tw["speed_best"])
    assert got[1][0]["song_id"] == 2
    _same(pairs, S.match_songs(d, ONLY, topn=3), "match_songs", ARRAYS + ("rows",))
    plain = S.match_songs(full, ONLY, topn=3)
    assert np.array_equal(pairs["nhash"], plain["nhash"]) and (pairs["npairs"] <= plain["npairs"]).all()
    assert ctx.song_filter is None
