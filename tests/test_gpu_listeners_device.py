"""GPU: StreamRecognizer(device=True) -- the listeners' sliding windows kept on the device (shz_listeners_*), one library
call per push -- returns after EVERY push exactly what the numpy recogniser (device=False) returns: the same
[(results, w0)], and the same number of hashes in every window.  Two recognisers run side by side on the same input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192
HOP = 2048


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    from oracle import synth
    ctx = S.get_context(0)
    n_songs, song_len = 50, 44100 * 20
    songs = [synth.music_clip(31, i, song_len) for i in range(n_songs)]
    db = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    for i in range(n_songs):
        sid = db.insert_song(f"song{i}", f"{i:040x}", int(len(set(zip(k[ho[i]:ho[i + 1]].tolist(), t1[ho[i]:ho[i + 1]].tolist())))))
        db.set_song_fingerprinted(sid)
    db.insert_clips(k, t1, ho, 1)
    db.finalize()
    yield S, ctx, synth, db, songs
    db.close()


def _pair(S, db, n, **kw):
    return S.StreamRecognizer(db, n, device=False, **kw), S.StreamRecognizer(db, n, device=True, **kw)


def _push_both(host, dev, chunks, end=None):
    """One push through both recognisers; everything they return and hold must agree."""
    a = host.push(chunks, end=end)
    b = dev.push(chunks, end=end)
    assert len(a) == len(b) == host.n
    for l in range(host.n):
        assert b[l][1] == a[l][1], ("w0", l)
        assert b[l][0] == a[l][0], ("results", l)
        assert type(b[l][1]) is type(a[l][1])
        assert dev.window_hashes(l) == len(host._k[l]) == host.window_hashes(l), ("window", l)
        assert dev.listeners.state(l)["w0"] == a[l][1]
        for c in range(host.channels):
            assert dev.fp.state(l * host.channels + c) == host.fp.state(l * host.channels + c)
    return a


def test_stereo_listeners_scenario(env):
    """The scenario of test_gpu_stream_recognize.py: 8 stereo listeners, 8192-sample chunks, not hop-aligned, all end on
    the last push."""
    S, ctx, synth, db, songs = env
    from shazam_amd import harness
    rng = np.random.default_rng(8)
    picks = [3, 17, 5, 9, 22, 30, 41, 48]
    starts = [int(rng.integers(1, 200)) * HOP + int(rng.integers(1, HOP)) for _ in picks]
    length = 44100 * 8
    listeners = []
    for j, (s, a) in enumerate(zip(picks, starts)):
        clean = songs[s][a:a + length]
        listeners.append((harness.mix(clean, synth.traffic_noise(70, 2 * j, length), 10),
                          harness.mix(clean, synth.traffic_noise(70, 2 * j + 1, length), 10)))
    host, dev = _pair(S, db, len(listeners), channels=2, window_seconds=5, topn=3)
    recognised = [False] * len(listeners)
    for a in range(0, length, CHUNK):
        ending = a + CHUNK >= length
        out = _push_both(host, dev, [[L[0][a:a + CHUNK], L[1][a:a + CHUNK]] for L in listeners], end=True if ending else None)
        for l, (res, w0) in enumerate(out):
            if res and res[0]["song_id"] == picks[l] + 1:
                recognised[l] = True
    assert all(recognised)
    # ended listeners keep their windows and are matched again
    out = _push_both(host, dev, [None] * len(listeners))
    assert all(res for res, _ in out)
    host.close()
    dev.close()


@pytest.mark.parametrize("window_seconds", [1, 5])
def test_mono_listeners_pauses_ends_resets_uneven_chunks(env, window_seconds):
    S, ctx, synth, db, songs = env
    from shazam_amd import harness
    n, length = 6, 44100 * 9
    rng = np.random.default_rng(21 + window_seconds)
    sig = [harness.mix(songs[7 * l + 2][5000 + 333 * l:5000 + 333 * l + length], synth.traffic_noise(71, l, length), 8)
           for l in range(n)]
    host, dev = _pair(S, db, n, channels=1, window_seconds=window_seconds, topn=2)
    pos = [0] * n
    ended = [False] * n
    sizes = [CHUNK, 0, 1, 4095, 4097, 12345, HOP, 3 * CHUNK + 17, 100, CHUNK]
    for p in range(60):
        chunks, ends = [], []
        for l in range(n):
            if ended[l] or (l == 1 and 10 <= p < 16) or (l == 4 and p % 5 == 0):
                chunks.append(None)                       # an ended listener; one that hears nothing for a while
                continue
            step = sizes[(p + 3 * l) % len(sizes)] if l != 0 else CHUNK
            c = sig[l][pos[l]:pos[l] + step]
            pos[l] += len(c)
            chunks.append(c if (l + p) % 7 else [c])      # (a bare array or a list of one channel)
            if (l == 2 and p == 20) or (pos[l] >= length):  # listener 2 ends early and is matched again afterwards
                ends.append(l)
                ended[l] = True
        out = _push_both(host, dev, chunks, end=ends or None)
        if p == 30:                                        # a subset starts afresh mid-way (one of them had ended)
            for r in (host, dev):
                r.reset([2, 3])
            for l in (2, 3):
                pos[l], ended[l] = 0, False
                assert dev.window_hashes(l) == 0 and host.window_hashes(l) == 0
        if p == 45:
            assert any(res for res, _ in out)
    for r in (host, dev):
        r.reset()
    _push_both(host, dev, [s[:CHUNK * 3] for s in sig])
    host.close()
    dev.close()


@pytest.mark.parametrize("signal", ["dc_12000_5s", "click_per_hop"])
def test_dense_listener_between_ordinary_ones(env, signal):
    """One listener hears stationary material, its neighbours music.  dc_12000_5s of oracle.synth.tie_inputs() (its tied
    cells lie below amp_min: 414 hashes in all) stays inside the object's first buffers; the click-per-hop signal, whose
    windows tie in hundreds of cells that are all peaks (about 16,000 hashes a push), does not: the streams'
    SHZ_E_CAPACITY is answered inside the call and the window grows far beyond its neighbours', which come out unchanged."""
    S, ctx, synth, db, songs = env
    if signal == "dc_12000_5s":
        dense = synth.tie_inputs()["dc_12000_5s"]
    else:
        dense = np.zeros(2048 * 60, np.int16)
        dense[1024::2048] = 20000
    n = 3
    sig = [songs[11][40000:40000 + len(dense)], dense, songs[29][70001:70001 + len(dense)]]
    host, dev = _pair(S, db, n, channels=1, window_seconds=5, topn=2)
    biggest = 0
    for a in range(0, len(dense), CHUNK):
        ending = a + CHUNK >= len(dense)
        _push_both(host, dev, [s[a:a + CHUNK] for s in sig], end=True if ending else None)
        biggest = max(biggest, dev.window_hashes(1))
    if signal == "click_per_hop":
        assert biggest > 20 * (3 * 256 + 4096), "the listener must outgrow the first buffers"
        assert biggest > 50 * max(dev.window_hashes(0), dev.window_hashes(2), 1)
    _push_both(host, dev, [None] * n)
    host.close()
    dev.close()


def test_refusals_leave_everything_as_it_was(env):
    S, ctx, synth, db, songs = env
    from shazam_amd import _ffi
    # a listener count that does not divide the streams
    fp = S.StreamFingerprinter(6, ctx=ctx)
    with pytest.raises(_ffi.ShzError) as e:
        _ffi.Listeners(fp.streams, db.table, 4, 107)
    assert e.value.code == _ffi.E_INVALID
    with pytest.raises(_ffi.ShzError) as e:
        _ffi.Listeners(fp.streams, db.table, 0, 107)
    assert e.value.code == _ffi.E_INVALID
    fp.close()
    n = 2
    sig = [songs[4][9000:9000 + 44100 * 4], songs[8][12000:12000 + 44100 * 4]]
    host, dev = _pair(S, db, n, channels=1, window_seconds=5, topn=2)
    for a in range(0, CHUNK * 12, CHUNK):
        _push_both(host, dev, [s[a:a + CHUNK] for s in sig])
    a = CHUNK * 12

    def snapshot():
        return [dev.fp.state(i) for i in range(n)], [dev.listeners.state(l) for l in range(n)]

    before = snapshot()
    pcm = np.concatenate([s[a:a + CHUNK] for s in sig])
    off = np.array([0, CHUNK, 2 * CHUNK], np.uint64)
    for topn in (0, 65):
        rc, _, _ = dev.listeners.push_raw(pcm, off, topn=topn)
        assert rc == _ffi.E_INVALID
    rc, _, _ = dev.listeners.push_raw(pcm, np.array([0, CHUNK, CHUNK - 1], np.uint64))
    assert rc == _ffi.E_INVALID                       # chunk_off decreases
    ctx.set_overlap(4096 - 1024)                       # the hop changes after creation
    try:
        rc, _, _ = dev.listeners.push_raw(pcm, off)
        assert rc == _ffi.E_STATE
        with pytest.raises(_ffi.ShzError) as e:
            dev.listeners.state(0)
        assert e.value.code == _ffi.E_STATE
    finally:
        ctx.set_overlap(4096 - HOP)
    assert snapshot() == before
    for a in range(CHUNK * 12, CHUNK * 20, CHUNK):     # and on they go, equal to the numpy recogniser
        _push_both(host, dev, [s[a:a + CHUNK] for s in sig])
    host.close()
    dev.close()
