"""GPU: the CONTENT of the device-resident listeners' windows (window_count_kernel / window_write_kernel in
csrc/shz_stream.hip), read back through the tests / tools entry shz_listeners_window after every push and compared element
by element and in order with the numpy recogniser's own window (StreamRecognizer(device=False)._k / ._t): key, t1, and the
query offset t1 - w0 the push handed to the match.  The match results cannot show a compaction that duplicates one entry
and drops another, or misplaces entries at a wave or round border: the match ignores order and removes duplicates.

Two recognisers run side by side on the same input, as in test_gpu_listeners_device.py.  The sizes the kernels met are
taken from the numpy recogniser alone (old_n: its window before the push; new_n: hashes its streams emitted; kept_old: old
entries with t1 >= w0) and the last test asserts that the scenarios together reached every class that matters to the
kernels: one wave / one round / two rounds / many, an old part that ends inside a wave, totals next to a multiple of the
256-entry round, and a push that kept nothing of the old entries."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192
HOP = 2048
ROUND = 256


class _Coverage:
    def __init__(self):
        self.done = {}
        self.sizes = []          # (old_n, new_n, kept_old, window after the push)

    def note(self, old_n, new_n, kept_old, win):
        self.sizes.append((old_n, new_n, kept_old, win))


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    from oracle import synth
    ctx = S.get_context(0)
    n_songs, song_len = 24, 44100 * 12
    songs = [synth.music_clip(47, i, song_len) for i in range(n_songs)]
    db = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    for i in range(n_songs):
        sid = db.insert_song(f"song{i}", f"{i:040x}", int(len(set(zip(k[ho[i]:ho[i + 1]].tolist(), t1[ho[i]:ho[i + 1]].tolist())))))
        db.set_song_fingerprinted(sid)
    db.insert_clips(k, t1, ho, 1)
    db.finalize()
    yield {"S": S, "ctx": ctx, "synth": synth, "db": db, "songs": songs, "cov": _Coverage()}
    db.close()


def _pair(S, db, n, window_frames=None, **kw):
    """the numpy recogniser and the device one; window_frames: a _ffi.Listeners created directly with that window in place
    of the one StreamRecognizer derives from window_seconds"""
    host, dev = S.StreamRecognizer(db, n, device=False, **kw), S.StreamRecognizer(db, n, device=True, **kw)
    if window_frames is not None:
        from shazam_amd import _ffi
        dev.listeners.close()
        dev.listeners = _ffi.Listeners(dev.fp.streams, db.table, n, int(window_frames))
        host.window_frames = dev.window_frames = int(window_frames)
    return host, dev


def _push_both(cov, host, dev, chunks, end=None):
    """One push through both recognisers; everything they return and hold must agree, the windows entry by entry."""
    ch = host.channels
    old_t = [host._t[l].copy() for l in range(host.n)]
    emitted = [host.fp.state(i)["emitted"] for i in range(host.n * ch)]
    a = host.push(chunks, end=end)
    b = dev.push(chunks, end=end)
    assert len(a) == len(b) == host.n
    for l in range(host.n):
        w0 = a[l][1]
        assert b[l][1] == w0, ("w0", l)
        assert dev.listeners.state(l)["w0"] == w0
        k, t, q = dev.listeners.window(l)
        assert k.dtype == t.dtype == q.dtype == np.uint32
        assert len(k) == len(host._k[l]), ("window entries", l, len(k), len(host._k[l]))
        assert np.array_equal(k, host._k[l]), ("key", l, int(np.flatnonzero(k != host._k[l])[0]))
        assert np.array_equal(t, host._t[l]), ("t1", l, int(np.flatnonzero(t != host._t[l])[0]))
        assert np.array_equal(q.astype(np.int64), t.astype(np.int64) - w0), ("q_off", l)
        assert dev.window_hashes(l) == len(k)
        assert b[l][0] == a[l][0], ("results", l)
        new_n = sum(host.fp.state(l * ch + c)["emitted"] - emitted[l * ch + c] for c in range(ch))
        kept_old = int(np.count_nonzero(old_t[l] >= w0))
        assert 0 <= new_n and kept_old <= len(host._k[l]) <= len(old_t[l]) + new_n
        cov.note(len(old_t[l]), new_n, kept_old, len(host._k[l]))
    return a


# ---- the scenarios (each runs once per module: the tests below and the coverage test share them) ------------------------

def _scenario_even(e, channels, window_seconds):
    """music listeners, 8192-sample chunks, not hop-aligned, all end on the last push and are matched once more"""
    S, db, synth, songs = e["S"], e["db"], e["synth"], e["songs"]
    from shazam_amd import harness
    rng = np.random.default_rng(80 + 10 * channels + window_seconds)
    picks = [3, 17, 5, 9][:3 if channels == 2 else 4]
    length = 44100 * 6
    listeners = []
    for j, s in enumerate(picks):
        a = int(rng.integers(1, 60)) * HOP + int(rng.integers(1, HOP))
        clean = songs[s][a:a + length]
        listeners.append([harness.mix(clean, synth.traffic_noise(70, channels * j + c, length), 10) for c in range(channels)])
    host, dev = _pair(S, db, len(listeners), channels=channels, window_seconds=window_seconds, topn=3)
    recognised = [False] * len(listeners)
    for a in range(0, length, CHUNK):
        ending = a + CHUNK >= length
        out = _push_both(e["cov"], host, dev, [[c[a:a + CHUNK] for c in L] for L in listeners], end=True if ending else None)
        for l, (res, _) in enumerate(out):
            recognised[l] |= bool(res) and res[0]["song_id"] == picks[l] + 1
    assert window_seconds < 5 or all(recognised)      # (a 1 s window need not tell the songs apart)
    _push_both(e["cov"], host, dev, [None] * len(listeners))
    host.close()
    dev.close()


def _scenario_uneven(e, window_seconds):
    """the chunk sizes, pauses, early end and mid-way reset of test_mono_listeners_pauses_ends_resets_uneven_chunks"""
    S, db, synth, songs = e["S"], e["db"], e["synth"], e["songs"]
    from shazam_amd import harness
    n, length = 5, 44100 * 7
    sig = [harness.mix(songs[4 * l + 2][5000 + 333 * l:5000 + 333 * l + length], synth.traffic_noise(71, l, length), 8)
           for l in range(n)]
    host, dev = _pair(S, db, n, channels=1, window_seconds=window_seconds, topn=2)
    pos, ended = [0] * n, [False] * n
    sizes = [CHUNK, 0, 1, 4095, 4097, 12345, HOP, 3 * CHUNK + 17, 100, CHUNK]
    for p in range(48):
        chunks, ends = [], []
        for l in range(n):
            if ended[l] or (l == 1 and 10 <= p < 16) or (l == 4 and p % 5 == 0):
                chunks.append(None)                       # an ended listener; one that hears nothing for a while
                continue
            step = sizes[(p + 3 * l) % len(sizes)] if l != 0 else CHUNK
            c = sig[l][pos[l]:pos[l] + step]
            pos[l] += len(c)
            chunks.append(c if (l + p) % 7 else [c])
            if (l == 2 and p == 20) or (pos[l] >= length):
                ends.append(l)
                ended[l] = True
        _push_both(e["cov"], host, dev, chunks, end=ends or None)
        if p == 30:                                        # a subset starts afresh mid-way (one of them had ended)
            for r in (host, dev):
                r.reset([2, 3])
            for l in (2, 3):
                pos[l], ended[l] = 0, False
                assert dev.window_hashes(l) == 0 and host.window_hashes(l) == 0
                k, t, q = dev.listeners.window(l)
                assert len(k) == len(t) == len(q) == 0
            for l in (0, 1, 4):                            # the others' windows are untouched by the reset
                k, t, _ = dev.listeners.window(l)
                assert np.array_equal(k, host._k[l]) and np.array_equal(t, host._t[l])
    for r in (host, dev):
        r.reset()
    _push_both(e["cov"], host, dev, [s[:CHUNK * 3] for s in sig])
    host.close()
    dev.close()


def _scenario_tiny(e, window_frames):
    """a window of 2 or 8 frames: a push of 8192 samples settles 4 frames, so every old entry (2) or most of them (8) expire
    and, at 2, the kept entries start in the middle of the new ones"""
    S, db, songs = e["S"], e["db"], e["songs"]
    from shazam_amd import _ffi
    n = 3
    sig = [songs[6 + l][30000 + 777 * l:30000 + 777 * l + CHUNK * 14] for l in range(n)]
    host, dev = _pair(S, db, n, window_frames=window_frames, channels=1, window_seconds=5, topn=2)
    for a in range(0, CHUNK * 14, CHUNK):
        # listener 1 gets its samples in pieces of 3 hops every third push only: bigger steps than its neighbours
        chunks = [sig[0][a:a + CHUNK], sig[1][a - 2 * CHUNK:a + CHUNK] if (a // CHUNK) % 3 == 2 else None, sig[2][a:a + CHUNK]]
        _push_both(e["cov"], host, dev, chunks)
    # the entry's own refusals: a listener out of range; less room than the window needs
    L = _ffi.lib()
    cnt = C.c_uint64(0)
    assert L.shz_listeners_window(dev.listeners.h, n, None, None, None, 0, C.byref(cnt)) == _ffi.E_INVALID
    need = max(range(n), key=dev.window_hashes)
    assert dev.window_hashes(need) > 1
    buf = [np.full(dev.window_hashes(need), 0xABCDEF01, np.uint32) for _ in range(3)]
    rc = L.shz_listeners_window(dev.listeners.h, need, _ffi.ptr(buf[0]), _ffi.ptr(buf[1]), _ffi.ptr(buf[2]), len(buf[0]) - 1, C.byref(cnt))
    assert rc == _ffi.E_CAPACITY and cnt.value == len(buf[0])
    assert all((b == 0xABCDEF01).all() for b in buf)                 # nothing was copied
    _push_both(e["cov"], host, dev, [None] * n)                     # and no state changed
    host.close()
    dev.close()


def _scenario_dense(e):
    """the click-per-hop signal (about 16,000 hashes a push) between two music listeners: many 256-entry rounds, the
    streams' SHZ_E_CAPACITY answered inside the push, and a neighbour whose entries lie behind a huge window"""
    S, db, songs = e["S"], e["db"], e["songs"]
    dense = np.zeros(2048 * 44, np.int16)
    dense[1024::2048] = 20000
    sig = [songs[11][40000:40000 + len(dense)], dense, songs[19][70001:70001 + len(dense)]]
    host, dev = _pair(S, db, 3, channels=1, window_seconds=5, topn=2)
    biggest = 0
    for a in range(0, len(dense), CHUNK):
        _push_both(e["cov"], host, dev, [s[a:a + CHUNK] for s in sig], end=True if a + CHUNK >= len(dense) else None)
        biggest = max(biggest, dev.window_hashes(1))
    assert biggest > 20 * (3 * 256 + 4096), "the listener must outgrow the first buffers"
    assert biggest > 50 * max(dev.window_hashes(0), dev.window_hashes(2), 1)
    _push_both(e["cov"], host, dev, [None] * 3)
    host.close()
    dev.close()


SCENARIOS = {("even", 1, 1): lambda e: _scenario_even(e, 1, 1), ("even", 1, 5): lambda e: _scenario_even(e, 1, 5),
             ("even", 2, 1): lambda e: _scenario_even(e, 2, 1), ("even", 2, 5): lambda e: _scenario_even(e, 2, 5),
             ("uneven", 1): lambda e: _scenario_uneven(e, 1), ("uneven", 5): lambda e: _scenario_uneven(e, 5),
             ("tiny", 2): lambda e: _scenario_tiny(e, 2), ("tiny", 8): lambda e: _scenario_tiny(e, 8),
             ("dense",): _scenario_dense}


def _ensure(e, name):
    """run a scenario once; a failure is kept and raised again for whoever asks next"""
    done = e["cov"].done
    if name not in done:
        try:
            SCENARIOS[name](e)
            done[name] = None
        except BaseException as err:
            done[name] = err
            raise
    elif done[name] is not None:
        raise done[name]


@pytest.mark.parametrize("window_seconds", [1, 5])
@pytest.mark.parametrize("channels", [1, 2])
def test_even_chunks(env, channels, window_seconds):
    _ensure(env, ("even", channels, window_seconds))


@pytest.mark.parametrize("window_seconds", [1, 5])
def test_uneven_chunks_pauses_an_early_end_and_a_reset(env, window_seconds):
    _ensure(env, ("uneven", window_seconds))


@pytest.mark.parametrize("window_frames", [2, 8])
def test_a_window_shorter_than_a_push(env, window_frames):
    _ensure(env, ("tiny", window_frames))


def test_a_dense_listener_between_two_ordinary_ones(env):
    _ensure(env, ("dense",))


def test_the_scenarios_reached_every_class_of_sizes(env):
    """from the numpy recogniser's sizes alone"""
    for name in SCENARIOS:
        _ensure(env, name)
    sizes = env["cov"].sizes
    n_in = [o + n for o, n, _, _ in sizes]
    wins = [w for _, _, _, w in sizes]
    print("pushes x listeners:", len(sizes), "| totals at a multiple of 256:", sorted(x for x in n_in if x and x % ROUND == 0),
          "| just below:", sum(1 for x in n_in if x >= ROUND and 0 < ROUND - x % ROUND <= 64 and x % ROUND),
          "| just above:", sum(1 for x in n_in if x > ROUND and 0 < x % ROUND <= 64),
          "| old ends inside a wave:", sum(1 for o, n, _, _ in sizes if o % 64 and n),
          "| nothing old kept:", sum(1 for o, n, ko, w in sizes if o > 0 and ko == 0 and n > 0 and 0 < w < n))
    for what, xs in (("entries a push walks over", n_in), ("window after a push", wins)):
        assert any(0 < x < 64 for x in xs), what
        assert any(64 < x <= 256 for x in xs), what
        assert any(256 < x <= 512 for x in xs), what
        assert any(x > 512 for x in xs), what
        assert any(x > 64 * ROUND for x in xs), what                  # (the dense listener: hundreds of rounds)
    assert any(o == 0 and n > 0 for o, n, _, _ in sizes) and any(o > 0 and n == 0 for o, n, _, _ in sizes)
    assert any(o == 0 and n == 0 for o, n, _, _ in sizes)
    # the old part ends inside a wave and new entries follow it in the same wave
    assert any(o % 64 != 0 and n > 0 for o, n, _, _ in sizes)
    # the last round of a push is nearly full / holds a few entries only (within a wave of a multiple of the round)
    assert any(x >= ROUND and 0 < ROUND - x % ROUND <= 64 and x % ROUND for x in n_in), "just below a multiple of 256"
    assert any(x > ROUND and 0 < x % ROUND <= 64 for x in n_in), "just above a multiple of 256"
    assert any(x >= ROUND and x % ROUND == 0 for x in n_in), "exactly a multiple of 256"
    # nothing of the old entries is kept, part of the new ones is; and the usual case: part of the old ones is
    assert any(o > 0 and ko == 0 and n > 0 and 0 < w < n for o, n, ko, w in sizes)
    assert any(0 < ko < o for o, _, ko, _ in sizes)
