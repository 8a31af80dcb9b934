"""GPU: what the listeners at a ladder refuse, with the documented code, and that a refused call moves nothing: every
stream's shz_streams_state and every peak window as before, and the next good push equal to that of a second object that
never saw the bad calls.  The two kinds of listener objects do not mix; a reset empties one listener's windows and leaves
the other's alone.  No call here provokes a fault: all of them are refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import listen_speed_cases as CS

pytestmark = pytest.mark.gpu

N, CH = 2, 2
KEYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "best", "profile")


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    ctx = S.get_context(0)
    sg = CS.songs()
    db, _ = CS.build_db(S, ctx, sg)
    yield {"S": S, "ctx": ctx, "db": db, "sig": CS.streams(sg), "lad": CS.ladder()}
    db.close()


def _obj(e, peaks=True, table=None, window_frames=CS.WINDOW_FRAMES):
    from shazam_amd import _ffi
    st = _ffi.Streams(e["ctx"], N * CH)
    return st, _ffi.Listeners(st, table or e["db"].table, N, window_frames, peaks=peaks)


def _cat(chunks):
    arrs = [np.zeros(0, np.int16) if c is None else np.ascontiguousarray(c, np.int16) for c in chunks]
    off = np.zeros(len(arrs) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrs])
    return (np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)), off


def _raw(L, pcm, off, tempo, pitch, topn=2, flags=0, end=None, n_warps=None):
    """shz_listeners_push_warps through the library itself: tempo / pitch may be None"""
    from shazam_amd import _ffi
    out = [np.zeros(N * max(topn, 1) * 8 + 8192, np.uint32) for _ in range(9)]
    k = n_warps if n_warps is not None else (len(tempo) if tempo is not None else len(pitch))
    return _ffi.lib().shz_listeners_push_warps(L.h, _ffi.ptr(pcm), off.ctypes.data_as(_ffi.u64p), _ffi.ptr(end), topn, _ffi.ptr(tempo),
                                               _ffi.ptr(pitch), k, flags, *[_ffi.ptr(o) for o in out])


def _snapshot(st, L):
    return ([st.state(i) for i in range(N * CH)], [L.peaks(l, c) for l in range(N) for c in range(CH)], [L.state(l) for l in range(N)])


def _same(a, b):
    assert a[0] == b[0] and a[2] == b[2]
    for (f0, t0), (f1, t1) in zip(a[1], b[1]):
        assert np.array_equal(f0, f1) and np.array_equal(t0, t1)


def test_the_two_kinds_do_not_mix(env):
    from shazam_amd import _ffi
    lad = env["lad"]
    feed_h, feed_p = CS.Feed(env["sig"]), CS.Feed(env["sig"])
    sh, Lh = _obj(env, peaks=False)
    sp, Lp = _obj(env, peaks=True)
    for _ in range(3):
        Lh.push(feed_h.take([40000] * 4)[0])
        Lp.push_speeds(feed_p.take([40000] * 4)[0], lad)
    pcm, off = _cat(feed_h.take([40000] * 4)[0])
    before_h = ([sh.state(i) for i in range(4)], [Lh.window(l) for l in range(N)])
    before_p = _snapshot(sp, Lp)
    cnt = C.c_uint64(7)
    # the ladder's calls on a hash-window object
    assert Lh.push_warps_raw(pcm, off, lad, lad)[0] == _ffi.E_STATE
    assert Lh.push_warps_raw(pcm, off, lad)[0] == _ffi.E_STATE                   # (shz_listeners_push_speeds)
    assert _ffi.lib().shz_listeners_peaks(Lh.h, 0, 0, None, None, 0, C.byref(cnt)) == _ffi.E_STATE and cnt.value == 7
    assert _ffi.lib().shz_listeners_timing(Lh.h, 1, None) == _ffi.E_STATE
    # the hash windows' calls on a peak-window object
    assert Lp.push_raw(pcm, off)[0] == _ffi.E_STATE
    assert _ffi.lib().shz_listeners_window(Lp.h, 0, None, None, None, 0, C.byref(cnt)) == _ffi.E_STATE
    after_h = ([sh.state(i) for i in range(4)], [Lh.window(l) for l in range(N)])
    assert before_h[0] == after_h[0]
    for x, y in zip(before_h[1], after_h[1]):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    _same(before_p, _snapshot(sp, Lp))
    # state, reset and destroy work on both kinds
    assert Lp.state(0)["w0"] == Lh.state(0)["w0"]
    Lp.reset([1])
    Lh.reset([1])
    assert Lp.state(1) == Lh.state(1) == {"window_hashes": 0, "w0": 0}
    for st, L in ((sh, Lh), (sp, Lp)):
        L.close()
        st.close()


def test_refusals_move_nothing(env):
    from shazam_amd import _ffi
    INV, STATE = _ffi.E_INVALID, _ffi.E_STATE
    ctx, lad = env["ctx"], env["lad"]
    sa, A = _obj(env)
    sb, B = _obj(env)
    fa, fb = CS.Feed(env["sig"]), CS.Feed(env["sig"])
    for p in range(10):                                   # stream 3 ends on the way: a stream that must not be pushed to again
        end = (3,) if p == 5 else ()
        for L, feed in ((A, fa), (B, fb)):
            ch, en = feed.take([30000] * 4, end)
            L.push_speeds(ch, lad, en, CS.TOPN)
    assert A.state(0)["window_hashes"] > 0 and A.state(0)["w0"] > 0
    chunks = fa.take([30000, 30000, 30000, None])[0]
    fb.take([30000, 30000, 30000, None])
    pcm, off = _cat(chunks)
    good = np.ascontiguousarray(lad, np.uint32)
    before = _snapshot(sa, A)
    err = lambda: _ffi.lib().shz_last_error(ctx.h).decode()
    cases = [
        ("a ladder of 0 rungs", INV, dict(tempo=good[:0], pitch=good[:0]), "n_warps must be in"),
        ("a ladder of 1,025 rungs", INV, dict(tempo=np.full(1025, 65536, np.uint32), pitch=np.full(1025, 65536, np.uint32)), "n_warps must be in"),
        ("a tempo of 32767", INV, dict(tempo=np.asarray([65536, 32767], np.uint32), pitch=np.asarray([65536, 65536], np.uint32)), "tempo 1 is 32767"),
        ("a pitch of 32767", INV, dict(tempo=np.asarray([65536, 65536], np.uint32), pitch=np.asarray([32767, 65536], np.uint32)), "pitch 0 is 32767"),
        ("a factor of 131073", INV, dict(tempo=np.asarray([131073], np.uint32), pitch=np.asarray([65536], np.uint32)), "tempo 0 is 131073"),
        ("a NULL pitch table", INV, dict(tempo=good, pitch=None), "pitch_q16 is NULL"),
        ("a NULL tempo table", INV, dict(tempo=None, pitch=good), "tempo_q16 is NULL"),
        ("topn 0", INV, dict(tempo=good, pitch=good, topn=0), "topn must be in"),
        ("topn 65", INV, dict(tempo=good, pitch=good, topn=65), "topn must be in"),
        ("an unknown flag", INV, dict(tempo=good, pitch=good, flags=_ffi.OUT_DEVICE), "flags may hold"),
    ]
    for what, code, kw, msg in cases:
        assert _raw(A, pcm, off, **kw) == code, what
        assert msg in err(), (what, err())
        _same(before, _snapshot(sa, A))
    # the speed ladder's own entry names its arguments
    assert A.push_warps_raw(pcm, off, good[:0])[0] == INV and "n_speeds must be in" in err()
    assert A.push_warps_raw(pcm, off, np.asarray([32767], np.uint32))[0] == INV and "speed 0 is 32767" in err()
    # a stream that has ended gets samples
    bad_pcm, bad_off = _cat([chunks[0], chunks[1], chunks[2], np.zeros(100, np.int16)])
    assert _raw(A, bad_pcm, bad_off, good, good) == STATE and "has ended" in err()
    # ... or a chunk_off that decreases
    dec = off.copy()
    dec[2] = dec[1] - 1
    assert _raw(A, pcm, dec, good, good) == INV and "chunk_off decreases" in err()
    _same(before, _snapshot(sa, A))
    # a table that is not finalized: an object of its own over the same streams' ctx
    t = _ffi.Table(ctx)
    t.insert([1, 2], 1, [0, 1])
    su, U = _obj(env, table=t)
    assert _raw(U, pcm, off, good, good) == STATE and "table not finalized" in err()
    assert all(su.state(i)["samples"] == 0 for i in range(N * CH))
    U.close()
    su.close()
    t.close()
    # the next good push: the same arrays as the object that never saw a bad call
    ra, wa = A.push_speeds(chunks, lad, None, CS.TOPN)
    rb, wb = B.push_speeds(chunks, lad, None, CS.TOPN)
    assert np.array_equal(wa, wb) and ra["nres"].all()
    for name in KEYS:
        assert np.array_equal(ra[name], rb[name]), name
    _same(_snapshot(sa, A), _snapshot(sb, B))
    for st, L in ((sa, A), (sb, B)):
        L.close()
        st.close()


def test_a_warped_time_of_2_pow_20_is_unsupported(env):
    """hop 16, window_frames 2^20 - 1, tempo 2.0: 8,392,768 samples settle H = 2^19 + 1 frames in one push, w0 = 0, and
    round((H - 1) * 2) = 2^20.  Refused before anything is launched; the same samples at tempo 1.0 would pass the check (not
    run: no need to extract half a million frames)."""
    from shazam_amd import _ffi
    ctx = env["ctx"]
    ctx.set_overlap(4096 - 16)
    try:
        st = _ffi.Streams(ctx, 1)
        L = _ffi.Listeners(st, env["db"].table, 1, (1 << 20) - 1, peaks=True)
        n = ((1 << 19) + 1 + 10 - 1) * 16 + 4096                   # C = H + 10 complete frames
        assert _ffi.stream_plan(0, n, 0, 16, False)[3] == (1 << 19) + 1
        pcm, off = np.zeros(n, np.int16), np.asarray([0, n], np.uint64)
        two = np.asarray([65536, 131072], np.uint32)
        rc, _, _ = L.push_warps_raw(pcm, off, two, two)
        assert rc == _ffi.E_UNSUPPORTED and "query offsets must be < 2^20" in _ffi.lib().shz_last_error(ctx.h).decode()
        assert st.state(0) == {"samples": 0, "settled": 0, "pending": 0, "emitted": 0}
        assert len(L.peaks(0, 0)[0]) == 0 and L.state(0) == {"window_hashes": 0, "w0": 0}
        # one frame fewer: t' = 2^20 - 2 is taken as far as the check goes
        assert ((((1 << 19) - 1) * 131072 + 32768) >> 16) == (1 << 20) - 2
        L.close()
        st.close()
    finally:
        ctx.set_overlap(4096 - 2048)


def test_reset_empties_one_listener_and_leaves_the_other(env):
    lad = env["lad"]
    st, L = _obj(env)
    feed = CS.Feed(env["sig"])
    for _ in range(8):
        L.push_speeds(feed.take([30000] * 4)[0], lad)
    other = [L.peaks(1, c) for c in range(CH)]
    other_state = L.state(1)
    assert all(len(L.peaks(0, c)[0]) for c in range(CH)) and L.state(0)["window_hashes"] > 0
    L.reset([0])
    assert L.state(0) == {"window_hashes": 0, "w0": 0} and L.state(1) == other_state
    for c in range(CH):
        assert len(L.peaks(0, c)[0]) == 0
        f, t = L.peaks(1, c)
        assert np.array_equal(f, other[c][0]) and np.array_equal(t, other[c][1])
    assert all(st.state(i)["samples"] == 0 for i in (0, 1)) and all(st.state(i)["samples"] == 240000 for i in (2, 3))
    # the listener starts afresh: frame 0 again, the other goes on
    feed.reset([0, 1])
    res, w0 = L.push_speeds(feed.take([60000] * 4)[0], lad)
    assert int(w0[0]) == 0 and int(w0[1]) > 0 and len(L.peaks(0, 0)[0]) > 0 and int(L.peaks(0, 0)[1].max()) < 30
    L.close()
    st.close()
