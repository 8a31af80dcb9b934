"""GPU: what shz_warp_pair_hash_tf, shz_recognize_warps and recognize_warps refuse -- 0 or more than 1,024 warps, a factor
outside [32768, 131072] in either table, one table NULL, a clip whose warped time at the largest tempo reaches 2^20, a
sharded database, a pair list together with a ladder -- each with its code and a message that names the argument, before
anything is launched: the context stays usable and the valid call that follows gives the right answer."""
import ctypes as C

import numpy as np
import pytest

import warp_twin as W

pytestmark = pytest.mark.gpu

SR = 44100
PF = np.asarray([10, 20, 30, 40], np.uint16)
PT = np.asarray([0, 0, 1, 2], np.uint32)
PO = np.asarray([0, 4], np.uint64)


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def song():
    return W.notes_clip(7, 0, 8)


@pytest.fixture(scope="module")
def db(S, ctx, song):
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch([song], ctx=ctx)
    d.insert_song("song0", "AB" * 20, int(ho[1]))
    d.set_song_fingerprinted(1)
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    yield d
    d.close()


def _warp_ok(ctx):
    got = ctx.warp_pair_hash_tf(PF, PT, PO, [65536, 60000], [70000, 65536], None, 3)
    want = W.warp_pair_batch_tf(PF, PT, PO, [0, 1], [65536, 60000], [70000, 65536], 3)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got[0]) > 0


def _raises(ctx, code, match, fn, *a, **kw):
    from shazam_amd import _ffi
    with pytest.raises(_ffi.ShzError, match=match) as e:
        fn(*a, **kw)
    assert e.value.code == code, (match, e.value)


def _warp_rc(ctx, tempos, pitches):
    ctx.check(ctx.warp_pair_hash_tf_raw(PF, PT, PO, tempos, pitches, None, 3, cap=64)[0])


def test_warp_hash_refusals(ctx):
    from shazam_amd import _ffi
    INV = _ffi.E_INVALID
    _warp_ok(ctx)
    one = [65536]
    for match, tempos, pitches in (
            (r"shz_warp_pair_hash_tf: n_warps must be in \[1, 1024\], got 0", [], []),
            (r"shz_warp_pair_hash_tf: n_warps must be in \[1, 1024\], got 1025", one * 1025, one * 1025),
            ("tempo 1 is 32767", [65536, 32767], [65536, 65536]),
            ("tempo 0 is 131073", [131073], one),
            ("pitch 1 is 32767", [65536, 65536], [65536, 32767]),
            ("pitch 0 is 131073", one, [131073]),
            ("pitch 2 is 0", one * 3, [32768, 131072, 0])):
        _raises(ctx, INV, match, _warp_rc, ctx, tempos, pitches)
        _warp_ok(ctx)
    # one table NULL, through the library itself
    L, sp, cnt = _ffi.lib(), np.asarray([65536], np.uint32), C.c_uint64()
    ho, k = np.zeros(2, np.uint64), np.zeros(64, np.uint32)
    u32p, u64p = _ffi.u32p, _ffi.u64p
    for tq, fq, match in ((None, sp.ctypes.data_as(u32p), "tempo_q16 is NULL"), (sp.ctypes.data_as(u32p), None, "pitch_q16 is NULL")):
        rc = L.shz_warp_pair_hash_tf(ctx.h, _ffi.ptr(PF), _ffi.ptr(PT), PO.ctypes.data_as(u64p), 1, None, 0, tq, fq, 1, 3, 0,
                                     _ffi.ptr(k), _ffi.ptr(k), ho.ctypes.data_as(u64p), 64, C.byref(cnt))
        assert rc == INV and match in L.shz_last_error(ctx.h).decode()
    _warp_ok(ctx)
    with pytest.raises(ValueError, match="two lists of one length"):
        ctx.warp_pair_hash_tf(PF, PT, PO, [65536, 65536], [65536], None, 3)


def _rec(ctx, db, song, tempos=(65536, 66000), pitches=(65536, 65536), clip_off=None):
    pcm = np.ascontiguousarray(song[:5 * SR])
    return ctx.recognize_warps(db.table, pcm, [0, len(pcm)] if clip_off is None else clip_off, [0, 1], list(tempos), list(pitches))


def _rec_ok(ctx, db, song):
    res, _ = _rec(ctx, db, song)
    assert int(res["nres"][0]) >= 1 and int(res["sid"][0, 0]) == 1 and int(res["delta"][0, 0]) == 0 and int(res["best"][0]) == 0


def test_recognize_refusals(ctx, db, song):
    from shazam_amd import _ffi
    INV, UNS = _ffi.E_INVALID, _ffi.E_UNSUPPORTED
    _rec_ok(ctx, db, song)
    one = [65536]
    huge = (1 << 19) * 2048 + 4096      # 2^19 + 1 frames: at tempo 2x the last frame lands on t' = 2^20.  Refused before the PCM is read
    for code, match, kw in (
            (INV, r"shz_recognize_warps: n_warps must be in \[1, 1024\], got 0", dict(tempos=[], pitches=[])),
            (INV, r"shz_recognize_warps: n_warps must be in \[1, 1024\], got 1025", dict(tempos=one * 1025, pitches=one * 1025)),
            (INV, "tempo 1 is 32767", dict(tempos=[65536, 32767], pitches=one * 2)),
            (INV, "tempo 0 is 131073", dict(tempos=[131073], pitches=one)),
            (INV, "pitch 1 is 32767", dict(tempos=one * 2, pitches=[65536, 32767])),
            (INV, "pitch 0 is 131073", dict(tempos=one, pitches=[131073])),
            (UNS, r"reaches t' = 1048576; query offsets must be < 2\^20", dict(tempos=[65536, 131072], pitches=one * 2, clip_off=[0, huge]))):
        _raises(ctx, code, match, _rec, ctx, db, song, **kw)
        _rec_ok(ctx, db, song)
    # the pitch table does not enter the time bound: the same clip at pitch 2x and tempo 1 passes the check (it is refused
    # later only if it were run; not run: the clip would be 2 GB) -- one frame fewer at tempo 2x stays below 2^20
    assert (((1 << 19) - 1) * 131072 + 32768) >> 16 == (1 << 20) - 2
    # one table NULL, through the library itself
    L, a = _ffi.lib(), np.ascontiguousarray(song[:5 * SR])
    co, qc = np.asarray([0, len(a)], np.uint64), np.asarray([0, 1], np.uint32)
    sp, out = np.asarray([65536, 66000], np.uint32), np.zeros(8, np.uint32)
    u32p, u64p, o = _ffi.u32p, _ffi.u64p, _ffi.ptr(out)
    for tq, fq, match in ((None, sp.ctypes.data_as(u32p), "tempo_q16 is NULL"), (sp.ctypes.data_as(u32p), None, "pitch_q16 is NULL")):
        rc = L.shz_recognize_warps(ctx.h, db.table.h, _ffi.ptr(a), co.ctypes.data_as(u64p), 1, qc.ctypes.data_as(u32p), 1, 44100, 10.0,
                                   5, 2, tq, fq, 2, 0, o, o, o, o, o, o, o, None, None, None, None)
        assert rc == INV and match in L.shz_last_error(ctx.h).decode(), match
    _rec_ok(ctx, db, song)


def test_python_layer_refusals(S, ctx, db, song):
    q = [song[:5 * SR]]
    d = S.get_database("hip")(ctx=ctx, shards=2)
    try:
        with pytest.raises(NotImplementedError, match=r"fused recognition takes the unsharded table \(shards=1\)"):
            S.recognize_warps(q, d, tempos=[65536])
    finally:
        d.close()
    with pytest.raises(TypeError, match="warps= is an explicit pair list: it excludes tempos= and pitches="):
        S.recognize_warps(q, db, tempos=[65536], warps=([65536], [65536]))
    with pytest.raises(TypeError, match="warps= is an explicit pair list"):
        S.recognize_warps(q, db, pitches=[65536], warps=([65536], [65536]))
    with pytest.raises(TypeError, match="separable"):
        S.recognize_warps(q, db, warps=([65536], [65536]), search="separable")
    with pytest.raises(ValueError, match="two lists of one length"):
        S.recognize_warps(q, db, warps=([65536, 65536], [65536]))
    with pytest.raises(TypeError, match="Q16"):
        S.recognize_warps(q, db, tempos=[1.0, 1.02])
    with pytest.raises(ValueError, match="search"):
        S.recognize_warps(q, db, tempos=[65536], search="coarse")
    # and the valid calls that follow: no ladders at all is the pair (65536, 65536)
    res, tm = S.recognize_warps(q, db)
    assert res[0][0]["song_id"] == 1 and res[0][0]["offset"] == 0 and (res[0][0]["tempo"], res[0][0]["pitch"]) == (1.0, 1.0)
    assert tm["warps"][0].tolist() == [65536] and tm["warps"][1].tolist() == [65536]
    res, _ = S.recognize_warps(q, db, warps=([66000, 65536], [65536, 65536]))
    assert res[0][0]["song_id"] == 1 and res[0][0]["tempo"] == 1.0
