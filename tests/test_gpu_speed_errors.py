"""GPU: what shz_warp_pair_hash and shz_recognize_speeds refuse -- a factor outside [32768, 131072], a ladder of 0 or more
than 1024 factors, a clip whose warped time could reach 2^20, NULL buffers, offsets that are no CSR, a table that is not
finalized -- each with its code and message, before anything is launched: the context stays usable and the valid call that
follows gives the right answer.  A sharded database raises NotImplementedError."""
import ctypes as C

import numpy as np
import pytest

import speed_twin as T

pytestmark = pytest.mark.gpu

SR = 44100


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def song():
    from oracle import synth
    return synth.music_clip(7, 0, 8 * SR)


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


PF = np.asarray([10, 20, 30, 40], np.uint16)
PT = np.asarray([0, 0, 1, 2], np.uint32)
PO = np.asarray([0, 4], np.uint64)


def _warp_ok(ctx):
    k, t1, ho = ctx.warp_pair_hash(PF, PT, PO, [65536, 70000], None, 3)
    ek, et, eho = T.warp_pair_batch(PF, PT, PO, [0, 1], [65536, 70000], 3)
    assert np.array_equal(k, ek) and np.array_equal(t1, et) and np.array_equal(ho, eho)


def _raises(ctx, code, match, fn, *a, **kw):
    from shazam_amd import _ffi
    with pytest.raises(_ffi.ShzError, match=match) as e:
        fn(*a, **kw)
        ctx.check(0)
    assert e.value.code == code, (match, e.value)


def _warp_rc(ctx, *a, **kw):
    rc = ctx.warp_pair_hash_raw(*a, **kw)[0]
    ctx.check(rc)


def test_warp_refusals(ctx):
    from shazam_amd import _ffi
    INV = _ffi.E_INVALID
    _warp_ok(ctx)
    cases = [
        ("speed 1 is 32767", dict(speeds=[65536, 32767])),
        ("speed 0 is 131073", dict(speeds=[131073])),
        (r"n_speeds must be in \[1, 1024\], got 0", dict(speeds=[])),
        (r"n_speeds must be in \[1, 1024\], got 1025", dict(speeds=[65536] * 1025)),
        (r"fan_value must be in \[1,64\]", dict(fan_value=0)),
        (r"fan_value must be in \[1,64\]", dict(fan_value=65)),
        ("peak_off decreases at clip 1", dict(peak_off=[0, 4, 2])),
        ("query_clip0 must start at 0 and end at n_clips = 1", dict(query_clip0=[0, 2])),
        ("query_clip0 must start at 0 and end at n_clips = 1", dict(query_clip0=[1, 1])),
        ("t decreases at peak 2", dict(peak_t=[0, 3, 1, 4])),
        (r"t must be < 2\^31", dict(peak_t=[0, 0, 1, 1 << 31])),
    ]
    for match, over in cases:
        kw = dict(peak_f=PF, peak_t=PT, peak_off=PO, speeds=[65536], query_clip0=None, fan_value=3, cap=64)
        kw.update(over)
        _raises(ctx, INV, match, _warp_rc, ctx, kw.pop("peak_f"), kw.pop("peak_t"), kw.pop("peak_off"), kw.pop("speeds"), **kw)
        _warp_ok(ctx)
    _raises(ctx, INV, "query_clip0 decreases at query 1", _warp_rc, ctx, np.tile(PF, 2), np.tile(PT, 2), [0, 4, 8], [65536],
            query_clip0=[0, 2, 1, 2], cap=64)
    # NULL buffers, through the library itself
    L, sp, cnt = _ffi.lib(), np.asarray([65536], np.uint32), C.c_uint64()
    ho = np.zeros(2, np.uint64)
    k = np.zeros(64, np.uint32)
    u32p, u64p = _ffi.u32p, _ffi.u64p
    for args, match in (
            ((_ffi.ptr(PF), _ffi.ptr(PT), None, 1, None, 0, sp.ctypes.data_as(u32p), 1), "peak_off is NULL"),
            ((_ffi.ptr(PF), _ffi.ptr(PT), PO.ctypes.data_as(u64p), 1, None, 0, None, 1), "speed_q16 is NULL"),
            ((None, _ffi.ptr(PT), PO.ctypes.data_as(u64p), 1, None, 0, sp.ctypes.data_as(u32p), 1), "NULL buffer")):
        rc = L.shz_warp_pair_hash(ctx.h, *args, 3, 0, _ffi.ptr(k), _ffi.ptr(k), ho.ctypes.data_as(u64p), 64, C.byref(cnt))
        assert rc == INV and match in L.shz_last_error(ctx.h).decode()
    rc = L.shz_warp_pair_hash(ctx.h, _ffi.ptr(PF), _ffi.ptr(PT), PO.ctypes.data_as(u64p), 1, None, 0, sp.ctypes.data_as(u32p), 1, 3, 0,
                              None, None, ho.ctypes.data_as(u64p), 64, C.byref(cnt))
    assert rc == INV and "NULL buffer" in L.shz_last_error(ctx.h).decode()
    rc = L.shz_warp_pair_hash(ctx.h, _ffi.ptr(PF), _ffi.ptr(PT), PO.ctypes.data_as(u64p), 1, None, 0, sp.ctypes.data_as(u32p), 1, 3, 64,
                              _ffi.ptr(k), _ffi.ptr(k), ho.ctypes.data_as(u64p), 64, C.byref(cnt))
    assert rc == INV and "flags may hold" in L.shz_last_error(ctx.h).decode()
    _warp_ok(ctx)


def _rec_args(song, **over):
    pcm = np.ascontiguousarray(song[:5 * SR])
    a = dict(pcm=pcm, clip_off=[0, len(pcm)], query_clip0=[0, 1], speeds=[65536, 66000], topn=2, fan_value=5)
    a.update(over)
    return a


def _rec(ctx, db, a):
    return ctx.recognize_speeds(db.table, a["pcm"], a["clip_off"], a["query_clip0"], a["speeds"], topn=a["topn"],
                                fan_value=a["fan_value"])


def _rec_ok(ctx, db, song):
    res, _ = _rec(ctx, db, _rec_args(song))
    assert int(res["nres"][0]) >= 1 and int(res["sid"][0, 0]) == 1 and int(res["delta"][0, 0]) == 0 and int(res["best"][0]) == 0


def test_recognize_refusals(ctx, db, song):
    from shazam_amd import _ffi
    INV, UNS = _ffi.E_INVALID, _ffi.E_UNSUPPORTED
    _rec_ok(ctx, db, song)
    huge = (1 << 19) * 2048 + 4096      # 2^19 + 1 frames: at 2x the last frame lands on t' = 2^20.  Refused before the PCM is read
    cases = [
        (INV, "speed 1 is 131073", dict(speeds=[65536, 131073])),
        (INV, "speed 0 is 100", dict(speeds=[100])),
        (INV, r"n_speeds must be in \[1, 1024\], got 0", dict(speeds=[])),
        (INV, r"n_speeds must be in \[1, 1024\], got 1025", dict(speeds=[65536] * 1025)),
        (INV, r"fan_value must be in \[1,64\]", dict(fan_value=0)),
        (INV, r"topn must be in \[1,64\]", dict(topn=65)),
        (INV, "query_clip0 must start at 0 and end at n_clips = 1", dict(query_clip0=[0, 2])),
        (INV, "query_clip0 decreases at query 1", dict(query_clip0=[0, 1, 0, 1])),
        (INV, "clip_off decreases at clip 0", dict(clip_off=[5, 0])),
        (UNS, r"reaches t' = 1048576; query offsets must be < 2\^20", dict(clip_off=[0, huge], speeds=[65536, 131072])),
    ]
    for code, match, over in cases:
        _raises(ctx, code, match, _rec, ctx, db, _rec_args(song, **over))
        _rec_ok(ctx, db, song)
    # one frame fewer is taken as far as the check goes: t' = 2^20 - 2 (not run: the clip would be 2 GB)
    assert (((1 << 19) - 1) * 131072 + 32768) >> 16 == (1 << 20) - 2
    # 1 clip that belongs to no query
    _raises(ctx, INV, "1 clips belong to no query", _rec, ctx, db, _rec_args(song, query_clip0=[0]))
    # NULL buffers, through the library itself
    L, a = _ffi.lib(), _rec_args(song)
    co, qc = np.asarray(a["clip_off"], np.uint64), np.asarray(a["query_clip0"], np.uint32)
    sp, out = np.asarray(a["speeds"], np.uint32), np.zeros(8, np.uint32)
    u32p, u64p, o = _ffi.u32p, _ffi.u64p, _ffi.ptr(out)

    def call(pcm=_ffi.ptr(a["pcm"]), co_=co.ctypes.data_as(u64p), qc_=qc.ctypes.data_as(u32p), sp_=sp.ctypes.data_as(u32p), best=o,
             sid=o):
        return L.shz_recognize_speeds(ctx.h, db.table.h, pcm, co_, 1, qc_, 1, 44100, 10.0, 5, 2, sp_, 2, 0, best, sid, o, o, o, o, o,
                                      None, None, None, None)
    for kw, match in ((dict(pcm=None), "pcm is NULL"), (dict(co_=None), "clip_off is NULL"), (dict(qc_=None), "query_clip0 is NULL"),
                      (dict(sp_=None), "speed_q16 is NULL"), (dict(best=None), "NULL buffer"), (dict(sid=None), "NULL buffer")):
        assert call(**kw) == INV and match in L.shz_last_error(ctx.h).decode(), match
    _rec_ok(ctx, db, song)


def test_table_that_is_not_finalized(S, ctx, song):
    from shazam_amd import _ffi
    t = _ffi.Table(ctx)
    t.insert([1, 2], 1, [0, 1])
    a = _rec_args(song)
    with pytest.raises(_ffi.ShzError, match="table not finalized") as e:
        ctx.recognize_speeds(t, a["pcm"], a["clip_off"], a["query_clip0"], a["speeds"])
    assert e.value.code == _ffi.E_STATE
    t.close()


def test_sharded_database_is_not_implemented(S, ctx, song):
    d = S.get_database("hip")(ctx=ctx, shards=2)
    try:
        with pytest.raises(NotImplementedError, match=r"fused recognition takes the unsharded table \(shards=1\)"):
            S.recognize_speeds([song[:5 * SR]], d, speeds=[65536])
    finally:
        d.close()


def test_python_layer_refuses_float_speeds(S, db, song):
    with pytest.raises(TypeError, match="Q16"):
        S.recognize_speeds([song[:5 * SR]], db, speeds=[1.0, 1.02])
