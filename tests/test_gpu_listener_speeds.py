"""GPU: listeners at a ladder (shz_listeners_push_warps / _push_speeds) equal the CPU pipeline after every push -- the oracle's
peaks of every channel's whole signal cut to the window (tests/listen_speed_twin.py), the numpy twins of the warp per variant,
the reference's vote, the same best-variant rule: profile, best, nres, nhash and the best variant's rows are compared for
equality.  Slicing the listeners x variants into several match passes changes nothing; a ladder of [65536] is
Context.warp_pair_hash + the table's match on the window's peaks; and end to end a StreamRecognizer with a ladder names a
song played at 1.03, its speed and where the window lies in it, which the plain listeners lose."""
import numpy as np
import pytest

import listen_speed_cases as CS
import listen_speed_twin as LT
import speed_twin as T
import warp_twin as W

pytestmark = pytest.mark.gpu

N, CH = 2, 2
KEYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "best", "profile")


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    ctx = S.get_context(0)
    sg = CS.songs()
    db, table = CS.build_db(S, ctx, sg)
    sig = CS.streams(sg)
    yield {"S": S, "ctx": ctx, "db": db, "table": table, "songs": sg, "sig": sig, "peaks": [CS.oracle_peaks(x) for x in sig],
           "lad": CS.ladder()}
    db.close()


def _listeners(e, n_streams, n, table=None):
    from shazam_amd import _ffi
    st = _ffi.Streams(e["ctx"], n_streams)
    return st, _ffi.Listeners(st, (table or e["db"].table), n, CS.WINDOW_FRAMES, peaks=True)


def test_equals_the_cpu_pipeline_after_every_push(env):
    """listener 0: a song at 1.03 on both channels; listener 1: a song at 1.0, 10 dB noise on its second channel.  Chunks of
    20,000 samples (not a multiple of the hop), the streams end with the last one and are matched once more."""
    st, L = _listeners(env, N * CH, N)
    feed, lad = CS.Feed(env["sig"]), env["lad"]
    n, chunk, found = len(env["sig"][0]), 20000, [set(), set()]
    for a in list(range(0, n, chunk)) + [None]:
        chunks, ends = feed.take([chunk if a is not None else None] * 4, end=range(4) if a is not None and a + chunk >= n else ())
        res, w0s = L.push_speeds(chunks, lad, ends, CS.TOPN)
        hs = feed.horizons()
        for l in range(N):
            w0, win = LT.window(env["peaks"][l * CH:(l + 1) * CH], hs[l * CH:(l + 1) * CH], CS.WINDOW_FRAMES)
            assert int(w0s[l]) == w0
            exp = LT.expected(win, w0, env["table"], lad, None, CS.TOPN)
            LT.assert_listener(res, l, exp)
            assert L.state(l)["window_hashes"] == exp["nhash"]
            if exp["nres"]:
                found[l].add((int(res["sid"][l, 0]), int(lad[int(res["best"][l])])))
    print("top answers (sid, rung):", found)
    assert any(sid == CS.FAST_SONG + 1 and abs(rung - T.q16(CS.FAST)) <= CS.STEP for sid, rung in found[0])
    assert any(sid == CS.PLAIN_SONG + 1 and abs(rung - 65536) <= CS.STEP for sid, rung in found[1])
    L.close()
    st.close()


def test_slices_of_listeners_give_the_same(env):
    """4 listeners -- the two above, each twice -- with SHZ_DEBUG_SPEED_SMALL_SLICES (two listeners a slice) and without:
    identical arrays, and the copies agree with their originals"""
    from shazam_amd import _ffi
    ctx, lad = env["ctx"], env["lad"]
    sig = env["sig"] + env["sig"]
    a, b = _listeners(env, 8, 4), _listeners(env, 8, 4)
    fa, fb = CS.Feed(sig), CS.Feed(sig)
    n, chunk = len(sig[0]), 50000
    for p, at in enumerate(range(0, n, chunk)):
        end = range(8) if at + chunk >= n else ()
        ctx.set_debug(_ffi.DEBUG_SPEED_SMALL_SLICES)
        try:
            ch, en = fa.take([chunk] * 8, end)
            ra, wa = a[1].push_speeds(ch, lad, en, CS.TOPN)
        finally:
            ctx.set_debug(0)
        ch, en = fb.take([chunk] * 8, end)
        rb, wb = b[1].push_speeds(ch, lad, en, CS.TOPN)
        assert np.array_equal(wa, wb)
        for name in KEYS:
            assert np.array_equal(ra[name], rb[name]), (name, p)
            assert np.array_equal(ra[name][:2], ra[name][2:]), (name, p)
    assert ra["nres"].all()
    for st, L in (a, b):
        L.close()
        st.close()


def test_one_rung_is_warp_pair_hash_and_match_on_the_windows_peaks(env):
    """A ladder of [65536] alone: the peaks Listeners.peaks returns, rebased, through Context.warp_pair_hash and the table's
    match -- two public calls -- give the push's arrays"""
    ctx, db = env["ctx"], env["db"]
    st, L = _listeners(env, N * CH, N)
    feed = CS.Feed(env["sig"])
    one = np.asarray([65536], np.uint32)
    for p in range(12):
        res, w0s = L.push_speeds(feed.take([40000, 40000, 40000, 30000])[0], one, None, CS.TOPN)
        pf, pt, po = [], [], [0]
        for l in range(N):
            for c in range(CH):
                f, t = L.peaks(l, c)
                pf.append(f)
                pt.append(t - np.uint32(w0s[l]))
                po.append(po[-1] + len(f))
        k, t1, ho = ctx.warp_pair_hash(np.concatenate(pf), np.concatenate(pt), np.asarray(po, np.uint64), one,
                                       np.asarray([0, CH, 2 * CH], np.uint32), st.fan_value)
        qo = np.asarray([ho[0], ho[CH], ho[2 * CH]], np.uint64)
        want = db.match(k, t1, qo, CS.TOPN)
        assert res["best"].tolist() == [0, 0]
        for name in ("nres", "nhash"):
            assert np.array_equal(res[name], want[name]), (name, p)
        for l in range(N):
            m = int(want["nres"][l])
            for name in ("sid", "delta", "aligned", "dedup"):
                assert np.array_equal(res[name][l, :m], want[name][l, :m]), (name, l, p)
            assert int(res["profile"][l, 0]) == (int(want["aligned"][l, 0]) if m else 0)
    assert res["nres"].all()
    L.close()
    st.close()


def test_end_to_end_a_song_at_1_03_is_found_with_its_speed_and_place(env):
    """listener 0 hears songs[5] from second 3 at 1.03, listener 1 songs[2] from second 2 at 1.0; 8192-sample chunks.  From
    the first push with a full window on: the ladder names listener 0's song, its speed within one rung, its offset within 2
    frames of 3 s + w0 * 1.03 (test_listen_speed_twin_host.py: the twin alone meets this at every such push); the plain
    device listeners do not report that song; the listener at 1.0 is found by both."""
    S, db, lad = env["S"], env["db"], env["lad"]
    sig = [env["sig"][0], env["sig"][2]]
    rec = S.StreamRecognizer(db, 2, channels=1, window_seconds=5, topn=CS.TOPN, device=True, speeds=lad)
    plain = S.StreamRecognizer(db, 2, channels=1, window_seconds=5, topn=CS.TOPN, device=True)
    assert rec.window_frames == plain.window_frames == CS.WINDOW_FRAMES
    n, asserted = len(sig[0]), 0
    for a in range(0, n, CS.CHUNK):
        chunks = [s[a:a + CS.CHUNK] for s in sig]
        end = True if a + CS.CHUNK >= n else None
        got, base = rec.push(chunks, end=end), plain.push(chunks, end=end)
        assert rec.last_profile.shape == (2, len(lad)) and rec.last_best.shape == (2,)
        if LT.horizon(min(a + CS.CHUNK, n), end is True) <= CS.WINDOW_FRAMES:
            continue
        asserted += 1
        (r0, w0), (r1, w1) = got
        assert w0 == base[0][1] == LT.horizon(min(a + CS.CHUNK, n), end is True) - CS.WINDOW_FRAMES
        assert r0, a
        top = (r0[0]["song_id"], r0[0]["offset"], round(r0[0]["speed"] * 65536))
        assert CS.end_to_end_ok(top, w0, lad), (a, w0, top)
        assert all(r["speed"] == float(lad[int(rec.last_best[0])]) / 65536 for r in r0)
        assert rec.window_hashes(0) == r0[0]["input_total_hashes"]
        assert not (base[0][0] and base[0][0][0]["song_id"] == CS.FAST_SONG + 1), (a, base[0][0][:1])
        assert r1 and r1[0]["song_id"] == CS.PLAIN_SONG + 1 and abs(round(r1[0]["speed"] * 65536) - 65536) <= CS.STEP
        assert base[1][0] and base[1][0][0]["song_id"] == CS.PLAIN_SONG + 1
    assert asserted == len(CS.full_window_pushes(n)) >= 20
    # the ladder belongs to the push: narrowed to the rung found, the answer stays (both listeners have ended: matched again)
    b = int(rec.last_best[0])
    again = rec.push([None, None], speeds=lad[b:b + 1])
    assert again[0][0] and again[0][0][0]["song_id"] == CS.FAST_SONG + 1 and again[0][0][0]["speed"] == float(lad[b]) / 65536
    assert rec.last_profile.shape == (2, 1)
    rec.close()
    plain.close()


def test_python_layer_refuses_what_it_documents(env):
    S, db = env["S"], env["db"]
    with pytest.raises(ValueError, match="exclude each other"):
        S.StreamRecognizer(db, 1, device=True, speeds=[65536], warps=[(1.0, 1.0)])
    with pytest.raises(ValueError, match="device=True"):
        S.StreamRecognizer(db, 1, speeds=[65536])
    with pytest.raises(ValueError, match="device=True"):
        S.StreamRecognizer(db, 1, warps=[(1.0, 1.03)])
    plain = S.StreamRecognizer(db, 1, device=True)
    with pytest.raises(ValueError, match="created with"):
        plain.push([np.zeros(100, np.int16)], speeds=[65536])
    plain.close()
    rec = S.StreamRecognizer(db, 1, device=True, speeds=[1.0, 1.03])        # floats, as recognize_speeds takes a ladder
    assert rec.ladder[1].tolist() == [65536, T.q16(1.03)]
    with pytest.raises(ValueError, match="exclude each other"):
        rec.push([None], speeds=[65536], warps=[(1.0, 1.0)])
    rec.close()


def test_warps_a_pitch_shifted_stream_on_a_3x3_grid(env):
    """warp_twin.notes_clip songs; the stream is song 1 from its first sample at tempo 1.0 / pitch 1.03.  A 3 x 3 grid (tempo
    rungs around 1.0, pitch rungs around 1.03) through StreamRecognizer(warps=): equal to the twin after every push, and
    the result dicts carry the chosen pair."""
    from shazam_amd.speed import DEFAULT_PITCH_STEP_Q16 as PS, DEFAULT_TEMPO_STEP_Q16 as TS, warp_grid
    S, ctx = env["S"], env["ctx"]
    sg = [W.notes_clip(3, c, 12.0) for c in range(3)]
    db, table = CS.build_db(S, ctx, sg)
    x = W.notes_clip(3, 1, 9.0, tempo=1.0, pitch=1.03)
    peaks = CS.oracle_peaks(x)
    mid = 65536 + PS * int(round((T.q16(1.03) - 65536) / PS))
    t16, f16 = warp_grid(np.asarray([65536 - TS, 65536, 65536 + TS], np.uint32), np.asarray([mid - PS, mid, mid + PS], np.uint32))
    rec = S.StreamRecognizer(db, 1, channels=1, window_seconds=5, topn=CS.TOPN, device=True, warps=(t16, f16))
    feed, chunk, hits = CS.Feed([x]), 30000, 0
    try:
        for a in range(0, len(x), chunk):
            chunks, ends = feed.take([chunk], end=(0,) if a + chunk >= len(x) else ())
            (dicts, w0), = rec.push(chunks, end=ends)
            w0_t, win = LT.window([peaks], feed.horizons(), CS.WINDOW_FRAMES)
            exp = LT.expected(win, w0_t, table, t16, f16, CS.TOPN)
            assert w0 == w0_t
            assert np.array_equal(rec.last_profile[0], exp["profile"]) and int(rec.last_best[0]) == exp["best"]
            assert len(dicts) == exp["nres"]
            for n, d in enumerate(dicts):
                assert (d["song_id"], d["offset"], d["hashes_matched_in_input"], d["input_total_hashes"]) == \
                    (int(exp["sid"][n]), int(exp["delta"][n]), int(exp["dedup"][n]), exp["nhash"])
                assert (d["tempo"], d["pitch"]) == (float(t16[exp["best"]]) / 65536, float(f16[exp["best"]]) / 65536)
                assert "speed" not in d
            hits += bool(dicts) and dicts[0]["song_id"] == 2 and abs(round(dicts[0]["pitch"] * 65536) - mid) <= PS
        assert hits >= 3
    finally:
        rec.close()
        db.close()
