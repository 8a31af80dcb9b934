"""GPU: shz_scan_extents -- the scan, its timeline and the extent pass on three zones (whole, head, tail) of every segment in one
call, the recordings' hashes staying on the device.  Windows and segments are shz_scan_batch's and shz_scan_timeline's; the zone
results are, bit for bit, Table.match_extents on zone queries built on the host AND the plain-Python definition
(tests/scan_extent_twin.py) over the exported table rows; the two identities of the definition; batch shapes that can go
wrong; the planted boundaries; capacity and refusals; scan(extents=True)."""
import numpy as np
import pytest

from scan_extent_twin import zone_results, zones

pytestmark = pytest.mark.gpu

ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
SEG = ("rec", "sid", "shift", "first", "last", "hits", "best")
WINDOW, STEP = 108, 22            # round(5 s * 44100 / 2048), round(1 s * 44100 / 2048)
SR, HOP = 44100, 2048
FILL = 77


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
    return [synth.music_clip(11, c, 8 * SR) for c in range(4)]


@pytest.fixture(scope="module")
def recording(songs):
    """343 frames: 3 s of noise | song 2 from 1 s to 7 s | the first 5 s of song 4 | 2 s of noise"""
    from oracle import synth
    return np.concatenate([synth.traffic_noise(5, 0, 3 * SR), songs[1][SR:7 * SR], songs[3][0:5 * SR],
                           synth.traffic_noise(5, 1, 2 * SR)])


@pytest.fixture(scope="module")
def interrupted(songs):
    """214 frames: 1 s of noise | song 3 with its seconds 2 .. 6 replaced by noise | 1 s of noise"""
    from oracle import synth
    x = songs[2].copy()
    x[2 * SR:6 * SR] = synth.traffic_noise(7, 0, 4 * SR)
    return np.concatenate([synth.traffic_noise(7, 1, SR), x, synth.traffic_noise(7, 2, SR)])


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    for c in range(4):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        assert sid == c + 1
        d.set_song_fingerprinted(sid)
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    yield d
    d.close()


@pytest.fixture(scope="module")
def rows(db):
    """The table as the twin reads it, exported once."""
    k, s, o = db.table.export()
    return list(zip(k.tolist(), s.tolist(), o.tolist()))


def _flatten(S, recordings):
    chans, first = [], [0]
    for r in recordings:
        cs = [r] if (isinstance(r, np.ndarray) and r.ndim == 1) else list(r)
        chans.extend(S._as_pcm(c) for c in cs)
        first.append(len(chans))
    off = np.zeros(len(chans) + 1, np.uint64)
    if chans:
        off[1:] = np.cumsum([len(c) for c in chans])
    pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
    return chans, pcm, off, np.asarray(first, np.uint32)


def _segs(seg):
    return [tuple(int(seg[k][i]) for k in SEG[:5]) for i in range(len(seg["rec"]))]


def _check(S, db, rows, recordings, window, step, min_aligned, max_gap, margin, tol, topns=(2,), flags=None, what=""):
    """One shz_scan_extents against (1) scan_batch + scan_timeline, (2) scan_zones and the twin's zones, (3) Table.match_extents
    on host-built zone queries, (4) the twin over the exported rows -- with and without the debug switches that force the
    extent pass's sub-batches of 3 queries and the scan's groups of 3 windows.  Returns the last (res, seg, zone, frames)."""
    from shazam_amd import _ffi
    ctx = db.ctx
    chans, pcm, off, first = _flatten(S, recordings)
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    frames = [max((ctx.frames_of(len(chans[c])) for c in range(int(first[r]), int(first[r + 1]))), default=0)
              for r in range(len(first) - 1)]
    chan_hashes = [(k[int(ho[c]):int(ho[c + 1])], t1[int(ho[c]):int(ho[c + 1])]) for c in range(len(chans))]
    out = None
    for topn in topns:
        want, want_wo, _ = ctx.scan_batch(db.table, pcm, off, first, window, step, topn=topn)
        want_seg = _ffi.scan_timeline(want_wo, want["sid"], want["delta"], want["aligned"], want["nres"], step, min_aligned, max_gap)
        segs = _segs(want_seg)
        want_zones = zones(segs, frames, window, step, margin)
        twin = zone_results(rows, chan_hashes, first, segs, frames, window, step, margin, tol)
        for flag in ((0, _ffi.DEBUG_EXTENT_SMALL_TILES | _ffi.DEBUG_SCAN_SMALL_GROUPS) if flags is None else flags):
            ctx.set_debug(flag)
            try:
                res, wo, seg, zone, ms = ctx.scan_extents(db.table, pcm, off, first, window, step, min_aligned, max_gap, margin, tol,
                                                          topn=topn)
                bare = ctx.scan_extents(db.table, pcm, off, first, window, step, min_aligned, max_gap, margin, tol, topn=topn,
                                        hist=False)[3]
                ref = _host_zone_extents(db, first, chan_hashes, segs, want_zones, tol)
            finally:
                ctx.set_debug(0)
            w = (what, topn, flag)
            # (1) windows and segments
            assert np.array_equal(wo, want_wo), w
            for name in ARRAYS:
                assert res[name].dtype == want[name].dtype and np.array_equal(res[name], want[name]), (w, name)
            for name in SEG:
                assert seg[name].dtype == want_seg[name].dtype and np.array_equal(seg[name], want_seg[name]), (w, name)
            assert all(m >= 0.0 for m in ms) and len(ms) == 4
            # (2) the zones
            lo, hi = _ffi.scan_zones(seg, frames, window, step, margin)
            assert np.array_equal(zone["lo"], lo) and np.array_equal(zone["hi"], hi), w
            assert list(zip(lo.reshape(-1).tolist(), hi.reshape(-1).tolist())) == want_zones, w
            # (3) Table.match_extents on the host-built queries, (4) the twin
            flat = {f: zone[f].reshape(-1) for f in _ffi.ZONE_FIELDS}
            for z, tw in enumerate(twin):
                got = {f: int(flat[f][z]) for f in _ffi.ZONE_FIELDS}
                assert got == {f: tw[f] for f in _ffi.ZONE_FIELDS}, (w, "twin", z, got, tw)
                assert zone["hist"].reshape(-1, 64)[z].tolist() == tw["hist"], (w, "twin hist", z)
                add = got["lo"] if got["count"] else 0
                assert got["count"] == int(ref["count"][z, 0]) and got["shift"] == int(ref["shift"][z]), (w, "match_extents", z)
                assert (got["q_first"], got["q_last"]) == (int(ref["q_first"][z, 0]) + add, int(ref["q_last"][z, 0]) + add), (w, z)
                assert (got["t_first"], got["t_last"]) == (int(ref["t_first"][z, 0]), int(ref["t_last"][z, 0])), (w, z)
                assert np.array_equal(zone["hist"].reshape(-1, 64)[z], ref["hist"][z, 0]), (w, "match_extents hist", z)
            assert np.array_equal(zone["hist"].sum(axis=2), zone["count"]), w
            assert bare["hist"] is None
            for f in _ffi.ZONE_FIELDS:
                assert np.array_equal(bare[f], zone[f]), (w, "without hist", f)
            out = (res, seg, zone, frames)
    return out


def _host_zone_extents(db, first, chan_hashes, segs, zone_list, tol):
    """Table.match_extents on the zones' queries built on the host from fingerprint_batch's output."""
    keys, qoffs, qoff, cs, dlo, dhi = [], [], [0], [], [], []
    for z, (lo, hi) in enumerate(zone_list):
        r, sid, h, _, _ = segs[z // 3]
        n = 0
        for c in range(int(first[r]), int(first[r + 1])):
            k, t1 = chan_hashes[c]
            m = (t1.astype(np.int64) >= lo) & (t1.astype(np.int64) < hi)
            keys.append(k[m])
            qoffs.append((t1[m].astype(np.int64) - lo).astype(np.uint32))
            n += int(m.sum())
        qoff.append(qoff[-1] + n)
        cs.append([sid])
        dlo.append([h + lo - tol])
        dhi.append([h + lo + tol])
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)   # noqa: E731
    return db.table.match_extents(cat(keys), cat(qoffs), np.asarray(qoff, np.uint64), np.asarray(cs, np.uint32).reshape(-1, 1),
                                  np.asarray(dlo, np.int32).reshape(-1, 1), np.asarray(dhi, np.int32).reshape(-1, 1))


# ---- windows, segments and zone results on the planted recording ---------------------------------------------------------
def test_recipe_windows_segments_and_zones(S, ctx, db, rows, recording):
    assert ctx.frames_of(len(recording)) == 343
    res, seg, zone, _ = _check(S, db, rows, [recording], WINDOW, STEP, 50, 1, WINDOW, 0, topns=(1, 2), what="recipe")
    assert _segs(seg) == [(0, 2, -43, 0, 7), (0, 4, -194, 8, 11)]
    assert zone["lo"].tolist() == [[0, 0, 154], [68, 68, 242]] and zone["hi"].tolist() == [[343, 108, 343], [343, 284, 343]]
    # any segment, tolerance 0: every window's hash set is a subset of zone 0's
    assert (zone["count"][:, 0] >= seg["best"]).all()


def test_one_window_segment_counts_the_windows_aligned(S, ctx, db, rows, recording):
    # the rank-0 counts of the 12 windows peak at window 3 (song 2) and window 9 (song 4); thresholds between the peaks and their
    # neighbours, max_gap 0 and margin 0 leave one-window segments
    want, _, _ = ctx.scan_batch(db.table, *_flatten(S, [recording])[1:], WINDOW, STEP, topn=2)
    al = want["aligned"][:, 0].astype(np.int64)
    assert int(np.argmax(al[:8])) == 3 and int(np.argmax(al[8:])) == 1
    for min_aligned in (int(al[3]), int(al[9])):
        res, seg, zone, _ = _check(S, db, rows, [recording], WINDOW, STEP, min_aligned, 0, 0, 0, what=("one window", min_aligned))
        one = np.flatnonzero(seg["first"] == seg["last"])
        assert len(one) >= 1
        for i in one.tolist():
            w = int(seg["first"][i])
            assert (int(zone["lo"][i, 0]), int(zone["hi"][i, 0])) == (w * STEP, min(w * STEP + WINDOW, 343))
            assert int(zone["count"][i, 0]) == int(res["aligned"][w, 0]) == int(seg["best"][i])
        assert (zone["count"][:, 0] >= seg["best"]).all()


# ---- shapes that can go wrong ---------------------------------------------------------------------------------------------
def test_stereo_unequal_and_duplicated_channels(S, ctx, db, rows, recording):
    part = recording[2 * SR:9 * SR]
    res, seg, zone, frames = _check(S, db, rows, [[part, part[:3 * SR + 777]], [part, part], part], 40, 15, 30, 1, 40, 0, what="stereo")
    assert len(seg["rec"]) >= 3 and set(seg["rec"].tolist()) == {0, 1, 2}
    # a duplicated channel changes nothing (the set semantics): recording 1's segments and zones are the mono recording's
    a, b = np.flatnonzero(seg["rec"] == 1), np.flatnonzero(seg["rec"] == 2)
    assert len(a) == len(b) > 0
    for f in ("lo", "hi", "count", "q_first", "q_last", "t_first", "t_last", "shift", "hist"):
        assert np.array_equal(zone[f][a], zone[f][b]), f


def test_batch_with_noise_and_an_empty_recording(S, ctx, db, rows, recording):
    from oracle import synth
    batch = [recording, synth.traffic_noise(9, 0, 4 * SR), np.zeros(0, np.int16), recording]
    res, seg, zone, frames = _check(S, db, rows, batch, WINDOW, STEP, 50, 1, WINDOW, 0, what="batch")
    assert frames == [343, 85, 1, 343]        # (a clip without samples is one zero-padded frame, as everywhere: one empty window)
    assert _segs(seg) == [(0, 2, -43, 0, 7), (0, 4, -194, 8, 11), (3, 2, -43, 0, 7), (3, 4, -194, 8, 11)]
    for f in ("lo", "hi", "count", "q_first", "q_last", "t_first", "t_last", "shift", "hist"):
        assert np.array_equal(zone[f][:2], zone[f][2:]), f


def test_same_song_twice_at_different_shifts(S, ctx, db, rows, songs):
    from oracle import synth
    rec = np.concatenate([synth.traffic_noise(8, 0, SR), songs[0][SR:4 * SR], synth.traffic_noise(8, 1, SR), songs[0][SR:4 * SR],
                          synth.traffic_noise(8, 2, SR)])
    res, seg, zone, _ = _check(S, db, rows, [rec], 43, 11, 20, 0, 43, 0, what="twice")
    mine = [s for s in _segs(seg) if s[1] == 1]
    assert len(mine) == 2 and mine[0][2] != mine[1][2], "one song, two shifts: two identities, no clamp between them"
    assert mine[0][2] - mine[1][2] == round(4 * SR / HOP), "the second play lies 4 s behind the first"


def test_interrupted_song_keeps_both_sides_apart(S, ctx, db, rows, interrupted):
    window, step, margin = 43, 11, 43
    assert ctx.frames_of(len(interrupted)) == 214
    res, seg, zone, _ = _check(S, db, rows, [interrupted], window, step, 20, 0, margin, 0, what="interrupted")
    # the precondition: two segments of one (song, shift), with a gap below the margin between them, so that both clamps act
    # (the CPU oracle's windows give the same two segments)
    assert _segs(seg) == [(0, 3, -21, 0, 5), (0, 3, -21, 12, 16)]
    assert 12 * step - (5 * step + window) < margin
    assert zone["hi"][0].tolist() == [132, 43, 132] and zone["lo"][1].tolist() == [98, 98, 176]
    out = S.scan([interrupted], db, window_seconds=window * HOP / SR, step_seconds=step * HOP / SR, min_aligned=20, max_gap=0,
                 extents=True)
    a, b = out[0]
    assert (a["shift"], b["shift"]) == (-21, -21) and a["song_id"] == b["song_id"] == 3
    # the noise lies from 3 s to 7 s of the recording.  A frame is 4096 samples wide, so a frame whose start lies up to one
    # frame width in front of a cut still holds audio of the other side: each end is held to its own side within that width
    width = 4096 / SR
    assert a["play_end_seconds"] <= 3.0 + width and b["play_start_seconds"] >= 7.0 - width
    assert a["play_end_seconds"] < 5.0 < b["play_start_seconds"]
    assert a["play_start_seconds"] < a["play_end_seconds"] and b["play_start_seconds"] < b["play_end_seconds"]


def test_margins_and_tolerances(S, ctx, db, rows, recording):
    for margin in (0, 1000):
        _check(S, db, rows, [recording], WINDOW, STEP, 50, 1, margin, 0, what=("margin", margin))
    with ctx.tolerance(2):
        for tol in (0, 2):
            res, seg, zone, _ = _check(S, db, rows, [recording], WINDOW, STEP, 50, 1, WINDOW, tol, what=("tolerance 2, d_tol", tol))
            assert len(seg["rec"]) == 2
    assert ctx.vote_tolerance == 0


# ---- ground truth -----------------------------------------------------------------------------------------------------------
def test_planted_boundaries(S, db, recording):
    """Song 2 plays from 3 s to 9 s of the recording, song 4 from 9 s to 14 s.
    The bound: the definition (tests/scan_extent_twin.py) on the CPU oracle's hashes of this fixture -- which equal the GPU's,
    tests/test_gpu_scan.py -- with dense_span puts the four ends at frames 64, 190, 192 and 298: 0.6, 3.8, 1.8 and 3.5 frames
    (0.028, 0.176, 0.084, 0.161 s) in front of the planted cuts.  An anchor's frame is its pair's EARLIER peak, so the last
    anchors lie a few frames in front of a play's end.  The head / tail zones are 108 + 108 frames or less: buckets of 2 or 4
    frames.  The largest error, 3.8 frames, rounded up to the widest bucket is 4 frames; plus one bucket: 8 frames = 0.372 s."""
    bound = 8 * HOP / SR
    coarse = S.scan([recording], db, min_aligned=50)[0]
    fine = S.scan([recording], db, min_aligned=50, extents=True)[0]
    assert len(coarse) == len(fine) == 2
    planted = [(3.0, 9.0), (9.0, 14.0)]
    closer = 0
    for c, f, (t0, t1) in zip(coarse, fine, planted):
        for key_c, key_f, t in (("start_seconds", "play_start_seconds", t0), ("end_seconds", "play_end_seconds", t1)):
            err_c, err_f = abs(c[key_c] - t), abs(f[key_f] - t)
            print(f"song {f['song_id']} {key_f}: {f[key_f]} (planted {t}, error {err_f:.3f} s; {key_c} {c[key_c]}, error {err_c:.3f} s)")
            assert err_f <= err_c and err_f <= bound, (key_f, f[key_f], t, bound)
            closer += err_f < err_c
    assert closer >= 3


# ---- capacity and refusals --------------------------------------------------------------------------------------------------
def _untouched(zone):
    return all((v == FILL).all() for v in zone.values())


def test_capacity_and_zero_segments(S, ctx, db, recording):
    from shazam_amd import _ffi
    _, pcm, off, first = _flatten(S, [recording])
    want, want_wo, _ = ctx.scan_batch(db.table, pcm, off, first, WINDOW, STEP, topn=2)
    args = (db.table, pcm, off, first, WINDOW, STEP)
    # room for one of the two segments
    rc, res, seg, zone, wo, n_wins, n_segs, _ = ctx.scan_extents_raw(*args, 50, 1, WINDOW, 0, cap_windows=12, cap_segs=1, fill=FILL)
    assert rc == _ffi.E_CAPACITY and (n_wins, n_segs) == (12, 2)
    assert np.array_equal(wo, want_wo) and all(np.array_equal(res[k], want[k]) for k in ARRAYS)
    assert tuple(int(seg[k][0]) for k in SEG[:5]) == (0, 2, -43, 0, 7)
    assert _untouched(zone), "zone outputs only ever come from a call that returns SHZ_OK"
    # room for no window: nothing is launched, the total is named
    rc, _, _, zone, wo, n_wins, n_segs, _ = ctx.scan_extents_raw(*args, 50, 1, WINDOW, 0, cap_windows=3, cap_segs=4, fill=FILL)
    assert rc == _ffi.E_CAPACITY and (n_wins, n_segs) == (12, 0) and np.array_equal(wo, want_wo) and _untouched(zone)
    # no segment
    rc, res, seg, zone, wo, n_wins, n_segs, _ = ctx.scan_extents_raw(*args, 10 ** 6, 1, WINDOW, 0, cap_windows=12, cap_segs=12, fill=FILL)
    assert rc == _ffi.OK and (n_wins, n_segs) == (12, 0) and _untouched(zone)
    assert all(np.array_equal(res[k], want[k]) for k in ARRAYS)
    # no recording
    rc, _, _, zone, wo, n_wins, n_segs, _ = ctx.scan_extents_raw(db.table, np.zeros(1, np.int16), np.zeros(1, np.uint64),
                                                                 np.zeros(1, np.uint32), WINDOW, STEP, 50, 1, WINDOW, 0, cap_segs=2, fill=FILL)
    assert rc == _ffi.OK and (n_wins, n_segs) == (0, 0) and _untouched(zone)


def test_refusals(S, ctx, db, recording):
    from shazam_amd import _ffi
    _, pcm, off, first = _flatten(S, [recording])
    args = (db.table, pcm, off, first)
    room = dict(cap_windows=12, cap_segs=12, fill=FILL)

    def refused(code, *a, **k):
        rc, _, seg, zone, _, _, n_segs, _ = ctx.scan_extents_raw(*a, **dict(room, **k))
        assert rc == code, (rc, code, a[4:], k)
        assert n_segs == 0 and _untouched(zone) and all((v == FILL).all() for v in seg.values())
    refused(_ffi.E_INVALID, *args, WINDOW, STEP, 50, 1, WINDOW, 32)                    # d_tol > 31
    refused(_ffi.E_INVALID, *args, WINDOW, STEP, 50, 1, 1 << 20, 0)                    # margin_frames >= 2^20
    refused(_ffi.E_INVALID, *args, WINDOW, STEP, 50, 1, WINDOW, 0, zones=False)        # NULL zone outputs with cap_segs > 0
    # shz_scan_batch's own refusals come first, with their codes
    refused(_ffi.E_INVALID, *args, 0, STEP, 50, 1, WINDOW, 32)
    refused(_ffi.E_INVALID, *args, 1 << 20, STEP, 50, 1, WINDOW, 0)
    refused(_ffi.E_INVALID, *args, WINDOW, 0, 50, 1, WINDOW, 0)
    refused(_ffi.E_INVALID, *args, WINDOW, STEP, 50, 1, WINDOW, 0, topn=65)
    refused(_ffi.E_INVALID, *args, WINDOW, STEP, 50, 1, WINDOW, 0, fan_value=0)
    refused(_ffi.E_CAPACITY, *args, WINDOW, STEP, 50, 1, WINDOW, 32, cap_windows=11)   # ... and the window capacity before d_tol
    # the table's state, as the match and the extent pass refuse it
    t = _ffi.Table(ctx)
    t.insert(np.array([5], np.uint32), np.array([1], np.uint32), np.array([0], np.uint32))
    refused(_ffi.E_STATE, t, pcm, off, first, WINDOW, STEP, 50, 1, WINDOW, 0)
    t.close()
    # with cap_segs = 0 the zone arrays may be NULL: the call counts the segments
    rc, _, _, _, _, n_wins, n_segs, _ = ctx.scan_extents_raw(*args, WINDOW, STEP, 50, 1, WINDOW, 0, cap_windows=12, cap_segs=0, zones=False)
    assert rc == _ffi.E_CAPACITY and (n_wins, n_segs) == (12, 2)
    # the context still works
    rc, _, _, zone, _, _, n_segs, _ = ctx.scan_extents_raw(*args, WINDOW, STEP, 50, 1, WINDOW, 0, **room)
    assert rc == _ffi.OK and n_segs == 2 and (zone["count"][:2, 0] > 0).all() and (zone["count"][2:] == FILL).all()


# ---- Python -------------------------------------------------------------------------------------------------------------------
def test_scan_with_extents(S, db, recording):
    plain = S.scan([recording], db, min_aligned=50)
    ext = S.scan([recording], db, min_aligned=50, extents=True)
    assert len(plain) == len(ext) == 1 and len(plain[0]) == len(ext[0]) == 2
    new = {"play_start_seconds", "play_end_seconds", "play_first_frame", "play_last_frame", "song_start_seconds", "song_end_seconds",
           "pairs", "extent_hist", "extent_shift", "extent_lo"}
    for p, e in zip(plain[0], ext[0]):
        assert set(e) == set(p) | new
        assert {k: e[k] for k in p} == p
        assert p["start_seconds"] <= e["play_start_seconds"] < e["play_end_seconds"] <= p["end_seconds"]
        assert e["pairs"] == int(e["extent_hist"].sum()) >= e["hashes_aligned"]
        assert e["song_start_seconds"] < e["song_end_seconds"]
        # the song's span and the recording's span are one stretch seen from both sides: the shift maps one to the other
        assert e["play_first_frame"] + e["shift"] >= round(e["song_start_seconds"] * SR / HOP)
        assert e["play_last_frame"] + e["shift"] <= round(e["song_end_seconds"] * SR / HOP) - 1
    a, b = ext[0]
    assert (a["play_first_frame"], a["play_last_frame"], b["play_first_frame"], b["play_last_frame"]) == (64, 191, 194, 297)
    # margin_seconds: None is one window; 0 keeps the zones to the segment's own windows
    tight = S.scan([recording], db, min_aligned=50, extents=True, margin_seconds=0)[0]
    assert tight[0]["extent_lo"] == 0 and tight[1]["extent_lo"] == 8 * STEP and ext[0][1]["extent_lo"] == 8 * STEP - WINDOW
    # delta_tol: d_tol follows it
    wide = S.scan([recording], db, min_aligned=50, extents=True, delta_tol=2)[0]
    assert all(w["pairs"] >= e["pairs"] for w, e in zip(wide, ext[0]))
    assert S.scan([recording], db, min_aligned=10 ** 6, extents=True) == [[]] and S.scan([], db, extents=True) == []
    for kw in (dict(speeds=True), dict(tempos=[65536], pitches=[65536]), dict(warps=([65536], [65536])), dict(search="separable")):
        with pytest.raises(ValueError):
            S.scan([recording], db, extents=True, **kw)
