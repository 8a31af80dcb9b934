"""GPU: shz_scan_plays -- the warp stage on a JOB list (one job per segment and channel, each at the segment's own pair), the
three zones of every segment cut from the jobs' hash lists, and the extent pass with the moments.

- The unity identity: at t16 = f16 = 65536, p = shift + window start and drift_bins 0 every zone output is shz_scan_extents',
  bit for bit, and the sums are Table.match_extents(fit=True)'s on the same queries.
- On the fixture of tests/scan_warp_cases.py every output and the three work counts equal the plain-Python definition
  (tests/scan_play_twin.py, which cuts the FULL warped list of the whole channel), at the default and at small tiles / groups;
  so do built edge cases.
- Refusals, ground truth and scan(extents="fit").

Ground truth (the recording of scan_warp_cases: cuts planted at 2.0, 9.95, 16.95 and 23.95 s, true tempos 1.16, 1.10 and 1.0),
computed FIRST on the CPU with the twin on the numpy oracle's peaks, segments and positions as scan_warp_cases states them,
window 108, step 43, margin one window, tolerance 0:

  drift_bins      pairs kept (pieces 1..3)   play_tempo               |fit - true|              |rung - true|
  0               770, 229, 652              1.16115, 1.08401, 1.0    0.00115, 0.01599, 0       0.00803, 0.01599, 0
  11 (default)    842, 482, 652              1.15890, 1.10014, 1.0    0.00110, 0.00014, 0       (the same)
  22              842, 483, 660              1.15890, 1.09983, 0.99875 0.00110, 0.00017, 0.00125

  border errors at the default, in frames of 46 ms (play_start / play_end minus the planted cut):
      starts -0.07, +6.74, +0.01      ends -1.26, +0.01, -3.72        (drift_bins 0: +21.74 and -32.99 on piece 2)

What the twin does NOT give: piece 2 starts 6.74 frames late (its first dense bucket; its first pair lies at frame 214, the cut
at 214.3), and piece 3 plays at a rung of the ladder, where the fit cannot be nearer than the rung: it EQUALS it (slope 0) at
drift_bins 0 and 11 and is 0.00125 off at 22.  The widest edge bucket is 4 frames (zone_shift 2), so the border bound is 6.74
rounded up to 8, plus one bucket: 12 frames."""
import numpy as np
import pytest

import scan_play_twin as PT
import scan_warp_cases as C

pytestmark = pytest.mark.gpu

SR, HOP = 44100, 2048
WINDOW, STEP = C.WINDOW, C.FIX_STEP
FILL = 77
CUTS = (2.0, 9.95, 16.95, 23.95)
TRUE_TEMPO = (1.16, 1.10, 1.0)
BORDER_FRAMES = 12                # see above
PAIRS = {0: (770, 229, 652), 11: (842, 482, 652), 22: (842, 483, 660)}
WORK = (4546, 17906, 29876)       # peak items warped, hash entries written, zone entries: the twin on the oracle's peaks
# the segments of the fixture with the positions the scan reports for their first and last window
SEGS = tuple((0, sid, a, b, C.DELTA[a], C.DELTA[b], pair[0], pair[1]) for sid, a, b, pair in C.SEGMENTS)


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def recording():
    return C.recording()


@pytest.fixture(scope="module")
def db(S, ctx):
    d, _ = C.make_db(S, ctx, C.songs())
    yield d
    d.close()


@pytest.fixture(scope="module")
def rows(db):
    """The table as the twin reads it, exported once."""
    k, s, o = db.table.export()
    return list(zip(k.tolist(), s.tolist(), o.tolist()))


def _seg(segs):
    from shazam_amd import _ffi
    return {k: np.asarray([s[i] for s in segs], np.int64) for i, (k, _) in enumerate(_ffi.PLAY_SEGMENT_FIELDS)}


def _check(S, db, rows, recordings, segs, window, step, margin, drift, fan=5, flags=None, what=""):
    """One shz_scan_plays against the twin on the device's own peaks: every zone output, the histograms and the three work
    counts -- with and without the debug switches that force the extent pass's small tiles and the scan's small groups."""
    from shazam_amd import _ffi
    ctx = db.ctx
    chans, pcm, off, first = C.flatten(S, recordings)
    peaks, frames = C.device_peaks(ctx, chans, pcm, off, first)
    chan_peaks = [p for rec in peaks for p in rec]
    want, work = PT.zone_results(rows, chan_peaks, first, segs, frames, window, step, margin, ctx.vote_tolerance + drift, fan)
    zone = None
    for flag in ((0, _ffi.DEBUG_EXTENT_SMALL_TILES | _ffi.DEBUG_SCAN_SMALL_GROUPS) if flags is None else flags):
        ctx.set_debug(flag)
        try:
            zone, got_work, ms = ctx.scan_plays(db.table, pcm, off, first, window, step, _seg(segs), margin, drift, fan_value=fan)
        finally:
            ctx.set_debug(0)
        PT.assert_zones(zone, want, (what, flag))
        assert got_work == work, (what, flag, got_work, work)
        assert len(ms) == 3 and all(m >= 0.0 for m in ms)
        assert np.array_equal(zone["hist"].sum(axis=2), zone["count"]), (what, flag)
    return zone, work, frames


# ---- the unity identity against shz_scan_extents, on the fixture of tests/test_gpu_scan_extents.py --------------------------
def test_unity_is_scan_extents_bit_for_bit(S, ctx):
    from oracle import synth
    from shazam_amd import _ffi
    songs = [synth.music_clip(11, c, 8 * SR) for c in range(4)]
    rec = np.concatenate([synth.traffic_noise(5, 0, 3 * SR), songs[1][SR:7 * SR], songs[3][0:5 * SR], synth.traffic_noise(5, 1, 2 * SR)])
    d = S.get_database("hip")(ctx=ctx)
    try:
        k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
        for c in range(4):
            assert d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c])) == c + 1
            d.set_song_fingerprinted(c + 1)
        d.table.insert_clips(k, t1, ho, 1)
        d.table.finalize()
        window, step = 108, 22
        for batch, margin, tol in (([rec], 108, 0), ([rec, [rec, rec[:4 * SR + 777]]], 40, 2)):
            chans, pcm, off, first = C.flatten(S, batch)
            with ctx.tolerance(tol):
                res, wo, seg, ext, _ = ctx.scan_extents(d.table, pcm, off, first, window, step, 50, 1, margin, tol)
                n = len(seg["rec"])
                assert n >= 2 and (tol or [tuple(int(seg[f][i]) for f in ("rec", "sid", "shift", "first", "last")) for i in range(2)] ==
                                   [(0, 2, -43, 0, 7), (0, 4, -194, 8, 11)])
                plays = dict(rec=seg["rec"], sid=seg["sid"], first=seg["first"], last=seg["last"],
                             pos_first=seg["shift"] + seg["first"].astype(np.int64) * step,
                             pos_last=seg["shift"] + seg["last"].astype(np.int64) * step, t16=np.full(n, 65536), f16=np.full(n, 65536))
                zone, work, _ = ctx.scan_plays(d.table, pcm, off, first, window, step, plays, margin, 0)
                # the sums: Table.match_extents(fit=True) on the zones' queries, built on the host from the extraction's hashes
                hk, ht, hho = S.fingerprint_batch(chans, ctx=ctx)
                keys, qoffs, qoff = [], [], [0]
                for i in range(n):
                    for z in range(3):
                        lo, hi, m = int(ext["lo"][i, z]), int(ext["hi"][i, z]), 0
                        for c in range(int(first[seg["rec"][i]]), int(first[seg["rec"][i] + 1])):
                            kk, tt = hk[int(hho[c]):int(hho[c + 1])], ht[int(hho[c]):int(hho[c + 1])].astype(np.int64)
                            sel = (tt >= lo) & (tt < hi)
                            keys.append(kk[sel])
                            qoffs.append((tt[sel] - lo).astype(np.uint32))
                            m += int(sel.sum())
                        qoff.append(qoff[-1] + m)
                ref = d.table.match_extents(np.concatenate(keys), np.concatenate(qoffs), np.asarray(qoff, np.uint64),
                                            np.repeat(seg["sid"], 3).reshape(-1, 1), zone["d_lo"].reshape(-1, 1),
                                            zone["d_hi"].reshape(-1, 1), fit=True)
            for f in _ffi.ZONE_FIELDS + ("hist",):
                assert zone[f].dtype == ext[f].dtype and np.array_equal(zone[f], ext[f]), (f, tol)
            shift = seg["shift"].astype(np.int64)[:, None]
            assert np.array_equal(zone["d_lo"], shift + ext["lo"] - tol) and np.array_equal(zone["d_hi"], shift + ext["lo"] + tol)
            for f in ("sum_q", "sum_u", "sum_qq", "sum_qu"):
                assert np.array_equal(zone[f].reshape(-1), ref[f].reshape(-1)), (f, tol)
            assert np.array_equal(zone["count"].reshape(-1), ref["count"].reshape(-1)) and zone["count"].sum() > 0
            assert work[2] == qoff[-1] and work[0] > 0 and work[1] >= work[2] // 3
    finally:
        d.close()


# ---- the fixture of scan_warp_cases: every output and the work counts against the twin ---------------------------------------
def test_segments_of_the_warped_scan_against_the_twin(S, ctx, db, rows, recording):
    assert ctx.frames_of(len(recording)) == 537
    for drift in (0, 11, 22):
        zone, work, _ = _check(S, db, rows, [recording], SEGS, WINDOW, STEP, WINDOW, drift, what=("fixture", drift))
        print("drift_bins", drift, "pairs", zone["count"][:, 0].tolist(), "work", work)
        assert tuple(zone["count"][:, 0].tolist()) == PAIRS[drift], "the pairs the CPU twin kept on the oracle's peaks"
        assert work == WORK
    # two segments of one recording at different pairs is what the fixture is; margins 0 and far beyond the recording
    for margin in (0, 5000):
        _check(S, db, rows, [recording], SEGS, WINDOW, STEP, margin, 11, flags=(0,), what=("margin", margin))


def test_tolerance_and_drift_bins_add_up(S, ctx, db, rows, recording):
    with ctx.tolerance(2):
        for drift in (0, 5):
            zone, _, _ = _check(S, db, rows, [recording], SEGS, WINDOW, STEP, WINDOW, drift, flags=(0,), what=("tolerance 2", drift))
            assert (zone["d_hi"][:, 1] - zone["d_lo"][:, 1]).tolist() == [2 * (2 + drift)] * 3


# ---- built edge cases, each against the twin -----------------------------------------------------------------------------------
WIDE = 1500                       # drift_bins of the edge cases: candidates 3,001 bins wide collect chance pairs at any pair


def test_a_time_group_straddling_the_border_at_half_tempo(S, ctx, db, rows, recording):
    """t16 = 32768: W(x) = (x + 1) >> 1, so an even lo shares its warped frame with lo - 1.  The peaks of own frame lo - 1
    belong to the zone's first t' group: the job keeps whole groups, and sp_place's merge of the two frames sees both."""
    chans, pcm, off, first = C.flatten(S, [recording])
    pt = C.device_peaks(ctx, chans, pcm, off, first)[0][0][0][1]
    a = 2
    margin = next(m for m in range(2, 60, 2) if (pt == a * STEP - m - 1).any() and (pt == a * STEP - m).any())
    lo = a * STEP - margin
    assert lo % 2 == 0 and PT.W(lo - 1, 32768) == PT.W(lo, 32768)
    for f16 in (65536, 32768, 131072):
        zone, _, _ = _check(S, db, rows, [recording], [(0, 1, a, 4, 0, 40, 32768, f16)], WINDOW, STEP, margin, WIDE,
                            what=("straddle", f16))
        assert zone["lo"][0].tolist() == [lo, lo, 4 * STEP]


def test_double_tempo_half_pitch_and_the_halo_past_the_end(S, ctx, db, rows, recording):
    # t16 = 131072: no two frames share a t'; f16 = 32768: f' = 2 f, the peaks above bin 1024 leave, at a job's edges too;
    # the last window reaches the recording's end: hi = F and the 200-frame halo runs past the clip's last peak
    for t16, f16 in ((131072, 65536), (65536, 32768), (131072, 32768), (54524, 67511)):
        zone, work, frames = _check(S, db, rows, [recording], [(0, 1, 0, 3, 0, 100, t16, f16), (0, 3, 7, 10, -64, 65, t16, f16)],
                                    WINDOW, STEP, 30, WIDE, flags=(0,), what=("pair", t16, f16))
        assert zone["hi"][1].tolist() == [537, 7 * STEP + WINDOW, 537] and frames == [537]
        assert work[0] > 256, "one job of more than a workgroup's items"


@pytest.mark.parametrize("fan", [1, 64])
def test_fan_values(S, ctx, db, rows, recording, fan):
    zone, work, _ = _check(S, db, rows, [recording], SEGS[:2], WINDOW, STEP, 20, 11, fan=fan, flags=(0,), what=("fan", fan))
    assert (work[1] == 0 and not zone["count"].any()) if fan == 1 else work[1] > 10 * work[0]


def test_stereo_empty_shorter_and_duplicated_channels(S, ctx, db, rows, recording):
    part = recording[:12 * SR]
    batch = [[part, part[:5 * SR + 777]], [part, part], [np.zeros(0, np.int16), part], part]
    segs = [(r, sid, a, b, pa, pb, t16, f16) for r in range(4) for _, sid, a, b, pa, pb, t16, f16 in SEGS[:2]]
    zone, work, frames = _check(S, db, rows, batch, segs, WINDOW, STEP, 40, 11, what="stereo")
    assert frames == [ctx.frames_of(12 * SR)] * 4 and frames[0] < 5 * STEP + WINDOW and zone["count"][:, 0].any()
    # a duplicated channel and an empty one change nothing (the set semantics): the mono recording's zones
    for f in PT.ZONE_KEYS + ("hist",):
        for r in (1, 2):
            assert np.array_equal(zone[f][2 * r:2 * r + 2], zone[f][6:8]), (f, r)


def test_many_jobs_with_empty_ones_between(S, ctx, db, rows, recording):
    """130 one-window segments of a stereo recording whose second channel is empty: 260 jobs, more than one workgroup of the
    range kernel, every second one without a peak -- and some of the others without one too (4-frame windows of noise)"""
    window, step = 8, 4
    pairs = [(65536, 65536), (60030, 63561), (76548, 67511), (32768, 131072)]
    segs = [(0, 1 + i % 4, i, i, i * step, i * step, *pairs[i % 4]) for i in range(130)]
    segs.append((1, 1, 0, 132, -50, 600, 76548, 65536))
    zone, work, frames = _check(S, db, rows, [[recording, np.zeros(0, np.int16)], recording], segs, window, step, 0, 40, what="jobs")
    assert len(segs) * 2 - 1 > 256 and frames == [537, 537] and work[0] > 256


# ---- refusals: before the first launch, nothing is written ----------------------------------------------------------------------
def _refused(ctx, db, code, pcm, off, first, segs, window, step, margin, drift, what, **kw):
    rc, zone, work, ms = ctx.scan_plays_raw(db.table, pcm, off, first, window, step, _seg(segs), margin, drift, fill=FILL, **kw)
    assert rc == code, (what, rc)
    assert all((v == FILL).all() for v in zone.values()) and work == (FILL,) * 3, what
    return zone


def test_refusals(S, ctx, db, rows, recording):
    from shazam_amd import _ffi
    chans, pcm, off, first = C.flatten(S, [recording])
    one = [(0, 1, 0, 4, 0, 172 + 4095 - 6, 65536, 65536)]          # c_a = 0, c_b = 4089: with w = 3 the whole zone spans 4,095 bins
    _check(S, db, rows, [recording], one, WINDOW, STEP, 0, 3, flags=(0,), what="width 4095")
    wide = [one[0][:5] + (one[0][5] + 1,) + one[0][6:]]
    _refused(ctx, db, _ffi.E_UNSUPPORTED, pcm, off, first, wide, WINDOW, STEP, 0, 3, "width 4096")
    with ctx.tolerance(1):
        _refused(ctx, db, _ffi.E_UNSUPPORTED, pcm, off, first, one, WINDOW, STEP, 0, 3, "width 4097 by the tolerance")
    _refused(ctx, db, _ffi.E_UNSUPPORTED, pcm, off, first, [SEGS[0]], WINDOW, STEP, 0, 2048, "drift_bins 2048")
    # the zone-length limit: 2^19 frames at factor 2 are 2^20 warped frames.  The frame counts follow from clip_off alone and the
    # call refuses before it touches the audio, so a clip_off that promises 2^19 + 1 frames needs no such buffer
    huge = np.asarray([0, ((1 << 19) + 2) * HOP], np.uint64)
    assert ctx.frames_of(int(huge[1])) >= 1 << 19
    _refused(ctx, db, _ffi.E_UNSUPPORTED, np.zeros(16, np.int16), huge, first, [(0, 1, 0, 0, 0, 0, 131072, 65536)], 1 << 19, 1, 0, 0,
             "zone length")
    # the rest, in the documented order
    bad = lambda i, v: [SEGS[0][:i] + (v,) + SEGS[0][i + 1:]]     # noqa: E731
    for code, segs, window, step, margin, kw, what in (
            (_ffi.E_INVALID, SEGS, 0, STEP, 0, {}, "window 0"), (_ffi.E_INVALID, SEGS, 1 << 20, STEP, 0, {}, "window 2^20"),
            (_ffi.E_INVALID, SEGS, WINDOW, 0, 0, {}, "step 0"), (_ffi.E_INVALID, SEGS, WINDOW, STEP, 0, dict(fan_value=0), "fan 0"),
            (_ffi.E_INVALID, SEGS, WINDOW, STEP, 0, dict(fan_value=65), "fan 65"), (_ffi.E_INVALID, SEGS, WINDOW, STEP, 1 << 20, {}, "margin"),
            (_ffi.E_INVALID, bad(0, 1), WINDOW, STEP, 0, {}, "rec"), (_ffi.E_INVALID, bad(2, 5), WINDOW, STEP, 0, {}, "first > last"),
            (_ffi.E_INVALID, bad(6, 32767), WINDOW, STEP, 0, {}, "t16"), (_ffi.E_INVALID, bad(7, 131073), WINDOW, STEP, 0, {}, "f16"),
            (_ffi.E_INVALID, SEGS[::-1], WINDOW, STEP, 0, {}, "order")):
        _refused(ctx, db, code, pcm, off, first, segs, window, step, margin, 0, what, **kw)
    # no segment: SHZ_OK, nothing launched, nothing written (not even the work counts)
    rc, zone, work, ms = ctx.scan_plays_raw(db.table, pcm, off, first, WINDOW, STEP, _seg([]), 0, 0, fill=FILL)
    assert rc == _ffi.OK and work == (FILL,) * 3 and ms == (0.0, 0.0, 0.0) and zone["lo"].shape == (0, 3)
    # a table that is not finalized
    t = _ffi.Table(ctx)
    try:
        t.insert(np.zeros(1, np.uint32), np.ones(1, np.uint32), np.zeros(1, np.uint32))
        rc, zone, work, _ = ctx.scan_plays_raw(t, pcm, off, first, WINDOW, STEP, _seg(SEGS), 0, 0, fill=FILL)
        assert rc == _ffi.E_STATE and (zone["count"] == FILL).all()
    finally:
        t.close()


# ---- scan(extents="fit"): the keys, and the ground truth ------------------------------------------------------------------------
def test_scan_fit_keys_and_ground_truth(S, ctx, db, recording):
    kw = dict(tempos=C.TEMPOS, pitches=C.PITCHES, min_aligned=C.MIN_ALIGNED, step_seconds=2)
    plain = S.scan([recording], db, **kw)[0]
    fit = S.scan([recording], db, extents="fit", **kw)[0]
    assert [(s["song_id"], s["first_window"], s["last_window"], s["pos_first"], s["pos_last"]) for s in fit] == \
        [(sid, a, b, pa, pb) for _, sid, a, b, pa, pb, _, _ in SEGS]
    frame = HOP / SR
    for i, (p, f) in enumerate(zip(plain, fit)):
        assert all(f[k] == p[k] for k in p), "every existing key keeps its value"
        assert set(f) - set(p) == {"play_start_seconds", "play_end_seconds", "play_first_frame", "play_last_frame", "song_start_seconds",
                                   "song_end_seconds", "pairs", "extent_hist", "extent_shift", "extent_lo", "fit", "play_tempo"}
        print("piece", i, {k: f[k] for k in ("play_start_seconds", "play_end_seconds", "play_first_frame", "play_last_frame",
                                             "song_start_seconds", "song_end_seconds", "pairs", "play_tempo", "tempo", "tempo_fit")})
        # the borders: within BORDER_FRAMES of the planted cuts (the window-grained ones are off by up to 2 s = 43 frames)
        assert abs(f["play_start_seconds"] - CUTS[i]) <= BORDER_FRAMES * frame, (i, f["play_start_seconds"])
        assert abs(f["play_end_seconds"] - CUTS[i + 1]) <= BORDER_FRAMES * frame, (i, f["play_end_seconds"])
        assert f["pairs"] == PAIRS[11][i] == f["fit"]["count"] and int(f["extent_hist"].sum()) == f["pairs"]
        assert f["song_start_seconds"] is not None and f["song_start_seconds"] <= 1.21
        # the tempo: nearer than the rung on the two pieces that play beside a rung; piece 3 plays AT a rung, the fit equals it
        rung_err, fit_err = abs(f["tempo"] - TRUE_TEMPO[i]), abs(f["play_tempo"] - TRUE_TEMPO[i])
        assert (fit_err < rung_err and fit_err <= 0.0012) if i < 2 else (f["play_tempo"] == f["tempo"] == 1.0), (i, f["play_tempo"])
    assert abs(fit[1]["play_tempo"] - 1.10) < 0.0002 < abs(fit[1]["tempo"] - 1.10)
    # drift_bins 0: only the rung's own bin, so piece 2 (rung 1.084, true 1.10) keeps fewer than half of its pairs and fits its rung
    zero = S.scan([recording], db, extents="fit", drift_bins=0, **kw)[0]
    assert [s["pairs"] for s in zero] == list(PAIRS[0]) and zero[1]["play_tempo"] == zero[1]["tempo"]
    # the separable search and a pair list reach the same plays; a margin of its own
    sep = S.scan([recording], db, extents="fit", search="separable", margin_seconds=1.0, **kw)[0]
    assert [s["song_id"] for s in sep] == [s["song_id"] for s in fit] and all(s["pairs"] > 0 and s["play_tempo"] is not None for s in sep)
    assert S.scan([recording], db, extents="fit", **dict(kw, min_aligned=10 ** 6)) == [[]] and S.scan([], db, extents="fit", **kw) == []


def test_scan_fit_with_a_speed_ladder_and_what_is_refused(S, ctx, db, recording):
    from shazam_amd.speed import speed_ladder
    kw = dict(speeds=speed_ladder(0.97, 1.03), min_aligned=40, step_seconds=2)
    plain = S.scan([recording], db, **kw)[0]
    fit = S.scan([recording], db, extents="fit", **kw)[0]
    assert len(plain) == len(fit) >= 1
    for p, f in zip(plain, fit):
        assert all(f[k] == p[k] for k in p) and "play_speed" in f and "play_tempo" not in f
        assert f["pairs"] >= 0 and (f["play_speed"] is None or 0.5 <= f["play_speed"] <= 2.0)
        assert f["start_seconds"] - 5.01 <= f["play_start_seconds"] and f["play_end_seconds"] <= f["end_seconds"] + 5.01   # (the margin)
    with pytest.raises(ValueError, match="extents=True"):
        S.scan([recording], db, extents="fit")
    with pytest.raises(ValueError, match='extents="fit"'):
        S.scan([recording], db, extents=True, speeds=True)
    with pytest.raises(ValueError):
        S.scan([recording], db, extents="full", speeds=True)
