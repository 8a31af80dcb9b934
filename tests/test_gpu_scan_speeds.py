"""GPU: shz_scan_speeds -- the peaks of every recording extracted once, warped for every rung of a ladder, the warped hash
lists cut into the recording's windows on the device and every (window, rung) matched -- gives, array for array, what the
host recipe gives: shz_peaks, the numpy twin of the warp per channel and rung (tests/speed_twin.py), the twin's window cut
(tests/scan_speed_twin.py), Table.match on those queries and the best-rung rule.  On a recording assembled from two table
songs pitched by +3 % and -3 % between noise, rank 0 is the CPU oracle's vote, scan(speeds=...) returns the two segments
with their speeds, and the plain scan finds nothing.  Batch shapes that can go wrong, slicing, another hop, rungs that
fold two frames into one, refusals, memory."""
import numpy as np
import pytest

import scan_speed_twin as ST
import speed_twin as T

pytestmark = pytest.mark.gpu

ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
WINDOW, STEP = 108, 22            # round(5 s * 44100 / 2048), round(1 s * 44100 / 2048)
SR = 44100
RUNG = 92                         # the default grid's step, Q16
LADDER = np.asarray([63512, 63604, 63696, 65444, 65536, 65628, 67376, 67468, 67560], np.uint32)
THREE = np.asarray([63604, 65536, 67468], np.uint32)
# measured on the CPU oracle + twins: the song frame at the start of windows 0-9 (song 2 at 1.03) and 10-19 (song 4 at 0.97)
FAST = [-23, 0, 22, 45, 68, 90, 113, 136, 158, 181]
SLOW = [-58, -36, -15, 6, 27, 49, 70, 91, 112, 134]


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
    return [synth.music_clip(7, c, 20 * SR) for c in range(4)]


def _pitched(song, second, seconds, s):
    return T.speed_up(song[second * SR: second * SR + int(seconds * SR * s) + 2], s)[:seconds * SR]


@pytest.fixture(scope="module")
def recording(songs):
    from oracle import synth
    return np.concatenate([synth.traffic_noise(5, 0, 3 * SR), _pitched(songs[1], 2, 10, 1.03), _pitched(songs[3], 0, 9, 0.97),
                           synth.traffic_noise(5, 1, 2 * SR)])


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    """Songs 1..4; returns (db, key32 -> [(sid, offset)]): one set of rows for the device table and for the CPU vote."""
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    per_song = []
    for c in range(4):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        assert sid == c + 1
        d.set_song_fingerprinted(sid)
        per_song.append((k[int(ho[c]):int(ho[c + 1])], t1[int(ho[c]):int(ho[c + 1])]))
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    yield d, T.table_of(per_song)
    d.close()


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


def _recipe(ctx, chans, pcm, off, first, window, step, ladder):
    """The host recipe's queries: peaks from the device extraction, everything behind them in numpy."""
    pf, pt, po = ctx.peaks(pcm, off)
    peaks, frames = [], []
    for r in range(len(first) - 1):
        cs = range(int(first[r]), int(first[r + 1]))
        peaks.append([(pf[int(po[c]):int(po[c + 1])], pt[int(po[c]):int(po[c + 1])]) for c in cs])
        frames.append(max((ctx.frames_of(len(chans[c])) for c in cs), default=0))
    return ST.host_queries(peaks, frames, window, step, ladder.tolist())


def _same(got, want, what=""):
    for name in ARRAYS + ("best", "profile"):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (what, name)


def _check(S, db, recordings, window, step, ladder, topns=(2,), full_sorts=(False,), what=""):
    """scan_speeds against the recipe; returns the last result and win_off."""
    ctx = db.ctx
    chans, pcm, off, first = _flatten(S, recordings)
    hk, hq, hqo, hwo = _recipe(ctx, chans, pcm, off, first, window, step, ladder)
    for topn in topns:
        for fs_ in full_sorts:
            m = db.table.match(hk, hq, hqo, topn, full_sort=fs_)
            want = ST.fold_best(m, int(hwo[-1]), ladder.tolist(), topn)
            got, win_off, ms = ctx.scan_speeds(db.table, pcm, off, first, window, step, ladder, topn=topn, full_sort=fs_)
            assert np.array_equal(win_off, hwo), (what, win_off, hwo)
            _same(got, want, (what, topn, fs_))
            assert len(ms) == 4 and all(x >= 0.0 for x in ms)
    return got, win_off


# ---- the recipe -------------------------------------------------------------------------------------------------------
def test_recipe_equals_match_and_oracle(S, ctx, db, recording):
    from oracle import cpu_ref as O
    d, table = db
    assert ctx.frames_of(len(recording)) == 515
    got, win_off = _check(S, d, [recording], WINDOW, STEP, LADDER, topns=(1, 2), full_sorts=(False, True), what="recipe")
    assert win_off.tolist() == [0, 20]
    print("best:", got["best"].tolist())
    print("delta:", got["delta"][:, 0].tolist())
    print("aligned:", got["aligned"][:, 0].tolist())
    print("unity rung:", got["profile"][:, 4].tolist())
    # rank 0 of every (window, rung) is the reference's vote on the oracle's peaks, warped and cut by the twins
    f, t = O.fingerprint_keys(recording)[2:]
    for v, s16 in enumerate(LADDER.tolist()):
        cut = ST.cut_windows([T.warp_pair(f, t, s16)], 20, WINDOW, STEP, s16)
        for w, (k, q) in enumerate(cut):
            ranked, dedup, nhash = T.aligned_votes(k, q, table, 1)
            assert int(got["profile"][w, v]) == (ranked[0][2] if ranked else 0), (w, v)
            if v == int(got["best"][w]):
                sid, delta, aligned = ranked[0]
                assert (int(got["sid"][w, 0]), int(got["delta"][w, 0]), int(got["aligned"][w, 0])) == (sid, delta, aligned), w
                assert int(got["nhash"][w]) == nhash and int(got["dedup"][w, 0]) == dedup[sid]
    # what was measured on the CPU: the songs, their positions, the rungs; the unity rung alone sees noise
    assert got["sid"][:10, 0].tolist() == [2] * 10 and got["sid"][10:, 0].tolist() == [4] * 10
    assert got["delta"][:, 0].tolist() == FAST + SLOW
    assert got["best"][:10].tolist() == [7] * 10 and set(got["best"][10:].tolist()) <= {0, 1}
    assert 57 <= int(got["aligned"][:10, 0].min()) and int(got["aligned"][:10, 0].max()) <= 142
    assert 54 <= int(got["aligned"][10:, 0].min()) and int(got["aligned"][10:, 0].max()) <= 96
    assert int(got["profile"][:, 4].max()) <= 16


def test_unity_ladder_is_the_plain_scan(S, ctx, db, recording, mixed_batch):
    d, _ = db
    for recs, window, step in (([recording], WINDOW, STEP), (mixed_batch, 40, 15)):
        _, pcm, off, first = _flatten(S, recs)
        for topn in (1, 3):
            want, wo0, _ = ctx.scan_batch(d.table, pcm, off, first, window, step, topn=topn)
            got, wo1, _ = ctx.scan_speeds(d.table, pcm, off, first, window, step, np.asarray([65536], np.uint32), topn=topn)
            assert np.array_equal(wo0, wo1) and len(want["nres"]) > 3
            for name in ARRAYS:
                assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, topn)
            assert not got["best"].any()
            assert np.array_equal(got["profile"][:, 0], np.where(want["nres"] > 0, want["aligned"][:, 0], 0))


def test_scan_returns_the_two_pitched_segments(S, db, recording):
    d, _ = db
    segs = S.scan([recording], d, speeds=LADDER, min_aligned=40)
    assert len(segs) == 1
    print(segs[0])
    assert len(segs[0]) == 2
    a, b = segs[0]
    assert (a["song_id"], a["first_window"], a["last_window"], a["windows"]) == (2, 0, 9, 10)
    assert (b["song_id"], b["first_window"], b["last_window"], b["windows"]) == (4, 10, 19, 10)
    assert abs(a["speed"] * 65536 - T.q16(1.03)) <= RUNG and abs(b["speed"] * 65536 - T.q16(0.97)) <= RUNG
    assert abs(a["pos_first"] - FAST[0]) <= 1 and abs(b["pos_first"] - SLOW[0]) <= 1
    assert abs(a["pos_last"] - FAST[-1]) <= 1 and abs(b["pos_last"] - SLOW[-1]) <= 1
    assert a["offset_seconds"] == round(a["pos_first"] / SR * 2048, 5) and b["offset_seconds"] == round(b["pos_first"] / SR * 2048, 5)
    assert a["speed_fit"] == (a["pos_last"] - a["pos_first"]) / (9 * STEP) and abs(a["speed_fit"] - 1.03) < 0.01
    assert abs(b["speed_fit"] - 0.97) < 0.01
    assert a["start_seconds"] == 0.0 and b["end_seconds"] == round(515 * 2048 / SR, 5)
    assert a["song_name"] == b"song1" and b["song_name"] == b"song3"
    # the raw arrays carry the ladder and the chosen factor per window
    w = S.scan_windows([recording], d, speeds=LADDER)
    assert w["profile"].shape == (20, 9) and np.array_equal(w["speeds"], LADDER) and len(w["ms"]) == 4
    assert np.array_equal(w["speed"], LADDER[w["best"]] / 65536.0)
    # the plain scan misses every pitched window: the feature, end to end
    assert S.scan([recording], d, min_aligned=40) == [[]]
    assert S.scan([], d, speeds=LADDER) == []


# ---- batch shapes that can go wrong -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch(songs, recording):
    from oracle import synth
    part = recording[2 * SR:9 * SR]
    return [
        [part, synth.mix_query(part, synth.traffic_noise(6, 3, len(part)), 3.0)],     # stereo, the second channel noise-mixed
        [],                                                                          # no clips: no window
        songs[1][:3000],                                                             # shorter than one window: one window
        [songs[2][:5 * SR], songs[2][:3 * SR + 777]],                                # channels of unequal length
    ]


def test_mixed_batch(S, db, mixed_batch):
    d, _ = db
    got, win_off = _check(S, d, mixed_batch, 40, 15, THREE, topns=(1, 3), what="mixed")
    counts = np.diff(win_off.astype(np.int64)).tolist()
    assert counts[0] > 3 and counts[1] == 0 and counts[2] == 1 and counts[3] > 1
    assert got["nres"][:counts[0]].any()


def test_recordings_without_clips_only(S, ctx, db):
    d, _ = db
    got, win_off, _ = ctx.scan_speeds(d.table, np.zeros(1, np.int16), np.zeros(1, np.uint64), np.zeros(3, np.uint32), WINDOW, STEP, THREE)
    assert win_off.tolist() == [0, 0, 0] and got["best"].shape == (0,) and got["profile"].shape == (0, 3)


def test_thirty_frames_window_one_and_step_above_window(S, ctx, db, songs):
    d, _ = db
    clip = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048]
    assert ctx.frames_of(len(clip)) == 30
    got, win_off = _check(S, d, [clip, clip[:20000]], 1, 4, THREE, what="window 1, step 4")
    assert win_off.tolist() == [0, 9, 12]
    assert np.any(got["nhash"] == 0) and np.any(got["nhash"] > 0)
    _check(S, d, [clip], 4, 9, THREE, what="step > window")


def test_step_that_puts_a_window_beyond_every_t1(S, ctx, db, songs):
    """Step 2^32 - 1: the second window starts above every t1' at every rung and is empty (test_gpu_scan.py has the reason)."""
    d, _ = db
    clip = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048]
    near, _ = _check(S, d, [clip], 4, 1, THREE, what="window 4 step 1")
    got, win_off = _check(S, d, [clip], 4, (1 << 32) - 1, THREE, what="step 2^32 - 1")
    assert win_off.tolist() == [0, 2]
    assert int(got["nhash"][1]) == 0 and int(got["nres"][1]) == 0 and not got["profile"][1].any()
    for name in ARRAYS + ("best", "profile"):
        assert np.array_equal(got[name][0], near[name][0]), name


def test_recordings_without_windows_front_middle_and_end(S, ctx, db, songs):
    """The descriptor search steps over recordings without windows, here with slices of one recording too (test_gpu_scan.py)."""
    from shazam_amd import _ffi
    d, _ = db
    a, b = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048], songs[1][3 * SR:3 * SR + 4096 + 29 * 2048]
    recs = [[], a, [], [], [b, b[:20000]], []]
    for debug in (0, _ffi.DEBUG_SCAN_SPEED_SMALL_SLICES):
        ctx.set_debug(debug)
        try:
            got, win_off = _check(S, d, recs, 4, 9, THREE, what=("empty recordings", debug))
        finally:
            ctx.set_debug(0)
        assert win_off.tolist() == [0, 0, 4, 4, 4, 8, 8]
        assert got["nhash"][:4].any() and got["nhash"][4:].any()


# ---- slicing ----------------------------------------------------------------------------------------------------------
def test_small_slices_and_device_pcm_give_the_same_arrays(S, ctx, db, recording, mixed_batch):
    from shazam_amd import _ffi
    d, _ = db
    for recs, window, step, ladder in (([recording], WINDOW, STEP, LADDER), (mixed_batch, 40, 15, LADDER[2:7]), (mixed_batch, 3, 2, THREE)):
        _, pcm, off, first = _flatten(S, recs)
        buf = ctx.alloc(pcm.nbytes)
        buf.upload(pcm)
        try:
            for full_sort in (False, True):
                want, wo0, _ = ctx.scan_speeds(d.table, pcm, off, first, window, step, ladder, topn=3, full_sort=full_sort)
                ctx.set_debug(_ffi.DEBUG_SCAN_SPEED_SMALL_SLICES)     # 1 recording x 2 rungs a slice, 3 windows a match group
                try:
                    got, wo1, _ = ctx.scan_speeds(d.table, buf, off, first, window, step, ladder, topn=3, full_sort=full_sort,
                                                  pcm_device=True)
                finally:
                    ctx.set_debug(0)
                assert len(want["nres"]) > 3 and np.array_equal(wo0, wo1)
                _same(got, want, ("small slices", window, step, full_sort))
        finally:
            buf.free()


def test_hop_1024(S, ctx, db, recording):
    """Another hop (shz_set_overlap): twice the frames, the windows counted and cut at that hop."""
    d, _ = db
    part = recording[4 * SR:9 * SR]
    ctx.set_overlap(4096 - 1024)
    try:
        assert ctx.frames_of(len(part)) == (len(part) - 4096) // 1024 + 1
        got, win_off = _check(S, d, [part, [part[:SR], part[SR:3 * SR]]], 50, 30, THREE, what="hop 1024")
        assert int(win_off[1]) == ST.window_count(ctx.frames_of(len(part)), 50, 30)
    finally:
        ctx.set_overlap(2048)


def test_rungs_that_fold_two_frames_into_one(S, ctx, db, recording):
    """Below unity two neighbouring frames can share one t' (at 32768: frames 2 k - 1 and 2 k), the warp re-orders their
    peaks, and a window that starts at an even frame starts in the middle of such a pair: the peaks of the frame in front
    of it belong to it."""
    d, _ = db
    part = recording[3 * SR:10 * SR]
    ladder = np.asarray([32768, 40000], np.uint32)
    _, pcm, off, _ = _flatten(S, [part])
    _, pt, _ = ctx.peaks(pcm, off)
    shared = [w for w in range(1, 8) if ST.W(w * 15 - 1, 32768) == ST.W(w * 15, 32768) and np.any(pt == w * 15 - 1) and np.any(pt == w * 15)]
    assert shared, "a window start whose frame shares its t' with the frame in front of it, peaks in both"
    got, _ = _check(S, d, [part], 40, 15, ladder, topns=(1, 2), what="folding rungs")
    assert got["nhash"].any() and got["nres"].any()
    _check(S, d, [[part, part[SR:]]], 7, 2, ladder, what="folding rungs, short windows, stereo")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(S, ctx, db, recording, songs):
    from shazam_amd import _ffi
    d, _ = db
    recs = [recording[:6 * SR], [songs[0][:3 * SR], songs[1][:3 * SR]]]
    _, pcm, off, first = _flatten(S, recs)
    u32 = lambda *xs: np.asarray(xs, np.uint32)   # noqa: E731
    ctx.scan_speeds(d.table, pcm, off, first, (1 << 19) - 1, STEP, u32(131072))   # the longest window still taken: 2^20 - 2 warped frames
    want, wo, _ = ctx.scan_speeds(d.table, pcm, off, first, WINDOW, STEP, THREE)
    total = int(wo[-1])
    before = (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats(), d.table.rows(), ctx.mem_info()[0])
    ok = dict(window_frames=WINDOW, step_frames=STEP, speeds=THREE)
    for what, rc0, kw, code in (
            ("empty ladder", first, dict(ok, speeds=u32()), _ffi.E_INVALID),
            ("1025 rungs", first, dict(ok, speeds=np.full(1025, 65536, np.uint32)), _ffi.E_INVALID),
            ("rung below 0.5", first, dict(ok, speeds=u32(65536, 32767)), _ffi.E_INVALID),
            ("rung above 2", first, dict(ok, speeds=u32(131073, 65536)), _ffi.E_INVALID),
            ("window 0", first, dict(ok, window_frames=0), _ffi.E_INVALID),
            ("window 2^20", first, dict(ok, window_frames=1 << 20), _ffi.E_INVALID),
            ("step 0", first, dict(ok, step_frames=0), _ffi.E_INVALID),
            ("topn 0", first, dict(ok, topn=0), _ffi.E_INVALID),
            ("rec_clip0 not ascending", u32(0, 2, 1, 3), ok, _ffi.E_INVALID),
            ("warped window of 2^20", first, dict(ok, window_frames=1 << 19, speeds=u32(65536, 131072)), _ffi.E_UNSUPPORTED),
            ("warped window above 2^20", first, dict(ok, window_frames=(1 << 20) - 1, speeds=u32(65537)), _ffi.E_UNSUPPORTED),
            ("room for one window less", first, dict(ok, cap_windows=total - 1), _ffi.E_CAPACITY),
            ("no room", first, dict(ok, cap_windows=0), _ffi.E_CAPACITY)):
        kw = dict(kw)
        args = (kw.pop("window_frames"), kw.pop("step_frames"), kw.pop("speeds"))
        with pytest.raises(_ffi.ShzError) as e:
            ctx.scan_speeds(d.table, pcm, off, rc0, *args, **kw)
        assert e.value.code == code, what
        if code == _ffi.E_CAPACITY:
            assert f"{total} windows" in str(e.value), "the message names the total"
    # nothing ran: no extraction, no match, no allocation, the table as it was
    assert (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats(), d.table.rows(), ctx.mem_info()[0]) == before
    got, _, _ = ctx.scan_speeds(d.table, pcm, off, first, WINDOW, STEP, THREE)
    _same(got, want, "after the refusals")


def test_capacity_reports_the_total_through_the_abi(S, ctx, db, recording):
    """SHZ_E_CAPACITY with *count = the total, known from the frame counts alone: nothing is extracted for it."""
    import ctypes as C
    from shazam_amd import _ffi
    d, _ = db
    _, pcm, off, first = _flatten(S, [recording, recording[:SR]])
    wo, cnt = np.zeros(3, np.uint64), C.c_uint64()
    s0 = ctx.extract_stats()
    free0 = ctx.mem_info()[0]
    rc = _ffi.lib().shz_scan_speeds(ctx.h, d.table.h, _ffi.ptr(pcm), off.ctypes.data_as(_ffi.u64p), 2, first.ctypes.data_as(_ffi.u32p),
                                    2, SR, 10.0, 5, WINDOW, STEP, 2, LADDER.ctypes.data_as(_ffi.u32p), len(LADDER), 0,
                                    wo.ctypes.data_as(_ffi.u64p), None, None, None, None, None, None, None, None, None, 20,
                                    C.byref(cnt), None, None, None, None)
    assert rc == _ffi.E_CAPACITY and cnt.value == 21 and wo.tolist() == [0, 20, 21]
    assert ctx.extract_stats() == s0 and ctx.mem_info()[0] == free0


# ---- memory -----------------------------------------------------------------------------------------------------------
def test_no_memory_growth(S, ctx, db, mixed_batch):
    d, _ = db
    _, pcm, off, first = _flatten(S, mixed_batch)
    free = []
    for i in range(20):
        ctx.scan_speeds(d.table, pcm, off, first, 40, 15, THREE, topn=3)
        free.append(ctx.mem_info()[0])
    assert free[19] == free[1], free
