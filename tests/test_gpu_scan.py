"""GPU: shz_scan_batch -- every recording fingerprinted once, its device-resident hash list cut into overlapping time
windows, all windows matched in one call -- gives, array for array, what shz_match_batch gives on windows built on the
host from shz_fingerprint_batch's output; on a recording assembled from two table songs between noise, rank 0 is the CPU
oracle's vote and scan() returns the two segments; batch shapes that can go wrong, grouping, refusals, memory."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
WINDOW, STEP = 108, 22            # round(5 s * 44100 / 2048), round(1 s * 44100 / 2048)
SR = 44100


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
    from oracle import synth
    return np.concatenate([synth.traffic_noise(5, 0, 3 * SR), songs[1][SR:7 * SR], songs[3][0:5 * SR],
                           synth.traffic_noise(5, 1, 2 * SR)])


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    """Songs 1..4, their hashes straight from the extraction (the table of the recipe)."""
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
def oracle_recipe(songs, recording):
    """The CPU oracle's table and the recording's hashes, computed once."""
    from oracle import cpu_ref as O
    odb = O.DictDB()
    for c, x in enumerate(songs):
        k, t1, _, _ = O.fingerprint_keys(x)
        sid = odb.insert_song(f"song{c}", "AB" * 20, len(k))
        odb.insert_hashes(sid, zip(k.tolist(), t1.tolist()))
    k, t1, _, _ = O.fingerprint_keys(recording)
    return odb, k, t1


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


def _window_count(frames, window, step):
    return 0 if frames == 0 else 1 if frames <= window else -(-(frames - window) // step) + 1


def _host_windows(ctx, chans, first, k, t1, ho, window, step):
    """The contract, on the host: per recording and window the (key32, t1 - s) of the hashes with s <= t1 < s + window over all
    channels -> (key32, q_off, query_off, win_off)."""
    keys, qoffs, query_off, win_off = [], [], [0], [0]
    t1 = t1.astype(np.int64)
    for r in range(len(first) - 1):
        cs = range(int(first[r]), int(first[r + 1]))
        frames = max((ctx.frames_of(len(chans[c])) for c in cs), default=0)
        for w in range(_window_count(frames, window, step)):
            s, n = w * step, 0
            for c in cs:
                a, b = int(ho[c]), int(ho[c + 1])
                m = (t1[a:b] >= s) & (t1[a:b] < s + window)
                keys.append(k[a:b][m])
                qoffs.append((t1[a:b][m] - s).astype(np.uint32))
                n += int(m.sum())
            query_off.append(query_off[-1] + n)
        win_off.append(len(query_off) - 1)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint32)   # noqa: E731
    return cat(keys).astype(np.uint32), cat(qoffs).astype(np.uint32), np.asarray(query_off, np.uint64), np.asarray(win_off, np.uint64)


def _same_arrays(a, b, what=""):
    for name in ARRAYS:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (what, name, a[name].shape, b[name].shape)
        assert np.array_equal(a[name], b[name]), (what, name)


def _check(S, db, recordings, window, step, topns=(2,), full_sorts=(False,), what=""):
    """scan_batch against Table.match on host-built windows; returns the last result and win_off."""
    ctx = db.ctx
    chans, pcm, off, first = _flatten(S, recordings)
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    hk, hq, hqo, hwo = _host_windows(ctx, chans, first, k, t1, ho, window, step)
    for topn in topns:
        for fs_ in full_sorts:
            want = db.table.match(hk, hq, hqo, topn, full_sort=fs_)
            got, win_off, ms = ctx.scan_batch(db.table, pcm, off, first, window, step, topn=topn, full_sort=fs_)
            assert np.array_equal(win_off, hwo), (what, win_off, hwo)
            _same_arrays(got, want, (what, topn, fs_))
            assert all(m >= 0.0 for m in ms)
    return got, win_off


# ---- the recipe -------------------------------------------------------------------------------------------------------
def test_recipe_equals_match_and_oracle(S, ctx, db, recording, oracle_recipe):
    from oracle import cpu_ref as O
    assert ctx.frames_of(len(recording)) == 343
    k, t1, ho = S.fingerprint_batch([recording], ctx=ctx)
    odb, ok, ot1 = oracle_recipe
    assert int(ho[-1]) == 4802 and np.array_equal(k, ok) and np.array_equal(t1, ot1)
    assert np.all(np.diff(t1.astype(np.int64)) >= 0), "t1 never decreases inside a clip: what the windows rest on"
    got, win_off = _check(S, db, [recording], WINDOW, STEP, topns=(1, 2, 10), full_sorts=(False, True), what="recipe")
    assert win_off.tolist() == [0, 12]
    # rank 0 of every window is the oracle's vote on the window's hash set
    weakest = None
    for w in range(12):
        s = w * STEP
        m = (ot1 >= s) & (ot1 < s + WINDOW)
        hs = set(zip(ok[m].tolist(), (ot1[m].astype(np.int64) - s).tolist()))
        matches, dedup = O.return_matches(hs, odb)
        sid, delta, aligned = O.vote(matches, 1)[0]
        assert (int(got["sid"][w, 0]), int(got["delta"][w, 0]), int(got["aligned"][w, 0])) == (sid, delta, aligned), w
        assert int(got["nhash"][w]) == len(hs) and int(got["npairs"][w]) == len(matches) and int(got["dedup"][w, 0]) == dedup[sid]
        assert (sid, delta - s) == ((2, -43) if w < 8 else (4, -194)), w
        weakest = aligned if weakest is None else min(weakest, aligned)
    assert weakest == 182


def test_scan_returns_the_two_segments(S, db, recording):
    hop = 2048
    segs = S.scan([recording], db, min_aligned=50)
    assert len(segs) == 1
    a, b = segs[0]
    assert (a["song_id"], a["shift"], a["windows"]) == (2, -43, 8) and (b["song_id"], b["shift"], b["windows"]) == (4, -194, 4)
    assert a["song_name"] == b"song1" and b["song_name"] == b"song3"
    # windows 0..7 and 8..11: starts at w * step, the end of window 11 (242 + 108 = 350) clipped to the 343 frames
    assert a["start_seconds"] == 0.0 and a["end_seconds"] == round((7 * STEP + WINDOW) * hop / SR, 5)
    assert b["start_seconds"] == round(8 * STEP * hop / SR, 5) and b["end_seconds"] == round(343 * hop / SR, 5)
    # the song position at the segment's start: song 2 is 43 frames in front of the recording's start (it begins after 3 s of
    # noise, one second into the song: (3 - 1) s = 43 frames), song 4 starts 18 frames behind window 8
    assert a["offset_seconds"] == round(-43 / SR * hop, 5) and b["offset_seconds"] == round((-194 + 8 * STEP) / SR * hop, 5)
    assert a["hashes_aligned"] >= 182 and b["hashes_aligned"] >= 182
    # the raw arrays come with the geometry
    w = S.scan_windows([recording], db, topn=3)
    assert (w["window_frames"], w["step_frames"], w["hop"], w["fs"]) == (WINDOW, STEP, hop, SR)
    assert w["frames"].tolist() == [343] and w["win_off"].tolist() == [0, 12] and w["sid"].shape == (12, 3)
    # a threshold above every count: no segment; no recording: no list
    assert S.scan([recording], db, min_aligned=10 ** 6) == [[]]
    assert S.scan([], db) == []


# ---- batch shapes that can go wrong -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch(songs, recording):
    from oracle import synth
    part = recording[2 * SR:9 * SR]
    return [
        [part, synth.mix_query(part, synth.traffic_noise(6, 3, len(part)), 3.0)],     # stereo, the channels differ
        songs[0][SR:6 * SR],                                                         # mono
        [songs[2][:5 * SR], songs[2][:3 * SR + 777]],                                # channels of unequal length
        songs[1][:3000],                                                             # one zero-padded frame: one window
        np.zeros(4 * SR, np.int16),                                                  # silence: nhash = nres = 0
        [],                                                                          # no clips: no window
        recording[6 * SR:12 * SR + 1234],
    ]


def test_mixed_batch(S, ctx, db, mixed_batch):
    got, win_off = _check(S, db, mixed_batch, 40, 15, topns=(1, 3), what="mixed")
    counts = np.diff(win_off.astype(np.int64)).tolist()
    assert counts[3] == 1 and counts[5] == 0 and counts[0] > 3 and counts[2] > 1
    sil = slice(int(win_off[4]), int(win_off[5]))
    assert counts[4] > 1 and not got["nhash"][sil].any() and not got["nres"][sil].any()
    assert int(got["nres"][0]) > 0 and int(got["nres"][int(win_off[6])]) > 0
    # the stereo recording's windows are unions: more distinct hashes than the first channel alone gives
    mono, _ = _check(S, db, [mixed_batch[0][0]], 40, 15, what="first channel")
    assert np.all(got["nhash"][:counts[0]] >= mono["nhash"]) and np.any(got["nhash"][:counts[0]] > mono["nhash"])


def test_recordings_without_clips_only(S, ctx, db):
    got, win_off, _ = ctx.scan_batch(db.table, np.zeros(1, np.int16), np.zeros(1, np.uint64), np.zeros(3, np.uint32), WINDOW, STEP)
    assert win_off.tolist() == [0, 0, 0] and got["nres"].shape == (0,) and got["sid"].shape == (0, 2)
    got, win_off, _ = ctx.scan_batch(db.table, np.zeros(1, np.int16), np.zeros(1, np.uint64), np.zeros(1, np.uint32), WINDOW, STEP)
    assert win_off.tolist() == [0] and got["nres"].shape == (0,)


def test_thirty_frames_window_one_and_step_above_window(S, ctx, db, songs):
    clip = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048]
    assert ctx.frames_of(len(clip)) == 30
    got, win_off = _check(S, db, [clip], 1, 1, what="window 1 step 1")
    assert win_off.tolist() == [0, 30]
    assert np.any(got["nhash"] == 0) and np.any(got["nhash"] > 0), "windows of one frame: many are empty, some are not"
    got, win_off = _check(S, db, [clip, clip[:20000]], 4, 9, what="step > window")
    assert win_off.tolist() == [0, 4, 6]
    _check(S, db, [clip], 7, 7, what="step = window")
    _check(S, db, [clip], 29, 1, what="two windows")


def test_step_that_puts_a_window_beyond_every_t1(S, ctx, db, songs):
    """Step 2^32 - 1: the second window starts above every t1.  Its start is not clamped to 32 bits anywhere; the device's
    searches compare in 64 bits, so it is empty, and the first window is what it is at any step."""
    clip = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048]
    near, _ = _check(S, db, [clip], 4, 1, what="window 4 step 1")
    got, win_off = _check(S, db, [clip], 4, (1 << 32) - 1, what="step 2^32 - 1")
    assert win_off.tolist() == [0, 2]
    assert int(got["nhash"][1]) == 0 and int(got["nres"][1]) == 0
    assert int(got["nhash"][0]) > 0
    for name in ARRAYS:
        assert np.array_equal(got[name][0], near[name][0]), name


def test_recordings_without_windows_front_middle_and_end(S, ctx, db, songs):
    """Recordings without windows share their start with the next one in the stage's descriptors: the search for "the last
    recording whose first item is <= i" must step over them, one or two at a time, in front, in the middle and at the end."""
    from shazam_amd import _ffi
    a, b = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048], songs[1][3 * SR:3 * SR + 4096 + 29 * 2048]
    recs = [[], a, [], [], [b, b[:20000]], []]
    for debug in (0, _ffi.DEBUG_SCAN_SMALL_GROUPS):
        ctx.set_debug(debug)
        try:
            got, win_off = _check(S, db, recs, 4, 9, what=("empty recordings", debug))
        finally:
            ctx.set_debug(0)
        assert win_off.tolist() == [0, 0, 4, 4, 4, 8, 8]
        assert got["nhash"][:4].any() and got["nhash"][4:].any()


def test_window_of_the_whole_recording_is_the_fused_call(S, ctx, db, mixed_batch):
    chans, pcm, off, first = _flatten(S, mixed_batch)
    frames = max(ctx.frames_of(len(c)) for c in chans)
    for window in (frames, frames + 1, (1 << 20) - 1):
        for topn in (1, 3):
            got, win_off, _ = ctx.scan_batch(db.table, pcm, off, first, window, STEP, topn=topn)
            # (a recording without clips is a query without hashes there and no window here)
            keep = [q for q in range(len(first) - 1) if first[q + 1] > first[q]]
            want, _, _ = ctx.recognize_batch(db.table, pcm, off, first, topn=topn)
            assert np.diff(win_off.astype(np.int64)).tolist() == [1 if q in keep else 0 for q in range(len(first) - 1)]
            _same_arrays(got, {k: v[keep] for k, v in want.items()}, ("whole recording", window, topn))


def test_hop_1024(S, ctx, db, recording):
    """Another hop (shz_set_overlap): twice the frames, the windows cut at that hop.  The table's offsets are at hop 2048, so
    the answers mean little; the arrays are those of the match on host-built windows all the same."""
    part = recording[3 * SR:8 * SR]
    ctx.set_overlap(4096 - 1024)
    try:
        assert ctx.frames_of(len(part)) == (len(part) - 4096) // 1024 + 1
        chans, pcm, off, first = _flatten(S, [part, [part[:SR], part[SR:3 * SR]]])
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, off)
        hk, hq, hqo, hwo = _host_windows(ctx, chans, first, k, t1, ho, 50, 30)
        want = db.table.match(hk, hq, hqo, 2)
        got, win_off, _ = ctx.scan_batch(db.table, pcm, off, first, 50, 30)
        assert np.array_equal(win_off, hwo) and int(win_off[1]) == _window_count(ctx.frames_of(len(part)), 50, 30)
        _same_arrays(got, want, "hop 1024")
    finally:
        ctx.set_overlap(2048)


def test_device_pcm_gives_the_same_arrays(S, ctx, db, mixed_batch):
    _, host, off, first = _flatten(S, mixed_batch)
    want, wo0, _ = ctx.scan_batch(db.table, host, off, first, 40, 15, topn=3)
    buf = ctx.alloc(host.nbytes)
    buf.upload(host)
    got, wo1, _ = ctx.scan_batch(db.table, buf, off, first, 40, 15, topn=3, pcm_device=True)
    buf.free()
    assert np.array_equal(wo0, wo1)
    _same_arrays(got, want, "device PCM")


# ---- grouping ---------------------------------------------------------------------------------------------------------
def test_small_groups_give_the_same_arrays(S, ctx, db, recording, mixed_batch):
    from shazam_amd import _ffi
    for recs, window, step in (([recording], WINDOW, STEP), (mixed_batch, 40, 15), (mixed_batch, 3, 1)):
        _, pcm, off, first = _flatten(S, recs)
        for full_sort in (False, True):
            want, wo0, _ = ctx.scan_batch(db.table, pcm, off, first, window, step, topn=3, full_sort=full_sort)
            ctx.set_debug(_ffi.DEBUG_SCAN_SMALL_GROUPS)
            try:
                got, wo1, _ = ctx.scan_batch(db.table, pcm, off, first, window, step, topn=3, full_sort=full_sort)
            finally:
                ctx.set_debug(0)
            assert len(want["nres"]) > 3 and np.array_equal(wo0, wo1)
            _same_arrays(got, want, ("groups of 3", window, step, full_sort))


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(S, ctx, db, recording, songs):
    from shazam_amd import _ffi
    recs = [recording[:6 * SR], [songs[0][:3 * SR], songs[1][:3 * SR]]]
    _, pcm, off, first = _flatten(S, recs)
    want, wo, _ = ctx.scan_batch(db.table, pcm, off, first, WINDOW, STEP)
    total = int(wo[-1])
    before = (ctx.spec_stats(), ctx.extract_stats(), db.table.match_stats(), db.table.rows(), ctx.mem_info()[0])
    ok = dict(window_frames=WINDOW, step_frames=STEP)
    for what, rc0, kw, code in (
            ("rec_clip0 not ascending", np.array([0, 2, 1, 3], np.uint32), ok, _ffi.E_INVALID),
            ("rec_clip0 ends early", np.array([0, 1, 2], np.uint32), ok, _ffi.E_INVALID),
            ("rec_clip0 starts late", np.array([1, 1, 3], np.uint32), ok, _ffi.E_INVALID),
            ("window 0", first, dict(ok, window_frames=0), _ffi.E_INVALID),
            ("window 2^20", first, dict(ok, window_frames=1 << 20), _ffi.E_INVALID),
            ("step 0", first, dict(ok, step_frames=0), _ffi.E_INVALID),
            ("topn 0", first, dict(ok, topn=0), _ffi.E_INVALID),
            ("topn 65", first, dict(ok, topn=65), _ffi.E_INVALID),
            ("room for one window less", first, dict(ok, cap_windows=total - 1), _ffi.E_CAPACITY),
            ("no room", first, dict(ok, cap_windows=0), _ffi.E_CAPACITY)):
        with pytest.raises(_ffi.ShzError) as e:
            ctx.scan_batch(db.table, pcm, off, rc0, **kw)
        assert e.value.code == code, what
        if code == _ffi.E_CAPACITY:
            assert f"{total} windows" in str(e.value), "the message names the total"
    # nothing ran: no extraction, no match, no allocation, the table as it was
    assert (ctx.spec_stats(), ctx.extract_stats(), db.table.match_stats(), db.table.rows(), ctx.mem_info()[0]) == before
    t = S.Table(ctx)                                               # a table that was never finalized
    with pytest.raises(_ffi.ShzError) as e:
        ctx.scan_batch(t, pcm, off, first, WINDOW, STEP)
    assert e.value.code == _ffi.E_STATE
    t.close()
    assert (ctx.spec_stats(), ctx.extract_stats(), db.table.match_stats(), db.table.rows()) == before[:4]
    got, _, _ = ctx.scan_batch(db.table, pcm, off, first, WINDOW, STEP)
    _same_arrays(got, want, "after the refusals")


def test_capacity_reports_the_total_through_the_abi(S, ctx, db, recording):
    """SHZ_E_CAPACITY with *count = the total, known from the frame counts alone: nothing is extracted for it."""
    import ctypes as C
    from shazam_amd import _ffi
    _, pcm, off, first = _flatten(S, [recording, recording[:SR]])
    wo, cnt = np.zeros(3, np.uint64), C.c_uint64()
    s0 = ctx.extract_stats()
    free0 = ctx.mem_info()[0]
    rc = _ffi.lib().shz_scan_batch(ctx.h, db.table.h, _ffi.ptr(pcm), off.ctypes.data_as(_ffi.u64p), 2, first.ctypes.data_as(_ffi.u32p),
                                   2, SR, 10.0, 5, WINDOW, STEP, 2, 0, wo.ctypes.data_as(_ffi.u64p), None, None, None, None, None,
                                   None, None, 12, C.byref(cnt), None, None, None)
    assert rc == _ffi.E_CAPACITY and cnt.value == 13 and wo.tolist() == [0, 12, 13]
    assert ctx.extract_stats() == s0 and ctx.mem_info()[0] == free0


# ---- memory -----------------------------------------------------------------------------------------------------------
def test_no_memory_growth(S, ctx, db, mixed_batch):
    _, pcm, off, first = _flatten(S, mixed_batch)
    free = []
    for i in range(5):
        ctx.scan_batch(db.table, pcm, off, first, 40, 15, topn=3)
        free.append(ctx.mem_info()[0])
    assert free[4] == free[1], free
