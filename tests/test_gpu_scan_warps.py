"""GPU: shz_scan_warps -- the peaks of every recording extracted once, warped for every (tempo, pitch) pair of a list, the
warped hash lists cut into the recording's windows with the TIME factor and every (window, warp) matched -- gives, array for
array, what the host recipe gives: shz_peaks, the numpy twin of the warp (tests/warp_twin.py), the twin's cut and fold
(tests/scan_warp_twin.py) and Table.match.  On a recording assembled from three table songs rendered at (1.16, 1), (1.10, 0.97)
and (1, 0.97) between noise, rank 0 is the CPU oracle's vote, the scan returns the three segments with their pairs and the
plain scan finds none of them.  A diagonal list is shz_scan_speeds, the unit pair shz_scan_batch.  Batch shapes that can go
wrong, slicing, another hop, tempos that fold two frames into one, refusals, capacity, memory.  Per-window selections:
tests/test_gpu_scan_warps_select.py."""
import numpy as np
import pytest

import scan_warp_cases as SC
import scan_warp_twin as SW
import speed_twin as T
import warp_twin as WT

pytestmark = pytest.mark.gpu

ARRAYS = SC.ARRAYS
WINDOW, STEP, SR = SC.WINDOW, SC.STEP, SC.SR
FACTORS = (32768, 62259, 65536, 68813, 131072)
QUAD_T = np.repeat(np.asarray(FACTORS, np.uint32), 5)          # all four quadrants, the axes and the corners
QUAD_F = np.tile(np.asarray(FACTORS, np.uint32), 5)
FOUR_T = np.asarray([62259, 68813, 65536, 68813, 62259], np.uint32)   # one pair a quadrant and the unit pair, not sorted
FOUR_F = np.asarray([62259, 62259, 65536, 68813, 68813], np.uint32)


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def songs():
    return SC.songs()


@pytest.fixture(scope="module")
def recording():
    return SC.recording()


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    d, table = SC.make_db(S, ctx, songs)
    yield d, table
    d.close()


@pytest.fixture(scope="module")
def mixed_batch(songs, recording):
    from oracle import synth
    part = recording[SR:8 * SR]
    return [
        [part, synth.mix_query(part, synth.traffic_noise(6, 3, len(part)), 3.0)],     # stereo, the second channel noise-mixed
        [],                                                                          # no clips: no window
        songs[1][:3000],                                                             # shorter than one window: one window
        [songs[2][:5 * SR], songs[2][:3 * SR + 777]],                                # channels of unequal length
    ]


# ---- the recipe -------------------------------------------------------------------------------------------------------
def test_recipe_equals_match_over_all_quadrants(S, ctx, db, recording):
    d, _ = db
    assert ctx.frames_of(len(recording)) == 537
    got, win_off = SC.check(S, d, [recording[:9 * SR]], WINDOW, STEP, QUAD_T, QUAD_F, topns=(1, 2), full_sorts=(False, True),
                            what="recipe")
    assert win_off.tolist() == [0, 5] and got["profile"].shape == (5, 25)
    print("best:", got["best"].tolist(), "aligned:", got["aligned"][:, 0].tolist())
    assert got["nres"].any() and got["profile"].any(axis=0).sum() > 4


def test_fixture_rank0_is_the_oracle_and_the_three_segments(S, ctx, db, recording):
    from oracle import cpu_ref as O
    from shazam_amd import _ffi
    from shazam_amd.speed import warp_grid
    d, table = db
    t16, f16 = warp_grid(SC.TEMPOS, SC.PITCHES)
    _, pcm, off, first = SC.flatten(S, [recording])
    got, win_off, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, SC.FIX_STEP, t16, f16)
    assert win_off.tolist() == [0, 11]
    print("best:", got["best"].tolist())
    print("delta:", got["delta"][:, 0].tolist())
    print("aligned:", got["aligned"][:, 0].tolist())
    # rank 0 of every (window, warp) is the reference's vote on the oracle's peaks, warped and cut by the twins
    f, t = O.fingerprint_keys(recording)[2:]
    for v, (a, p) in enumerate(zip(t16.tolist(), f16.tolist())):
        cut = SW.cut_windows([WT.warp_pair_tf(f, t, a, p)], 11, WINDOW, SC.FIX_STEP, a)
        for w, (k, q) in enumerate(cut):
            ranked, dedup, nhash = T.aligned_votes(k, q, table, 1)
            assert int(got["profile"][w, v]) == (ranked[0][2] if ranked else 0), (w, v)
            if v == int(got["best"][w]):
                sid, delta, aligned = ranked[0]
                assert (int(got["sid"][w, 0]), int(got["delta"][w, 0]), int(got["aligned"][w, 0])) == (sid, delta, aligned), w
                assert int(got["nhash"][w]) == nhash and int(got["dedup"][w, 0]) == dedup[sid]
    # what was measured on the CPU (scan_warp_cases.py): the songs, their positions, the pairs, the counts
    assert got["best"].tolist() == SC.BEST and got["sid"][:, 0].tolist() == SC.SID
    assert got["delta"][:, 0].tolist() == SC.DELTA and got["aligned"][:, 0].tolist() == SC.ALIGNED
    assert min(SC.ALIGNED) > SC.MIN_ALIGNED > max(SC.PLAIN + SC.SPEED)
    # the three segments, each pair within one rung of what the renderer was told
    seg = _ffi.scan_timeline_warps(win_off, got["sid"], got["delta"], got["aligned"], got["nres"], got["best"], SC.FIX_STEP, t16, f16,
                                   SC.MIN_ALIGNED, 1, SC.TEMPO_RUNG, SC.PITCH_RUNG, 4)
    assert len(seg["rec"]) == 3
    for i, ((sid, first_w, last_w, pair), (_, tempo, pitch, _s)) in enumerate(zip(SC.SEGMENTS, SC.PIECES)):
        v = int(seg["warp"][i])
        assert (int(seg["sid"][i]), int(seg["first"][i]), int(seg["last"][i])) == (sid, first_w, last_w)
        assert (int(t16[v]), int(f16[v])) == pair
        assert abs(int(t16[v]) - T.q16(tempo)) <= SC.TEMPO_RUNG and abs(int(f16[v]) - T.q16(pitch)) <= SC.PITCH_RUNG
        assert int(seg["hits"][i]) == last_w - first_w + 1
        assert (int(seg["pos_first"][i]), int(seg["pos_last"][i])) == (SC.DELTA[first_w], SC.DELTA[last_w])
    # the plain scan and the default speed ladder stay below the threshold on every window: none of the segments
    from shazam_amd.speed import speed_ladder
    plain, wo, _ = ctx.scan_batch(d.table, pcm, off, first, WINDOW, SC.FIX_STEP)
    assert np.where(plain["nres"] > 0, plain["aligned"][:, 0], 0).tolist() == SC.PLAIN
    assert len(_ffi.scan_timeline(wo, plain["sid"], plain["delta"], plain["aligned"], plain["nres"], SC.FIX_STEP, SC.MIN_ALIGNED)["rec"]) == 0
    sp, _, _ = ctx.scan_speeds(d.table, pcm, off, first, WINDOW, SC.FIX_STEP, speed_ladder())
    assert sp["profile"].max(axis=1).tolist() == SC.SPEED


# ---- identities -------------------------------------------------------------------------------------------------------
def test_a_diagonal_list_is_the_speed_scan_and_the_unit_pair_the_plain_scan(S, ctx, db, recording, mixed_batch):
    d, _ = db
    ladder = np.asarray([63604, 32768, 65536, 67468, 65628], np.uint32)
    for recs, window, step in (([recording[:10 * SR]], WINDOW, STEP), (mixed_batch, 40, 15)):
        _, pcm, off, first = SC.flatten(S, recs)
        for topn in (1, 3):
            want, wo0, _ = ctx.scan_speeds(d.table, pcm, off, first, window, step, ladder, topn=topn)
            got, wo1, _ = ctx.scan_warps(d.table, pcm, off, first, window, step, ladder, ladder.copy(), topn=topn)
            assert np.array_equal(wo0, wo1) and len(want["nres"]) > 3
            SC.same(got, want, ("diagonal", topn))
            want, wo0, _ = ctx.scan_batch(d.table, pcm, off, first, window, step, topn=topn)
            one = np.asarray([65536], np.uint32)
            got, wo1, _ = ctx.scan_warps(d.table, pcm, off, first, window, step, one, one, topn=topn)
            assert np.array_equal(wo0, wo1)
            SC.same(got, want, ("unit pair", topn), ARRAYS)
            assert not got["best"].any()
            assert np.array_equal(got["profile"][:, 0], np.where(want["nres"] > 0, want["aligned"][:, 0], 0))


# ---- batch shapes that can go wrong -----------------------------------------------------------------------------------
def test_mixed_batch(S, db, mixed_batch):
    d, _ = db
    got, win_off = SC.check(S, d, mixed_batch, 40, 15, FOUR_T, FOUR_F, topns=(1, 3), what="mixed")
    counts = np.diff(win_off.astype(np.int64)).tolist()
    assert counts[0] > 3 and counts[1] == 0 and counts[2] == 1 and counts[3] > 1
    assert got["nres"][:counts[0]].any()


def test_recordings_without_clips_only(S, ctx, db):
    d, _ = db
    got, win_off, _ = ctx.scan_warps(d.table, np.zeros(1, np.int16), np.zeros(1, np.uint64), np.zeros(3, np.uint32), WINDOW, STEP,
                                     FOUR_T, FOUR_F)
    assert win_off.tolist() == [0, 0, 0] and got["best"].shape == (0,) and got["profile"].shape == (0, 5) and got["work"] == (0, 0)


def test_thirty_frames_window_one_and_step_above_window(S, ctx, db, songs):
    d, _ = db
    clip = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048]
    assert ctx.frames_of(len(clip)) == 30
    got, win_off = SC.check(S, d, [clip, clip[:20000]], 1, 4, FOUR_T, FOUR_F, what="window 1, step 4")
    assert win_off.tolist() == [0, 9, 12]
    assert np.any(got["nhash"] == 0) and np.any(got["nhash"] > 0)
    SC.check(S, d, [clip], 4, 9, FOUR_T, FOUR_F, what="step > window")


def test_step_that_puts_a_window_beyond_every_t1(S, ctx, db, songs):
    """Step 2^32 - 1: the second window starts above every t1' at every warp and is empty (test_gpu_scan.py has the reason)."""
    d, _ = db
    clip = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048]
    near, _ = SC.check(S, d, [clip], 4, 1, FOUR_T, FOUR_F, what="window 4 step 1")
    got, win_off = SC.check(S, d, [clip], 4, (1 << 32) - 1, FOUR_T, FOUR_F, what="step 2^32 - 1")
    assert win_off.tolist() == [0, 2]
    assert int(got["nhash"][1]) == 0 and int(got["nres"][1]) == 0 and not got["profile"][1].any()
    for name in ARRAYS + ("best", "profile"):
        assert np.array_equal(got[name][0], near[name][0]), name


def test_recordings_without_windows_front_middle_and_end(S, ctx, db, songs):
    from shazam_amd import _ffi
    d, _ = db
    a, b = songs[3][2 * SR:2 * SR + 4096 + 29 * 2048], songs[1][3 * SR:3 * SR + 4096 + 29 * 2048]
    recs = [[], a, [], [], [b, b[:20000]], []]
    for debug in (0, _ffi.DEBUG_SCAN_SPEED_SMALL_SLICES):
        ctx.set_debug(debug)
        try:
            got, win_off = SC.check(S, d, recs, 4, 9, FOUR_T, FOUR_F, what=("empty recordings", debug))
        finally:
            ctx.set_debug(0)
        assert win_off.tolist() == [0, 0, 4, 4, 4, 8, 8]
        assert got["nhash"][:4].any() and got["nhash"][4:].any()


def test_small_slices_and_device_pcm_give_the_same_arrays(S, ctx, db, recording, mixed_batch):
    from shazam_amd import _ffi
    d, _ = db
    for recs, window, step in (([recording[:12 * SR]], WINDOW, STEP), (mixed_batch, 40, 15), (mixed_batch, 3, 2)):
        _, pcm, off, first = SC.flatten(S, recs)
        buf = ctx.alloc(pcm.nbytes)
        buf.upload(pcm)
        try:
            for full_sort in (False, True):
                want, wo0, _ = ctx.scan_warps(d.table, pcm, off, first, window, step, FOUR_T, FOUR_F, topn=3, full_sort=full_sort)
                ctx.set_debug(_ffi.DEBUG_SCAN_SPEED_SMALL_SLICES)     # 1 recording x 2 warps a slice, 3 windows a match group
                try:
                    got, wo1, _ = ctx.scan_warps(d.table, buf, off, first, window, step, FOUR_T, FOUR_F, topn=3, full_sort=full_sort,
                                                 pcm_device=True)
                finally:
                    ctx.set_debug(0)
                assert len(want["nres"]) > 3 and np.array_equal(wo0, wo1)
                SC.same(got, want, ("small slices", window, step, full_sort))
                assert got["work"] == want["work"]
        finally:
            buf.free()


def test_hop_1024(S, ctx, db, recording):
    d, _ = db
    part = recording[3 * SR:8 * SR]
    ctx.set_overlap(4096 - 1024)
    try:
        assert ctx.frames_of(len(part)) == (len(part) - 4096) // 1024 + 1
        got, win_off = SC.check(S, d, [part, [part[:SR], part[SR:3 * SR]]], 50, 30, FOUR_T, FOUR_F, what="hop 1024")
        assert int(win_off[1]) == SW.window_count(ctx.frames_of(len(part)), 50, 30)
    finally:
        ctx.set_overlap(2048)


def test_tempos_that_fold_two_frames_into_one(S, ctx, db, recording):
    """At tempo 32768 frames 2 k - 1 and 2 k share one t', whatever the pitch: a window that starts at an even frame starts in
    the middle of such a pair, and the peaks of the frame in front of it belong to it."""
    d, _ = db
    part = recording[5 * SR:12 * SR]
    t16, f16 = np.asarray([32768, 32768, 40000, 32768], np.uint32), np.asarray([65536, 131072, 62259, 32768], np.uint32)
    _, pcm, off, _ = SC.flatten(S, [part])
    _, pt, _ = ctx.peaks(pcm, off)
    shared = [w for w in range(1, 8) if SW.W(w * 15 - 1, 32768) == SW.W(w * 15, 32768) and np.any(pt == w * 15 - 1) and np.any(pt == w * 15)]
    assert shared, "a window start whose frame shares its t' with the frame in front of it, peaks in both"
    got, _ = SC.check(S, d, [part], 40, 15, t16, f16, topns=(1, 2), what="folding tempos")
    assert got["nhash"].any() and got["nres"].any()
    SC.check(S, d, [[part, part[SR:]]], 7, 2, t16, f16, what="folding tempos, short windows, stereo")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(S, ctx, db, recording, songs):
    from shazam_amd import _ffi
    d, _ = db
    recs = [recording[:6 * SR], [songs[0][:3 * SR], songs[1][:3 * SR]]]
    _, pcm, off, first = SC.flatten(S, recs)
    u32 = lambda *xs: np.asarray(xs, np.uint32)   # noqa: E731
    # the longest window still taken, from t16 alone: 2^20 - 2 warped frames; the pitch may be 2 at any window
    ctx.scan_warps(d.table, pcm, off, first, (1 << 19) - 1, STEP, u32(131072), u32(131072))
    ctx.scan_warps(d.table, pcm, off, first, (1 << 20) - 1, STEP, u32(65536), u32(131072))
    want, wo, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, FOUR_T, FOUR_F)
    total = int(wo[-1])
    before = (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats(), d.table.rows(), ctx.mem_info()[0])
    ok = dict(window_frames=WINDOW, step_frames=STEP, tempos=FOUR_T, pitches=FOUR_F)
    two = lambda a, b: dict(ok, tempos=a, pitches=b)   # noqa: E731
    for what, rc0, kw, code, says in (
            ("empty list", first, two(u32(), u32()), _ffi.E_INVALID, "n_warps"),
            ("1025 warps", first, two(np.full(1025, 65536, np.uint32), np.full(1025, 65536, np.uint32)), _ffi.E_INVALID, "n_warps"),
            ("tempo below 0.5", first, two(u32(65536, 32767), u32(65536, 65536)), _ffi.E_INVALID, "tempo 1"),
            ("tempo above 2", first, two(u32(131073, 65536), u32(65536, 65536)), _ffi.E_INVALID, "tempo 0"),
            ("pitch below 0.5", first, two(u32(65536, 65536), u32(65536, 32767)), _ffi.E_INVALID, "pitch 1"),
            ("pitch above 2", first, two(u32(65536, 65536), u32(131073, 65536)), _ffi.E_INVALID, "pitch 0"),
            ("window 0", first, dict(ok, window_frames=0), _ffi.E_INVALID, ""),
            ("window 2^20", first, dict(ok, window_frames=1 << 20), _ffi.E_INVALID, ""),
            ("step 0", first, dict(ok, step_frames=0), _ffi.E_INVALID, ""),
            ("topn 0", first, dict(ok, topn=0), _ffi.E_INVALID, ""),
            ("rec_clip0 not ascending", u32(0, 2, 1, 3), ok, _ffi.E_INVALID, ""),
            ("warped window of 2^20", first, dict(two(u32(65536, 131072), u32(32768, 32768)), window_frames=1 << 19), _ffi.E_UNSUPPORTED, ""),
            ("warped window above 2^20", first, dict(two(u32(65537), u32(65536)), window_frames=(1 << 20) - 1), _ffi.E_UNSUPPORTED, ""),
            ("room for one window less", first, dict(ok, cap_windows=total - 1), _ffi.E_CAPACITY, f"{total} windows"),
            ("no room", first, dict(ok, cap_windows=0), _ffi.E_CAPACITY, f"{total} windows")):
        kw = dict(kw)
        args = (kw.pop("window_frames"), kw.pop("step_frames"), kw.pop("tempos"), kw.pop("pitches"))
        with pytest.raises(_ffi.ShzError) as e:
            ctx.scan_warps(d.table, pcm, off, rc0, *args, **kw)
        assert e.value.code == code, what
        assert says in str(e.value), (what, str(e.value))
    # nothing ran: no extraction, no match, no allocation, the table as it was
    assert (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats(), d.table.rows(), ctx.mem_info()[0]) == before
    got, _, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, FOUR_T, FOUR_F)
    SC.same(got, want, "after the refusals")


def test_capacity_reports_the_total_through_the_abi(S, ctx, db, recording):
    """SHZ_E_CAPACITY with *count = the total, known from the frame counts alone: nothing is extracted for it."""
    import ctypes as C
    from shazam_amd import _ffi
    d, _ = db
    _, pcm, off, first = SC.flatten(S, [recording, recording[:SR]])
    wo, cnt, work = np.zeros(3, np.uint64), C.c_uint64(), np.ones(2, np.uint64)
    s0 = ctx.extract_stats()
    free0 = ctx.mem_info()[0]
    rc = _ffi.lib().shz_scan_warps(ctx.h, d.table.h, _ffi.ptr(pcm), off.ctypes.data_as(_ffi.u64p), 2, first.ctypes.data_as(_ffi.u32p),
                                   2, SR, 10.0, 5, WINDOW, STEP, 2, FOUR_T.ctypes.data_as(_ffi.u32p), FOUR_F.ctypes.data_as(_ffi.u32p),
                                   len(FOUR_T), None, None, 0, wo.ctypes.data_as(_ffi.u64p), None, None, None, None, None, None, None,
                                   None, None, work.ctypes.data_as(_ffi.u64p), 21, C.byref(cnt), None, None, None, None)
    assert rc == _ffi.E_CAPACITY and cnt.value == 22 and wo.tolist() == [0, 21, 22] and work.tolist() == [0, 0]
    assert ctx.extract_stats() == s0 and ctx.mem_info()[0] == free0


# ---- memory -----------------------------------------------------------------------------------------------------------
def test_no_memory_growth(S, ctx, db, mixed_batch):
    d, _ = db
    _, pcm, off, first = SC.flatten(S, mixed_batch)
    free = []
    for i in range(20):
        ctx.scan_warps(d.table, pcm, off, first, 40, 15, FOUR_T, FOUR_F, topn=3)
        free.append(ctx.mem_info()[0])
    assert free[19] == free[1], free
