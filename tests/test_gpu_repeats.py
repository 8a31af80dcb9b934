"""GPU: repeated content inside recordings (shz_repeats_hashes / shz_repeats_batch / find_repeats) against the plain-Python
definition in tests/repeat_twin.py, array for array: built hash lists at every edge of the definition, a run laid across every
block border, fuzz, capacity, refusals, the fused call against the host-column form, and planted audio.  Every comparison runs
with debug 0 and with SHZ_DEBUG_REPEAT_SMALL_SLICES (one recording a slice, tiles of 64 pairs, blocks of 64 elements)."""
import ctypes as C
import math

import numpy as np
import pytest

import repeat_twin as twin

pytestmark = pytest.mark.gpu

SR, HOP = 44100, 2048
FILL = 0x5A5A5A5A
CELL_KEYS = ("cell_off", "lag", "block", "pairs", "first", "last", "rec_hashes", "rec_pairs", "rec_skipped_keys", "rec_skipped_rows")
T_MAX = (1 << 20) - 1


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _same(got, want, what=""):
    for k in CELL_KEYS:
        assert [int(x) for x in got[k]] == [int(x) for x in want[k]], (k, what)


def _check(S, ctx, key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run=64, cell_shift=5, min_cell_pairs=1):
    """repeats_hashes == the twin, under both slicings; returns the twin's result"""
    want = twin.cells(key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run, cell_shift, min_cell_pairs)
    for debug in (0, S._ffi.DEBUG_REPEAT_SMALL_SLICES):
        ctx.set_debug(debug)
        try:
            got = ctx.repeats_hashes(key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run, cell_shift, min_cell_pairs)
        finally:
            ctx.set_debug(0)
        _same(got, want, f"debug {debug}")
    return want


def _one(S, ctx, hashes, **kw):
    """one mono recording from a list of (key, t)"""
    k, t = [h[0] for h in hashes], [h[1] for h in hashes]
    return _check(S, ctx, k, t, [0, len(k)], [0, 1], **kw)


# ---- built lists ----------------------------------------------------------------------------------------------------------
def test_run_of_exactly_max_run_and_one_more(S, ctx):
    for max_run in (2, 5, 1024):
        full = [(7, 3 * i) for i in range(max_run)]
        over = [(9, 2 * i) for i in range(max_run + 1)]
        want = _one(S, ctx, full + over + [(8, 1)], min_lag=1, max_lag=T_MAX, max_run=max_run, min_cell_pairs=1)
        assert want["rec_pairs"] == [max_run * (max_run - 1) // 2]
        assert (want["rec_skipped_keys"], want["rec_skipped_rows"]) == ([1], [max_run + 1])


def test_lags_at_the_bounds(S, ctx):
    hashes = [(1, 100), (1, 100 + 9), (2, 100), (2, 100 + 10), (3, 100), (3, 100 + 40), (4, 100), (4, 100 + 41)]
    want = _one(S, ctx, hashes, min_lag=10, max_lag=40)
    assert want["lag"] == [10, 40] and want["rec_pairs"] == [2]
    want = _one(S, ctx, hashes, min_lag=10, max_lag=10)
    assert want["lag"] == [10]
    # inside one run: the partners are a range in the middle of it, for every element
    run = [(5, t) for t in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89)]
    for lo, hi in ((0, 0), (0, T_MAX), (1, 1), (2, 8), (3, 34), (50, 60), (90, 100)):
        _one(S, ctx, run, min_lag=lo, max_lag=hi)


def test_times_at_the_block_border(S, ctx):
    for shift in (0, 1, 5, 19):
        edge = 1 << shift
        hashes = [(1, edge - 1), (1, edge - 1 + 50), (2, edge), (2, edge + 50), (3, 0), (3, 50)]
        want = _one(S, ctx, hashes, min_lag=1, max_lag=100, cell_shift=shift)
        assert want["rec_pairs"] == [3] and sum(want["pairs"]) == 3
        assert set(want["block"]) == ({0, 1} if shift else {0, edge - 1, edge})


def test_no_pair_crosses_recordings_and_channels_collapse(S, ctx):
    # the same key in two adjacent recordings; the same (key, t) in both channels of the stereo recording in the middle
    k = [1, 1, 2,   1, 1, 3,  1, 3, 1,   1, 2]
    t = [10, 40, 5, 10, 40, 7, 40, 7, 90, 70, 35]
    ho = [0, 3, 6, 9, 11]
    want = _check(S, ctx, k, t, ho, [0, 1, 3, 4], min_lag=1, max_lag=1000)
    assert want["rec_hashes"] == [3, 4, 2] and want["rec_pairs"] == [1, 3, 0]
    # ... and the three as one recording: now they do pair
    want = _check(S, ctx, k, t, ho, [0, 4], min_lag=1, max_lag=1000)
    assert want["rec_hashes"] == [7]


def test_empty_recordings_and_single_hashes(S, ctx):
    # no clips | clips without hashes | one hash | a pair | no clips at the end
    k, t = [5, 6, 6], [9, 1, 31]
    want = _check(S, ctx, k, t, [0, 0, 0, 1, 3], [0, 0, 2, 3, 4, 4], min_lag=1, max_lag=100)
    assert want["cell_off"] == [0, 0, 0, 0, 1, 1] and want["rec_hashes"] == [0, 0, 1, 2, 0]
    # nothing at all: recordings without a hash, and no recording
    want = _check(S, ctx, [], [], [0, 0], [0, 0, 1], min_lag=1, max_lag=100)
    assert want["cell_off"] == [0, 0, 0]
    want = _check(S, ctx, [], [], [0], [0], min_lag=1, max_lag=100)
    assert want["cell_off"] == [0]


def test_last_run_ends_at_the_arrays_end_and_the_largest_time(S, ctx):
    hashes = [(1, 5), (0xFFFFFFFF, T_MAX - 300), (0xFFFFFFFF, T_MAX - 1), (0xFFFFFFFF, T_MAX), (0, 0), (0, T_MAX)]
    want = _one(S, ctx, hashes, min_lag=1, max_lag=T_MAX)
    assert want["lag"] == [1, 299, 300, T_MAX]
    assert want["last"][-1] == 0 and want["first"][1] == T_MAX - 300


def test_min_cell_pairs_drops_cells(S, ctx):
    hashes = [(k, t) for k in range(6) for t in (4 + k, 104 + k)] + [(k, t) for k in range(10, 13) for t in (40 + k, 140 + k)] \
        + [(20, 70), (20, 170)]
    want = _one(S, ctx, hashes, min_lag=1, max_lag=500, min_cell_pairs=1)
    assert want["pairs"] == [6, 3, 1] and want["first"] == [4, 50, 70] and want["last"] == [9, 52, 70]
    want = _one(S, ctx, hashes, min_lag=1, max_lag=500, min_cell_pairs=3)
    assert want["pairs"] == [6, 3]
    want = _one(S, ctx, hashes, min_lag=1, max_lag=500, min_cell_pairs=4)
    assert want["pairs"] == [6] and want["rec_pairs"] == [10]
    want = _one(S, ctx, hashes, min_lag=1, max_lag=500, min_cell_pairs=7)
    assert want["pairs"] == [] and want["cell_off"] == [0, 0]


def test_run_across_every_block_border(S, ctx):
    """300 entries of one key at consecutive times behind 0 .. 70 entries of smaller keys: the run, its partners' ranges and
    its pairs' tiles straddle every 64- and 256-element border in turn"""
    for filler in range(71):
        hashes = [(k, 11) for k in range(filler)] + [(1000, 50 + i) for i in range(300)]
        want = _one(S, ctx, hashes, min_lag=280, max_lag=290, max_run=512, cell_shift=3)
        assert want["rec_pairs"] == [sum(300 - lag for lag in range(280, 291))]
    hashes = [(k, 11) for k in range(33)] + [(1000, 50 + i) for i in range(300)]
    want = _one(S, ctx, hashes, min_lag=1, max_lag=T_MAX, max_run=512, cell_shift=4)
    assert want["rec_pairs"] == [300 * 299 // 2]


def test_fuzz(S, ctx):
    rng = np.random.default_rng(2026)
    for case in range(40):
        n_recs = int(rng.integers(1, 6))
        k, t, ho, rc0 = [], [], [0], [0]
        for _ in range(n_recs):
            for _ in range(int(rng.integers(1, 3))):
                n = int(rng.integers(0, 3001) // (n_recs * 2)) if case % 3 else int(rng.integers(0, 40))
                keys = rng.integers(0, 40, n) if case % 2 else rng.integers(0, 1 << 32, n, dtype=np.uint64)
                k.extend(int(x) for x in keys)
                t.extend(int(x) for x in rng.integers(0, 600, n))
                ho.append(len(k))
            rc0.append(len(ho) - 1)
        lo = int(rng.integers(0, 50))
        _check(S, ctx, k, t, ho, rc0, min_lag=lo, max_lag=lo + int(rng.integers(0, 600)), max_run=int(rng.integers(2, 80)),
               cell_shift=int(rng.integers(0, 8)), min_cell_pairs=int(rng.integers(1, 6)))


def test_slices_of_several_recordings(S, ctx):
    """the workspace limit cuts the recordings into slices of more than one; a recording that alone exceeds a slice is refused"""
    rng = np.random.default_rng(7)
    k, t, ho = [], [], [0]
    for r in range(9):
        n = 30 + 25 * (r % 3)
        k.extend(int(x) for x in rng.integers(0, 6, n))
        t.extend(int(x) for x in rng.integers(0, 300, n))
        ho.append(len(k))
    rc0 = list(range(10))
    want = twin.cells(k, t, ho, rc0, 1, 400, 64, 4, 1)
    assert 250 < max(want["rec_pairs"]) <= 600 and sum(want["rec_pairs"]) > 1500
    try:
        ctx.set_workspace_limit(128 * 600)             # 600 pairs a slice: two or three recordings
        _same(ctx.repeats_hashes(k, t, ho, rc0, 1, 400, 64, 4, 1), want)
        ctx.set_workspace_limit(128 * 250)
        with pytest.raises(S.ShzError, match=r"recording \d+ has \d+ pairs.*min_lag.*max_run") as e:
            ctx.repeats_hashes(k, t, ho, rc0, 1, 400, 64, 4, 1)
        assert e.value.code == S._ffi.E_UNSUPPORTED
    finally:
        ctx.set_workspace_limit(0)


def test_capacity(S, ctx):
    hashes = [(k, t) for k in range(5) for t in (3, 40 + 10 * k, 200 + 64 * k)]
    k, t = [h[0] for h in hashes], [h[1] for h in hashes]
    args = (k + k, t + t, [0, len(k), 2 * len(k)], [0, 1, 2], 1, 1000, 64, 5, 1)
    want = twin.cells(*args)
    need = len(want["lag"])
    assert need > 4
    for cap in (0, need - 1):
        rc, out, n = ctx.repeats_hashes_raw(*args, cap_cells=cap, fill=FILL)
        assert (rc, n) == (S._ffi.E_CAPACITY, need)
        for key in ("cell_off", "rec_hashes", "rec_pairs", "rec_skipped_keys", "rec_skipped_rows"):
            assert [int(x) for x in out[key]] == want[key]
        for key in ("lag", "block", "pairs", "first", "last"):
            assert [int(x) for x in out[key]] == want[key][:cap]
    rc, out, n = ctx.repeats_hashes_raw(*args, cap_cells=need, fill=FILL)
    assert (rc, n) == (S._ffi.OK, need)
    _same(out, want)


def _untouched(rc, out, n):
    assert n == FILL and all(int(x) == FILL for a in out.values() for x in a)
    return rc


def test_refusals_leave_the_outputs_untouched(S, ctx):
    F = S._ffi
    k, t, ho, rc0 = [1, 1, 2], [5, 50, 7], [0, 2, 3], [0, 2]

    def raw(k=k, t=t, ho=ho, rc0=rc0, min_lag=1, max_lag=100, max_run=64, cell_shift=5, min_cell_pairs=1, flags=0):
        return _untouched(*ctx.repeats_hashes_raw(k, t, ho, rc0, min_lag, max_lag, max_run, cell_shift, min_cell_pairs, flags,
                                                  cap_cells=4, fill=FILL))
    assert raw(rc0=[1, 2]) == F.E_INVALID                                        # rec_clip0 does not start at 0
    assert raw(rc0=[0, 2, 1, 2]) == F.E_INVALID                                  # ... decreases
    assert raw(rc0=[0, 1]) == F.E_INVALID                                        # ... does not end at n_clips
    assert raw(ho=[1, 2, 3]) == F.E_INVALID                                      # hash_off does not start at 0
    assert raw(ho=[0, 3, 2]) == F.E_INVALID                                      # ... decreases
    assert raw(min_lag=101) == F.E_INVALID                                       # max_lag < min_lag
    assert raw(max_lag=1 << 20) == F.E_INVALID
    assert raw(max_run=1) == F.E_INVALID and raw(max_run=1025) == F.E_INVALID
    assert raw(cell_shift=20) == F.E_INVALID
    assert raw(min_cell_pairs=0) == F.E_INVALID
    assert raw(t=[5, 1 << 20, 7]) == F.E_INVALID                                 # a time beyond 20 bits
    assert raw(flags=1) == F.E_INVALID
    assert raw(ho=[0] * 4098, rc0=list(range(4098))) == F.E_UNSUPPORTED          # 4,097 recordings
    assert raw(k=[], t=[], ho=[0, 0, 0], rc0=[0]) == F.E_INVALID                 # clips that belong to no recording
    with pytest.raises(S.ShzError, match="max_run must be in"):
        ctx.repeats_hashes(k, t, ho, rc0, 1, 100, max_run=1)
    # the bounds themselves are fine
    rc, _, n = ctx.repeats_hashes_raw(k, t, ho, rc0, 0, T_MAX, 1024, 19, 1, cap_cells=4)
    assert (rc, n) == (F.OK, 1)
    rc, _, n = ctx.repeats_hashes_raw(k, t, ho, rc0, 7, 7, 2, 0, 0xFFFFFFFF, cap_cells=4)
    assert (rc, n) == (F.OK, 0)
    # NULL handles and arrays, straight at the ABI
    L = F.lib()
    a = {n_: np.asarray(v, d) for n_, v, d in (("k", k, np.uint32), ("t", t, np.uint32), ("ho", ho, np.uint64), ("rc0", rc0, np.uint32))}
    outs = [np.full(4, FILL, np.uint64)] + [np.full(4, FILL, np.uint32) for _ in range(7)] + [np.full(4, FILL, np.uint64) for _ in range(2)]
    cnt = C.c_uint64(FILL)

    def call(h=ctx.h, key=a["k"], t1=a["t"], hoff=a["ho"], rec=a["rc0"], out=outs, count=C.byref(cnt), cap=4):
        return L.shz_repeats_hashes(h, F.ptr(key), F.ptr(t1), F.ptr(hoff), 2, F.ptr(rec), 1, 1, 100, 64, 5, 1, 0,
                                    *[F.ptr(o) for o in out], cap, count)
    assert call(h=None) == F.E_INVALID
    assert call(count=None) == F.E_INVALID
    assert call(key=None) == F.E_INVALID and call(t1=None) == F.E_INVALID
    assert call(hoff=None) == F.E_INVALID and call(rec=None) == F.E_INVALID
    for i in (0, 1, 6, 9):                                                       # cell_off, a cell array, a rec_* array
        assert call(out=outs[:i] + [None] + outs[i + 1:]) == F.E_INVALID
    assert cnt.value == FILL and all(int(x) == FILL for o in outs for x in o)
    assert call(out=outs[:1] + [None] * 5 + outs[6:], cap=0) == F.E_CAPACITY     # (without room the cell arrays may be NULL)
    assert cnt.value == 1
    # the fused call: its own refusals, before anything is extracted
    pcm = np.zeros(8192, np.int16)

    def fused(off=(0, 8192), rc0=(0, 1), fan_value=5, **kw):
        p = dict(min_lag=1, max_lag=100, max_run=64, cell_shift=5, min_cell_pairs=1)
        p.update(kw)
        rc, out, n, ms = ctx.repeats_batch_raw(pcm, list(off), list(rc0), fan_value=fan_value, cap_cells=4, fill=FILL, **p)
        assert ms == (float(np.float32(FILL)),) * 3                              # the three times too
        return _untouched(rc, out, n)
    assert fused(fan_value=0) == F.E_INVALID and fused(fan_value=65) == F.E_INVALID
    assert fused(max_lag=1 << 20) == F.E_INVALID and fused(max_run=1025) == F.E_INVALID and fused(cell_shift=20) == F.E_INVALID
    assert fused(min_cell_pairs=0) == F.E_INVALID and fused(min_lag=200) == F.E_INVALID
    assert fused(rc0=(1, 1)) == F.E_INVALID and fused(off=(0, 8192, 4096), rc0=(0, 2)) == F.E_INVALID
    assert L.shz_repeats_batch(None, *[None] * 2, 0, None, 0, 44100, 10.0, 5, 1, 100, 64, 5, 1, 0, *[None] * 10, 0, None, None, None,
                               None) == F.E_INVALID
    # silence: a recording without hashes
    rc, out, n, _ = ctx.repeats_batch_raw(pcm, [0, 8192], [0, 1], 1, 100, cap_cells=4)
    assert (rc, n) == (F.OK, 0) and [int(x) for x in out["cell_off"]] == [0, 0] and int(out["rec_hashes"][0]) == 0


# ---- planted audio ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """The four recordings and what was planted in them: (start, end, lag) in seconds of the earlier airing"""
    from oracle import synth
    songs = [synth.music_clip(11, c, 8 * SR) for c in range(4)]
    N = lambda s, c, n: synth.traffic_noise(s, c, n * SR)                        # noqa: E731
    a, j, b = songs[1][SR:7 * SR], songs[0][2 * SR:5 * SR], songs[3][SR:5 * SR]
    recs = [np.concatenate([N(5, 0, 3), a, N(5, 1, 2), songs[3][:4 * SR], a, N(5, 2, 2)]),
            np.concatenate([N(5, 0, 3), songs[0], songs[2], N(5, 1, 2)]),
            np.concatenate([N(6, 0, 2), j, N(6, 1, 4), j, songs[2][:5 * SR], j, N(6, 2, 1)]),
            np.concatenate([N(7, 0, 1), a, N(7, 1, 6), b, N(7, 2, 1), a, N(7, 3, 6), b, N(7, 4, 1)])]
    truth = [[(3, 9, 12)], [], [(2, 5, 7), (2, 5, 15), (9, 12, 8)], [(1, 7, 17), (13, 17, 17)]]
    return recs, truth


@pytest.fixture(scope="module")
def found(S, ctx, planted):
    reps = S.find_repeats(planted[0], Fs=SR, min_lag_seconds=1, ctx=ctx)
    (_, cells, rep, _, _), = S.repeats._find_raw(planted[0], SR, 1, None, 5, 8, 1, 1, 100, 64, None, ctx)   # the same calls' arrays
    return reps, cells, rep


def test_planted_repeats_are_found(S, planted, found):
    reps, _, _ = found
    frames = lambda sec: sec * SR / HOP                                          # noqa: E731
    for r, truth in enumerate(planted[1]):
        mine = [p for p in reps if p["recording"] == r]
        print(r, [(p["first"], p["last"], p["lag"], p["lag_lo"], p["lag_hi"], p["pairs"]) for p in mine], mine[0]["stats"] if mine else "")
        assert len(mine) == len(truth)
        for p, (start, end, lag) in zip(mine, sorted(truth, key=lambda x: (x[0], x[2]))):
            assert math.floor(frames(lag)) <= p["lag_lo"] <= p["lag"] <= p["lag_hi"] <= math.ceil(frames(lag))
            # inside the planted span widened by one frame: last <= end + 1 as it stands.  The lower side is taken from the
            # frame that holds the span's first sample, floor(start) - 1 <= first: frame f covers the samples [f, f + 2) hops,
            # so the frame in front of floor(start) still reaches into the planted audio and may carry its first peak (the
            # reference's own hashes put `first` at 42 for a span that begins at frame 43.07)
            assert math.floor(frames(start)) - 1 <= p["first"] <= p["last"] <= frames(end) + 1
            assert p["last"] - p["first"] >= 0.9 * (frames(end) - frames(start))
            assert p["pairs"] >= 100 and p["rec"] == r
            assert p["first_start_seconds"] == round(p["first"] * HOP / SR, 5)
            assert p["second_start_seconds"] == round((p["first"] + p["lag"]) * HOP / SR, 5)
            assert abs(p["lag_seconds"] - lag) <= HOP / SR


def test_occurrences_group_the_three_airings(S, found):
    reps, _, _ = found
    groups = S.occurrences(reps)
    want = twin.occurrences(reps)
    assert [(g["recording"], g["intervals"]) for g in groups] == want
    three = [g for g in groups if g["recording"] == 2]
    assert len(three) == 1 and len(three[0]["intervals"]) == 3 and len(three[0]["repeats"]) == 3
    assert [len(g["intervals"]) for g in groups if g["recording"] == 0] == [2]
    assert [len(g["intervals"]) for g in groups if g["recording"] == 3] == [2, 2]


def test_planted_cells_and_repeats_equal_the_twin_on_the_gpus_hashes(S, ctx, planted, found):
    _, cells, rep = found
    k, t1, ho = S.fingerprint_batch(planted[0], ctx=ctx)
    lo = max(1, int(round(1 * SR / HOP)))
    want = twin.cells(k, t1, ho, list(range(5)), lo, T_MAX, 64, 5, 8)
    _same(cells, want)
    assert want["rec_pairs"][1] < min(want["rec_pairs"][r] for r in (0, 2, 3)) // 4   # the control: far fewer pairs
    folded = twin.fold(want["cell_off"], want["lag"], want["block"], want["pairs"], want["first"], want["last"], 1, 1, 100)
    assert len(folded) == 6
    for key, _ in S._ffi.REPEAT_FIELDS:
        assert [int(x) for x in rep[key]] == [w[key] for w in folded]


def test_batch_equals_hashes(S, ctx, planted):
    """the fused call == the host-column form on fingerprint_batch's output: mono and stereo, host PCM and device PCM"""
    recs = planted[0]
    F = S._ffi
    for clips, rc0 in (([recs[0], recs[2]], [0, 1, 2]),                            # mono
                       ([recs[0], recs[2], recs[3], recs[3], recs[1]], [0, 2, 4, 5])):   # stereo: two takes | the same twice | mono
        off = np.zeros(len(clips) + 1, np.uint64)
        off[1:] = np.cumsum([len(c) for c in clips])
        pcm = np.concatenate(clips)
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, off)
        want = ctx.repeats_hashes(k, t1, ho, rc0, 22, 5000, 64, 5, 2)
        assert len(want["lag"]) > 10
        for debug in (0, F.DEBUG_REPEAT_SMALL_SLICES):
            ctx.set_debug(debug)
            try:
                got, ms = ctx.repeats_batch(pcm, off, rc0, 22, 5000, 64, 5, 2)
                _same(got, want, "host pcm")
                assert all(m > 0 for m in ms)
                buf = ctx.alloc(pcm.nbytes)
                try:
                    buf.upload(pcm)
                    got, _ = ctx.repeats_batch(buf, off, rc0, 22, 5000, 64, 5, 2, pcm_device=True, cap_cells=len(want["lag"]))
                    _same(got, want, "device pcm")
                finally:
                    buf.free()
            finally:
                ctx.set_debug(0)


def test_find_repeats_hashes_and_stereo_recordings(S, ctx, planted, found):
    recs = planted[0]
    k, t1, ho = S.fingerprint_batch(recs, ctx=ctx)
    assert S.find_repeats_hashes(k, t1, ho, Fs=SR, min_lag_seconds=1, ctx=ctx) == found[0]
    # a stereo recording whose channels are the same take: the hashes collapse, the repeat is the mono one's
    both = S.find_repeats([[recs[0], recs[0]]], Fs=SR, min_lag_seconds=1, ctx=ctx)
    assert both == [p for p in found[0] if p["recording"] == 0]


def test_more_recordings_than_a_call_holds_are_split(S, ctx, planted, found, monkeypatch):
    """find_repeats / find_repeats_hashes cut their recordings into calls of MAX_RECS: with 2 a call (a last call of one) and
    with 3, stereo recordings among them, the repeats are the one call's -- recording numbers, CSR rebasing and all"""
    recs = planted[0]
    mixed = [recs[0], [recs[2], recs[2]], recs[1], [recs[3], recs[0]], recs[2]]
    whole = S.find_repeats(mixed, Fs=SR, min_lag_seconds=1, ctx=ctx)
    assert [p["recording"] for p in whole if p["recording"] in (0, 1, 4)] == [0, 1, 1, 1, 4, 4, 4] and len(whole) > 7
    chans = [recs[0], recs[2], recs[2], recs[1], recs[3], recs[0], recs[2]]
    rc0 = [0, 1, 3, 4, 6, 7]
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    assert S.find_repeats_hashes(k, t1, ho, rc0, Fs=SR, min_lag_seconds=1, ctx=ctx) == whole
    for most in (2, 3):
        monkeypatch.setattr(S.repeats, "MAX_RECS", most)
        assert S.find_repeats(mixed, Fs=SR, min_lag_seconds=1, ctx=ctx) == whole
        assert S.find_repeats_hashes(k, t1, ho, rc0, Fs=SR, min_lag_seconds=1, ctx=ctx) == whole


def test_resample_to_goes_through_the_device_resampler(S, ctx, planted):
    """find_repeats(resample_to=): the recordings, taken as 48 kHz audio, are resampled on the device and the frames counted at
    the new rate -- the repeats are those of the hashes fingerprint_batch(resample_to=) gives for the same audio"""
    recs = [planted[0][0], planted[0][2]]
    got = S.find_repeats(recs, Fs=48000, min_lag_seconds=1, resample_to=SR, ctx=ctx)
    k, t1, ho = S.fingerprint_batch(recs, Fs=48000, ctx=ctx, resample_to=SR)
    assert got == S.find_repeats_hashes(k, t1, ho, Fs=SR, min_lag_seconds=1, ctx=ctx)
    assert [p["recording"] for p in got] == [0, 1, 1, 1]
    plain = S.find_repeats(recs, Fs=SR, min_lag_seconds=1, ctx=ctx)
    assert len(plain) == len(got)
    for p, q in zip(got, plain):                                                 # the same airings, 48000 / 44100 slower
        assert abs(p["lag"] - q["lag"] * SR / 48000) <= 2 and p["lag"] < q["lag"]
