"""GPU: content shared between recordings (shz_shared_hashes / shz_shared_batch / find_shared) against the plain-Python
definition in tests/shared_twin.py, array for array: built hash lists at every edge of the definition (runs at max_run on
either side, lags at both ends of the 21-bit field, windows cut at 0 and at 2^20 - 1, block borders, tiles of 64 and 2,048
pairs, jobs without items or pairs), fuzz, slices, capacity, refusals, and planted audio.  Every comparison runs with debug 0
and with SHZ_DEBUG_REPEAT_SMALL_SLICES (one job a slice, tiles of 64 pairs, blocks of 64 items)."""
import ctypes as C
import math

import numpy as np
import pytest

import repeat_twin
import shared_twin as twin

pytestmark = pytest.mark.gpu

SR, HOP = 44100, 2048
FILL = 0x5A5A5A5A
T_MAX = (1 << 20) - 1
BIAS = 1 << 20
CELL_KEYS = ("cell_off", "lag", "block", "pairs", "first", "last", "rec_hashes", "job_pairs", "job_skipped_keys", "job_skipped_rows")


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _ints(got, k):
    return [int(x) - BIAS for x in got[k]] if k == "lag" else [int(x) for x in got[k]]


def _same(got, want, what=""):
    for k in CELL_KEYS:
        assert _ints(got, k) == [int(x) for x in want[k]], (k, what)


def _check(S, ctx, key32, t1, hash_off, rec_clip0, jobs, lag_lo=-T_MAX, lag_hi=T_MAX, max_run=64, cell_shift=5, min_cell_pairs=1):
    """shared_hashes == the twin, under both slicings; returns the twin's result"""
    want = twin.cells(key32, t1, hash_off, rec_clip0, jobs, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs)
    for debug in (0, S._ffi.DEBUG_REPEAT_SMALL_SLICES):
        ctx.set_debug(debug)
        try:
            got = ctx.shared_hashes(key32, t1, hash_off, rec_clip0, jobs, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs)
        finally:
            ctx.set_debug(0)
        _same(got, want, f"debug {debug}")
    return want


def _mono(recs):
    """mono recordings from lists of (key, t): key32, t1, hash_off, rec_clip0"""
    k = [h[0] for r in recs for h in r]
    t = [h[1] for r in recs for h in r]
    ho = [0]
    for r in recs:
        ho.append(ho[-1] + len(r))
    return k, t, ho, list(range(len(recs) + 1))


def _recs(S, ctx, recs, jobs, **kw):
    return _check(S, ctx, *_mono(recs), jobs, **kw)


def _per_lag(want, j):
    out = {}
    for i in range(want["cell_off"][j], want["cell_off"][j + 1]):
        out[want["lag"][i]] = out.get(want["lag"][i], 0) + want["pairs"][i]
    return out


# ---- built lists ----------------------------------------------------------------------------------------------------------
def test_runs_of_exactly_max_run_and_one_more_on_either_side(S, ctx):
    for max_run in (2, 5, 1024):
        a = [(7, 3 * i) for i in range(max_run)] + [(9, 2 * i) for i in range(max_run + 1)] + [(11, 4)] + [(13, 6)] \
            + [(15, 5 * i) for i in range(max_run + 1)]                          # 15: over the limit here, absent from b
        b = [(7, 50)] + [(9, 60)] + [(11, 7 * i) for i in range(max_run)] + [(13, 2 * i + 1) for i in range(max_run + 1)] + [(16, 1)]
        want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)], max_run=max_run)
        assert want["job_pairs"] == [2 * max_run] * 2
        assert want["job_skipped_keys"] == [2, 2] and want["job_skipped_rows"] == [2 * (max_run + 2)] * 2


def test_lags_at_the_ends_of_the_field_and_windows_cut_at_the_ends_of_time(S, ctx):
    a = [(1, 0), (2, 77), (3, T_MAX)]
    b = [(1, T_MAX), (2, 77), (3, 0)]
    want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)])
    assert want["lag"] == [-T_MAX, 0, T_MAX] * 2 and want["first"] == [T_MAX, 77, 0, T_MAX, 77, 0]
    # one run on either side: windows below 0, above 2^20 - 1, wholly outside on both sides, of one lag, at the field's ends
    a = [(5, t) for t in (0, 5, 100, T_MAX - 5, T_MAX)]
    b = [(5, t) for t in (0, 3, 8, 90, 105, T_MAX - 50, T_MAX - 2, T_MAX)]
    seen = []
    for lo, hi in ((-T_MAX, T_MAX), (0, 0), (-100, 10), (-10, 100), (-100, -50), (50, 100), (3, 3), (-5, -5), (-T_MAX, -T_MAX),
                   (T_MAX, T_MAX), (T_MAX - 5, T_MAX), (-T_MAX, 5 - T_MAX), (-2, 3), (-T_MAX, -1), (1, T_MAX)):
        want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)], lag_lo=lo, lag_hi=hi)
        assert all(lo <= g <= hi for g in want["lag"])
        seen.append(want["job_pairs"])
    assert seen[0] == [40, 40] and seen[1] == [2, 2] and seen[8] == [1, 1] and seen[9] == [1, 1]
    assert seen[4][0] > 0 and seen[5][0] > 0                                     # (cut, not empty: t_a = 100 and T_MAX - 5 reach b)
    # wholly outside: every t_a + window misses [0, 2^20 - 1]
    want = _recs(S, ctx, [[(5, 0), (5, 9)], [(5, 0), (5, 3)]], [(0, 1)], lag_lo=-100, lag_hi=-10)
    assert want["job_pairs"] == [0]
    want = _recs(S, ctx, [[(5, T_MAX), (5, T_MAX - 9)], [(5, T_MAX), (5, T_MAX - 3)]], [(0, 1)], lag_lo=10, lag_hi=100)
    assert want["job_pairs"] == [0]


def test_times_at_the_block_border(S, ctx):
    for shift in (0, 5, 19):
        edge = 1 << shift
        a = [(1, edge - 1), (2, edge), (3, 0), (4, edge - 1), (4, edge)]
        b = [(1, edge - 1 + 50), (2, edge + 50), (3, 50), (4, edge + 49), (4, edge + 50)]
        want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)], cell_shift=shift, lag_lo=-100, lag_hi=100)
        assert want["job_pairs"] == [7, 7]
        assert set(want["block"][:want["cell_off"][1]]) == ({0, 1} if shift else {0, edge - 1, edge})


def test_min_cell_pairs_drops_cells(S, ctx):
    a = [(k, 4 + k) for k in range(6)] + [(k, 40 + k) for k in range(10, 13)] + [(20, 70)]
    b = [(k, 104 + k) for k in range(6)] + [(k, 140 + k) for k in range(10, 13)] + [(20, 170)]
    for mcp, pairs in ((1, [6, 3, 1]), (3, [6, 3]), (4, [6]), (7, [])):
        want = _recs(S, ctx, [a, b], [(0, 1)], min_cell_pairs=mcp)
        assert want["pairs"] == pairs and want["job_pairs"] == [10] and want["lag"] == [100] * len(pairs)
    want = _recs(S, ctx, [a, b], [(1, 0)], min_cell_pairs=3)
    assert want["lag"] == [-100, -100] and want["first"] == [104, 150]


def test_run_across_every_block_border(S, ctx):
    """300 entries of one key in a behind 0 .. 70 items without a partner, against 11 entries in b: the items, their partner
    ranges and the pairs' tiles straddle every 64- and 256-item border in turn"""
    b = [(1000, 40 + 31 * i) for i in range(11)] + [(2000, 1)]
    for filler in range(71):
        a = [(k, 11) for k in range(filler)] + [(1000, 50 + i) for i in range(300)]
        _recs(S, ctx, [a, b], [(0, 1)], lag_lo=-40, lag_hi=25, max_run=512, cell_shift=3)
    a = [(k, 11) for k in range(33)] + [(1000, 50 + i) for i in range(300)]
    want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)], max_run=512, cell_shift=4)
    assert want["job_pairs"] == [3300, 3300]


def test_sets_collapse_and_lonely_keys_give_nothing(S, ctx):
    # recording 0 is stereo: (1, 10) in both channels and twice in the left one; recording 1 holds it three times
    k = [1, 1, 2, 1, 3,   1, 1, 1, 4]
    t = [10, 10, 5, 10, 9,  40, 40, 40, 5]
    want = _check(S, ctx, k, t, [0, 3, 5, 9], [0, 2, 3], [(0, 1), (1, 0)])
    assert want["rec_hashes"] == [3, 2] and want["job_pairs"] == [1, 1] and want["lag"] == [30, -30]
    # keys 2, 3 (only in 0) and 4 (only in 1): nothing, and nothing skipped
    assert want["job_skipped_keys"] == [0, 0]


def test_tiles_of_64_and_of_2048_pairs_exactly_and_one_more(S, ctx):
    for m_a, m_b, extra in ((32, 2, 0), (32, 2, 1), (32, 64, 0), (32, 64, 1), (1, 1, 0)):
        a = [(50, 3 * i) for i in range(m_a)] + [(60, 7)] * extra
        b = [(50, 2 * i) for i in range(m_b)] + [(60, 9)] * extra
        want = _recs(S, ctx, [a, b], [(0, 1)], max_run=64, cell_shift=2)
        assert want["job_pairs"] == [m_a * m_b + extra]


def test_items_without_partners_at_the_head_in_the_middle_and_at_the_end(S, ctx):
    a = [(1, 3), (1, 4), (5, 10), (5, 20), (6, 1), (6, 2), (6, 3), (7, 30), (9, 8), (9, 9)]
    b = [(5, 15), (7, 31), (7, 29), (8, 0)]
    want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)])
    assert want["job_pairs"] == [4, 4] and want["lag"] == [-5, -1, 1, 5, -5, -1, 1, 5]
    # ... with a window that leaves a key of both recordings without a pair (5: lags -5 and 5)
    want = _recs(S, ctx, [a, b], [(0, 1)], lag_lo=-1, lag_hi=4)
    assert want["job_pairs"] == [2]


def test_jobs(S, ctx):
    r0 = [(1, 10), (2, 20), (3, 30)]
    r1 = []
    r2 = [(1, 15), (3, 25), (3, 300)]
    r3 = [(9, 9)]
    r4 = [(2, 1000), (1, 10)]
    recs = [r0, r1, r2, r3, r4]
    # an empty recording as a and as b; jobs without pairs first, between and last; one a against many b; a job twice
    jobs = [(1, 0), (0, 2), (0, 1), (0, 3), (0, 4), (0, 2), (3, 0), (2, 0), (4, 3)]
    want = _recs(S, ctx, recs, jobs)
    assert want["job_pairs"] == [0, 3, 0, 0, 2, 3, 0, 3, 0] and want["rec_hashes"] == [3, 0, 3, 1, 2]
    c = want["cell_off"]
    assert [want[k][c[1]:c[2]] for k in ("lag", "first")] == [want[k][c[5]:c[6]] for k in ("lag", "first")]
    # (a, b) and (b, a): the same counters, the lags mirrored
    rng = np.random.default_rng(3)
    a = [(int(k), int(t)) for k, t in zip(rng.integers(0, 12, 300), rng.integers(0, 500, 300))]
    b = [(int(k), int(t)) for k, t in zip(rng.integers(0, 12, 200), rng.integers(0, 500, 200))] + [(5, t) for t in range(600, 650)]
    want = _recs(S, ctx, [a, b], [(0, 1), (1, 0)], max_run=40, min_cell_pairs=1)
    assert want["job_pairs"][0] == want["job_pairs"][1] > 1000
    assert want["job_skipped_keys"][0] == want["job_skipped_keys"][1] >= 1
    assert want["job_skipped_rows"][0] == want["job_skipped_rows"][1]
    assert _per_lag(want, 0) == {-g: n for g, n in _per_lag(want, 1).items()}
    # no jobs: rec_hashes all the same
    want = _recs(S, ctx, recs, [])
    assert want["cell_off"] == [0] and want["rec_hashes"] == [3, 0, 3, 1, 2]
    # no hashes at all, with and without jobs; no recordings
    want = _check(S, ctx, [], [], [0, 0, 0], [0, 1, 2], [(0, 1), (1, 0)])
    assert want["cell_off"] == [0, 0, 0] and want["rec_hashes"] == [0, 0]
    _check(S, ctx, [], [], [0], [0], [])


def test_fuzz(S, ctx):
    rng = np.random.default_rng(2027)
    for case in range(36):
        n_recs = 6
        k, t, ho, rc0 = [], [], [0], [0]
        for _ in range(n_recs):
            for _ in range(int(rng.integers(1, 3))):
                n = int(rng.integers(0, 401)) // 2
                k.extend(int(x) for x in rng.integers(0, 40, n))
                tt = rng.integers(0, 4096, n)
                tt[rng.random(n) < 0.02] = T_MAX
                t.extend(int(x) for x in tt)
                ho.append(len(k))
            rc0.append(len(ho) - 1)
        jobs = []
        while len(jobs) < 10:
            a, b = (int(x) for x in rng.integers(0, n_recs, 2))
            if a != b:
                jobs.append((a, b))
        lo, hi = sorted(int(x) for x in rng.integers(-5000, 5001, 2))
        if case % 6 == 0:
            lo, hi = -T_MAX, T_MAX
        _check(S, ctx, k, t, ho, rc0, jobs, lag_lo=lo, lag_hi=hi, max_run=(2, 5, 64)[case % 3], cell_shift=(0, 5, 19)[(case // 3) % 3],
               min_cell_pairs=(1, 3)[(case // 9) % 2])


def test_slices_of_several_jobs(S, ctx):
    """the workspace limit cuts the jobs into slices of more than one; a job that alone exceeds a slice is refused"""
    rng = np.random.default_rng(8)
    recs = []
    for r in range(5):
        n = 40 + 20 * (r % 3)
        recs.append([(int(x), int(y)) for x, y in zip(rng.integers(0, 6, n), rng.integers(0, 300, n))])
    k, t, ho, rc0 = _mono(recs)
    jobs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (2, 0), (1, 3), (3, 1), (0, 4)]
    want = twin.cells(k, t, ho, rc0, jobs, -400, 400, 64, 4, 1)
    assert 700 < max(want["job_pairs"]) <= 900 and min(want["job_pairs"]) > 350 and sum(want["job_pairs"]) > 4000
    try:
        ctx.set_workspace_limit(128 * 900)             # 900 pairs a slice: one or two jobs
        _same(ctx.shared_hashes(k, t, ho, rc0, jobs, -400, 400, 64, 4, 1), want)
        ctx.set_workspace_limit(128 * 700)
        with pytest.raises(S.ShzError, match=r"job 1 \(recordings 1 and 2\) has 756 pairs.*lag window \[-400, 400\].*max_run \(64\)") as e:
            ctx.shared_hashes(k, t, ho, rc0, jobs, -400, 400, 64, 4, 1)
        assert e.value.code == S._ffi.E_UNSUPPORTED
    finally:
        ctx.set_workspace_limit(0)


def test_capacity(S, ctx):
    a = [(k, t) for k in range(5) for t in (3, 40 + 10 * k)]
    b = [(k, t) for k in range(5) for t in (7, 200 + 64 * k)]
    args = (*_mono([a, b]), [(0, 1), (1, 0)], -1000, 1000, 64, 5, 1)
    want = twin.cells(*args)
    need = len(want["lag"])
    assert need > 4
    for cap in (0, need - 1):
        rc, out, n = ctx.shared_hashes_raw(*args, cap_cells=cap, fill=FILL)
        assert (rc, n) == (S._ffi.E_CAPACITY, need)
        for key in ("cell_off", "rec_hashes", "job_pairs", "job_skipped_keys", "job_skipped_rows"):
            assert _ints(out, key) == want[key]
        for key in ("lag", "block", "pairs", "first", "last"):
            assert _ints(out, key) == want[key][:cap]
    rc, out, n = ctx.shared_hashes_raw(*args, cap_cells=need, fill=FILL)
    assert (rc, n) == (S._ffi.OK, need)
    _same(out, want)


def _untouched(rc, out, n):
    assert n == FILL and all(int(x) == FILL for a in out.values() for x in a)
    return rc


def test_refusals_leave_the_outputs_untouched(S, ctx):
    F = S._ffi
    k, t, ho, rc0 = [1, 1, 2, 1], [5, 50, 7, 9], [0, 2, 3, 4], [0, 2, 3]

    def raw(k=k, t=t, ho=ho, rc0=rc0, jobs=((0, 1),), lag_lo=-100, lag_hi=100, max_run=64, cell_shift=5, min_cell_pairs=1, flags=0):
        return _untouched(*ctx.shared_hashes_raw(k, t, ho, rc0, jobs, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs, flags,
                                                 cap_cells=4, fill=FILL))
    assert raw(rc0=[1, 2, 3]) == F.E_INVALID                                     # rec_clip0 does not start at 0
    assert raw(rc0=[0, 2, 1, 3]) == F.E_INVALID                                  # ... decreases
    assert raw(rc0=[0, 1, 2]) == F.E_INVALID                                     # ... does not end at n_clips
    assert raw(ho=[1, 2, 3, 4]) == F.E_INVALID                                   # hash_off does not start at 0
    assert raw(ho=[0, 3, 2, 4]) == F.E_INVALID                                   # ... decreases
    assert raw(lag_lo=101) == F.E_INVALID                                        # lag_hi < lag_lo
    assert raw(lag_hi=1 << 20) == F.E_INVALID and raw(lag_lo=-(1 << 20)) == F.E_INVALID
    assert raw(lag_lo=-(1 << 31), lag_hi=(1 << 31) - 1) == F.E_INVALID
    assert raw(max_run=1) == F.E_INVALID and raw(max_run=1025) == F.E_INVALID
    assert raw(cell_shift=20) == F.E_INVALID
    assert raw(min_cell_pairs=0) == F.E_INVALID
    assert raw(t=[5, 1 << 20, 7, 9]) == F.E_INVALID                              # a time beyond 20 bits
    assert raw(flags=1) == F.E_INVALID
    assert raw(jobs=((0, 0),)) == F.E_INVALID and raw(jobs=((0, 1), (1, 1))) == F.E_INVALID      # a == b
    assert raw(jobs=((0, 2),)) == F.E_INVALID and raw(jobs=((2, 0),)) == F.E_INVALID             # a recording that is not there
    assert raw(jobs=((0, 1),) * 4097) == F.E_UNSUPPORTED                         # 4,097 jobs
    assert raw(ho=[0] * 4098, rc0=list(range(4098))) == F.E_UNSUPPORTED          # 4,097 recordings
    assert raw(k=[], t=[], ho=[0, 0, 0], rc0=[0], jobs=()) == F.E_INVALID        # clips that belong to no recording
    with pytest.raises(S.ShzError, match="joins recording 1 with itself"):
        ctx.shared_hashes(k, t, ho, rc0, [(1, 1)], -100, 100)
    # the bounds themselves are fine
    rc, _, n = ctx.shared_hashes_raw(k, t, ho, rc0, [(0, 1)] * 4096, -T_MAX, T_MAX, 1024, 19, 1, cap_cells=8192)
    assert (rc, n) == (F.OK, 8192)                                               # (two cells a job)
    rc, _, n = ctx.shared_hashes_raw(k, t, ho, rc0, [(0, 1)], 4, 4, 2, 0, 0xFFFFFFFF, cap_cells=4)
    assert (rc, n) == (F.OK, 0)
    # NULL handles and arrays, straight at the ABI
    L = F.lib()
    a = {n_: np.asarray(v, d) for n_, v, d in (("k", k, np.uint32), ("t", t, np.uint32), ("ho", ho, np.uint64), ("rc0", rc0, np.uint32),
                                               ("ja", [0], np.uint32), ("jb", [1], np.uint32))}
    # cell_off | lag block pairs first last | rec_hashes | job_pairs | job_skipped_keys | job_skipped_rows
    outs = [np.full(4, FILL, d) for d in (np.uint64, *[np.uint32] * 6, np.uint64, np.uint32, np.uint64)]
    cnt = C.c_uint64(FILL)

    def call(h=ctx.h, key=a["k"], t1=a["t"], hoff=a["ho"], rec=a["rc0"], ja=a["ja"], jb=a["jb"], out=outs, count=C.byref(cnt), cap=4):
        return L.shz_shared_hashes(h, F.ptr(key), F.ptr(t1), F.ptr(hoff), 3, F.ptr(rec), 2, F.ptr(ja), F.ptr(jb), 1, -100, 100, 64, 5, 1, 0,
                                   *[F.ptr(o) for o in out], cap, count)
    assert call(h=None) == F.E_INVALID
    assert call(count=None) == F.E_INVALID
    assert call(key=None) == F.E_INVALID and call(t1=None) == F.E_INVALID
    assert call(hoff=None) == F.E_INVALID and call(rec=None) == F.E_INVALID
    assert call(ja=None) == F.E_INVALID and call(jb=None) == F.E_INVALID         # a NULL job list with a job
    for i in (0, 1, 6, 7, 9):                                                    # cell_off, a cell array, rec_hashes, job_* arrays
        assert call(out=outs[:i] + [None] + outs[i + 1:]) == F.E_INVALID
    assert cnt.value == FILL and all(int(x) == FILL for o in outs for x in o)
    assert call(out=outs[:1] + [None] * 5 + outs[6:], cap=0) == F.E_CAPACITY     # (without room the cell arrays may be NULL)
    assert cnt.value == 2
    # the fused call: its own refusals, before anything is extracted
    pcm = np.zeros(16384, np.int16)

    def fused(off=(0, 8192, 16384), rc0=(0, 1, 2), jobs=((0, 1),), fan_value=5, **kw):
        p = dict(lag_lo=-100, lag_hi=100, max_run=64, cell_shift=5, min_cell_pairs=1)
        p.update(kw)
        rc, out, n, ms = ctx.shared_batch_raw(pcm, list(off), list(rc0), jobs, fan_value=fan_value, cap_cells=4, fill=FILL, **p)
        assert ms == (float(np.float32(FILL)),) * 3                              # the three times too
        return _untouched(rc, out, n)
    assert fused(fan_value=0) == F.E_INVALID and fused(fan_value=65) == F.E_INVALID
    assert fused(lag_hi=1 << 20) == F.E_INVALID and fused(max_run=1025) == F.E_INVALID and fused(cell_shift=20) == F.E_INVALID
    assert fused(min_cell_pairs=0) == F.E_INVALID and fused(lag_lo=200) == F.E_INVALID
    assert fused(jobs=((1, 1),)) == F.E_INVALID and fused(jobs=((0, 2),)) == F.E_INVALID
    assert fused(rc0=(1, 1, 2)) == F.E_INVALID and fused(off=(0, 8192, 4096)) == F.E_INVALID
    assert L.shz_shared_batch(None, *[None] * 2, 0, None, 0, 44100, 10.0, 5, None, None, 0, -1, 1, 64, 5, 1, 0, *[None] * 10, 0, None,
                              None, None, None) == F.E_INVALID
    # silence: recordings without hashes
    rc, out, n, _ = ctx.shared_batch_raw(pcm, [0, 8192, 16384], [0, 1, 2], [(0, 1)], -100, 100, cap_cells=4)
    assert (rc, n) == (F.OK, 0) and [int(x) for x in out["cell_off"]] == [0, 0] and [int(x) for x in out["rec_hashes"]] == [0, 0]


# ---- planted audio ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """The four recordings of tests/test_gpu_repeats.py, built the same way, and what they share: per job (a, b) the stretches
    (start, end, lag) -- seconds of a, and seconds from a to b"""
    from oracle import synth
    songs = [synth.music_clip(11, c, 8 * SR) for c in range(4)]
    N = lambda s, c, n: synth.traffic_noise(s, c, n * SR)                        # noqa: E731
    a, j, b = songs[1][SR:7 * SR], songs[0][2 * SR:5 * SR], songs[3][SR:5 * SR]
    recs = [np.concatenate([N(5, 0, 3), a, N(5, 1, 2), songs[3][:4 * SR], a, N(5, 2, 2)]),
            np.concatenate([N(5, 0, 3), songs[0], songs[2], N(5, 1, 2)]),
            np.concatenate([N(6, 0, 2), j, N(6, 1, 4), j, songs[2][:5 * SR], j, N(6, 2, 1)]),
            np.concatenate([N(7, 0, 1), a, N(7, 1, 6), b, N(7, 2, 1), a, N(7, 3, 6), b, N(7, 4, 1)])]
    truth = {(0, 1): [(0, 3, 0)],                                                # the common noise head
             # a at 3 and 15 s of 0, at 1 and 18 s of 3; songs[3][1:4] at 12 s of 0, at 13 and 30 s of 3
             (0, 3): [(3, 9, -2), (3, 9, 15), (15, 21, -14), (15, 21, 3), (12, 15, 1), (12, 15, 18)],
             # songs[0][2:5] at 5 s of 1, at 2, 9 and 17 s of 2; songs[2][:5] at 11 s of 1, at 12 s of 2
             (1, 2): [(5, 8, -3), (5, 8, 4), (5, 8, 12), (11, 16, 1)],
             (0, 2): [], (1, 3): [], (2, 3): []}
    return recs, truth


@pytest.fixture(scope="module")
def found(S, ctx, planted):
    return S.find_shared(planted[0], Fs=SR, ctx=ctx)


@pytest.fixture(scope="module")
def hashes(S, ctx, planted):
    return S.fingerprint_batch(planted[0], ctx=ctx)


def test_planted_stretches_are_found(S, planted, found):
    """The 11 stretches of the fixture, in their jobs, at their lags and inside their spans.  Coverage: a stretch [first, last]
    is inclusive and covers last - first + 1 frames; a planted span of n samples holds (n - 4096) // 2048 + 1 WHOLE frames
    (shz_frame_count: frame f is the samples [2048 f, 2048 f + 4096)), the only frames that see nothing but the shared audio,
    and a stretch must cover 0.9 of those.  With the reference's own hashes the weakest are the noise head of (0, 1), frames
    0 .. 57 of 63 (0.92; louder music behind it takes the peaks of its last frames), and the 3 s stretches, 59 of 63 (0.94)."""
    frames = lambda sec: sec * SR / HOP                                          # noqa: E731
    whole = lambda start, end: ((end - start) * SR - 4096) // HOP + 1            # noqa: E731
    jobs = S.shared._all_pairs(4)
    for p in found:
        print((p["rec_a"], p["rec_b"]), p["first"], p["last"], p["lag"], p["lag_lo"], p["lag_hi"], p["pairs"], p["stats"])
    assert len(found) == 11
    for n, job in enumerate(jobs):
        mine = [p for p in found if p["job"] == n]
        truth = planted[1][job]
        assert len(mine) == len(truth), job
        assert all((p["recording_a"], p["recording_b"], p["rec_a"], p["rec_b"]) == (*job, *job) for p in mine)
        for p, (start, end, lag) in zip(mine, sorted(truth, key=lambda x: (x[0], x[2]))):
            assert math.floor(frames(lag)) <= p["lag_lo"] <= p["lag"] <= p["lag_hi"] <= math.ceil(frames(lag))
            # inside the planted span, widened by a frame on either side as test_planted_repeats_are_found widens it
            assert math.floor(frames(start)) - 1 <= p["first"] <= p["last"] <= frames(end) + 1
            print("   cover", p["last"] - p["first"] + 1, "of", whole(start, end))
            assert p["last"] - p["first"] + 1 >= 0.9 * whole(start, end)
            assert p["pairs"] >= 100 and p["stats"]["skipped_keys"] == 0
            secs = lambda f: round(f * HOP / SR, 5)                              # noqa: E731
            assert (p["a_start_seconds"], p["a_end_seconds"]) == (secs(p["first"]), secs(p["last"] + 1))
            assert (p["b_start_seconds"], p["b_end_seconds"]) == (secs(max(0, p["first"] + p["lag"])), secs(p["last"] + p["lag"] + 1))
            assert p["lag_seconds"] == secs(p["lag"]) and abs(p["lag_seconds"] - lag) <= HOP / SR


def test_b_start_seconds_is_clamped_at_zero(S):
    cells = dict(rec_hashes=[5, 6], job_pairs=[9], job_skipped_keys=[0], job_skipped_rows=[0])
    rep = dict(rec=[0], lag=[BIAS - 3], lag_lo=[BIAS - 4], lag_hi=[BIAS - 3], first=[1], last=[40], pairs=[9], cells=[2])
    p, = S.shared._shared_dicts(cells, rep, 7, [(1, 0)], [0, 1], SR, HOP)
    assert (p["lag"], p["lag_lo"], p["lag_hi"], p["job"], p["rec_a"], p["rec_b"]) == (-3, -4, -3, 7, 1, 0)
    assert p["b_start_seconds"] == 0.0 and p["b_end_seconds"] == round(38 * HOP / SR, 5) and p["lag_seconds"] == round(-3 * HOP / SR, 5)
    assert p["stats"] == dict(hashes_a=6, hashes_b=5, pairs=9, skipped_keys=0, skipped_rows=0)


def test_batch_equals_hashes_equals_the_twin_on_the_gpus_hashes(S, ctx, planted, hashes, found):
    """the fused call on host PCM and on device PCM == the host-column form on fingerprint_batch's output == the twin"""
    recs = planted[0]
    F = S._ffi
    k, t1, ho = hashes
    jobs = S.shared._all_pairs(4)
    want = twin.cells(k, t1, ho, list(range(5)), jobs, -T_MAX, T_MAX, 64, 5, 8)
    assert want["job_skipped_keys"] == [0] * 6
    off = np.zeros(5, np.uint64)
    off[1:] = np.cumsum([len(c) for c in recs])
    pcm = np.concatenate(recs)
    for debug in (0, F.DEBUG_REPEAT_SMALL_SLICES):
        ctx.set_debug(debug)
        try:
            _same(ctx.shared_hashes(k, t1, ho, list(range(5)), jobs, -T_MAX, T_MAX, 64, 5, 8), want, "hashes")
            got, ms = ctx.shared_batch(pcm, off, list(range(5)), jobs, -T_MAX, T_MAX, 64, 5, 8)
            _same(got, want, "host pcm")
            assert all(m > 0 for m in ms)
            buf = ctx.alloc(pcm.nbytes)
            try:
                buf.upload(pcm)
                got, _ = ctx.shared_batch(buf, off, list(range(5)), jobs, -T_MAX, T_MAX, 64, 5, 8, pcm_device=True,
                                          cap_cells=len(want["lag"]))
                _same(got, want, "device pcm")
            finally:
                buf.free()
        finally:
            ctx.set_debug(0)
    # the fold of the twin's cells on biased lags is what find_shared reports
    folded = repeat_twin.fold(want["cell_off"], [g + BIAS for g in want["lag"]], want["block"], want["pairs"], want["first"],
                              want["last"], 1, 1, 100)
    assert [(p["job"], p["first"], p["last"], p["lag"], p["lag_lo"], p["lag_hi"], p["pairs"], p["cells"]) for p in found] == \
        [(w["rec"], w["first"], w["last"], w["lag"] - BIAS, w["lag_lo"] - BIAS, w["lag_hi"] - BIAS, w["pairs"], w["cells"]) for w in folded]
    assert S.find_shared_hashes(k, t1, ho, Fs=SR, ctx=ctx) == found


def test_shared_occurrences_group_the_airings(S, ctx, planted, found):
    reps = S.find_repeats(planted[0], Fs=SR, min_lag_seconds=1, ctx=ctx)
    assert len(reps) == 6
    groups = S.shared_occurrences(found, reps)
    assert [(g["airings"], g["shared"], g["repeats"]) for g in groups] == twin.occurrences(found, reps)
    assert [len(g["airings"]) for g in groups] == [2, 4, 3, 4, 2]


def test_a_stereo_recording_as_a_and_mirrored_pairs(S, ctx, planted, found):
    recs = planted[0]
    # both channels the same take: the hashes collapse, the stretches are the mono ones
    both = S.find_shared([[recs[0], recs[0]], recs[3]], pairs=[(0, 1)], Fs=SR, ctx=ctx)
    mono = [p for p in found if p["job"] == 2]
    strip = lambda ps: [{k: v for k, v in p.items() if k not in ("job", "rec_a", "rec_b", "recording_a", "recording_b")} for p in ps]  # noqa: E731
    assert len(both) == 6 and strip(both) == strip(mono)
    # (3, 0) mirrors (0, 3): the same stretches seen from 3, the lags negated
    back = S.find_shared(recs, pairs=[(3, 0)], Fs=SR, ctx=ctx)
    assert sorted((-p["lag_hi"], -p["lag_lo"]) for p in back) == sorted((p["lag_lo"], p["lag_hi"]) for p in mono)
    assert all((p["rec_a"], p["rec_b"], p["job"]) == (3, 0, 0) for p in back)
    assert [p["stats"]["pairs"] for p in back[:1]] == [mono[0]["stats"]["pairs"]]


def test_more_jobs_than_a_call_holds_are_split(S, ctx, planted, found, hashes, monkeypatch):
    """find_shared / find_shared_hashes cut their jobs into calls of MAX_JOBS jobs naming MAX_RECS recordings: the dicts are
    the one call's -- job numbers, the recordings' renumbering and all"""
    k, t1, ho = hashes
    for most_jobs, most_recs in ((2, 4096), (4, 4096), (4096, 3), (1, 2)):
        monkeypatch.setattr(S.shared, "MAX_JOBS", most_jobs)
        monkeypatch.setattr(S.shared, "MAX_RECS", most_recs)
        assert S.find_shared(planted[0], Fs=SR, ctx=ctx) == found
        assert S.find_shared_hashes(k, t1, ho, Fs=SR, ctx=ctx) == found


def test_resample_to_goes_through_the_device_resampler(S, ctx, planted):
    """find_shared(resample_to=): the recordings, taken as 48 kHz audio, are resampled on the device and the frames counted at
    the new rate -- the stretches are those of the hashes fingerprint_batch(resample_to=) gives for the same audio"""
    recs = [planted[0][1], planted[0][2]]
    got = S.find_shared(recs, Fs=48000, resample_to=SR, ctx=ctx)
    k, t1, ho = S.fingerprint_batch(recs, Fs=48000, ctx=ctx, resample_to=SR)
    assert got == S.find_shared_hashes(k, t1, ho, Fs=SR, ctx=ctx)
    assert len(got) == 4
    plain = S.find_shared(recs, Fs=SR, ctx=ctx)
    assert len(plain) == 4
    for p, q in zip(got, plain):                                                 # the same stretches, 48000 / 44100 slower
        assert abs(p["lag"] - q["lag"] * SR / 48000) <= 2 and abs(p["lag"]) <= abs(q["lag"])
