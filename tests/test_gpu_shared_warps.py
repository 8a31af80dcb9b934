"""GPU: altered content shared between recordings (shz_shared_warps_peaks / shz_shared_warps_batch / find_shared at a ladder)
against the plain-Python definition in tests/shared_warp_twin.py, array for array: built peak lists at every edge of the
definition (peaks that leave, bins that fold, frames that merge, the last warped frame, a window per job inside one wave, the
same (a, v) under many jobs, self jobs, runs at max_run on either side, the limits on virtual recordings and warps), fuzz,
capacity, refusals, and the two-recording fixture of DESIGN.md 3.7r.  Every comparison runs with debug 0 and with
SHZ_DEBUG_REPEAT_SMALL_SLICES (one job a slice, tiles of 64 pairs, blocks of 64 items)."""
import ctypes as C
import math

import numpy as np
import pytest

import shared_warp_cases as K
import shared_warp_twin as twin
from warp_twin import warp_peaks_tf

pytestmark = pytest.mark.gpu

SR, HOP = K.SR, K.HOP
FILL = 0x5A5A5A5A
T_MAX = (1 << 20) - 1
BIAS = 1 << 20
S_ONE = 65536
KEYS = ("cell_off", "lag", "block", "pairs", "first", "last", "rec_hashes", "job_hashes", "job_pairs", "job_skipped_keys",
        "job_skipped_rows")
WIDE = (-T_MAX, T_MAX)


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
    for k in KEYS:
        assert _ints(got, k) == [int(x) for x in want[k]], (k, what)


def _both(S, ctx, fn):
    """fn() under both slicings"""
    out = []
    for debug in (0, S._ffi.DEBUG_REPEAT_SMALL_SLICES):
        ctx.set_debug(debug)
        try:
            out.append(fn())
        finally:
            ctx.set_debug(0)
    return out


def _lists(recs):
    """mono recordings from lists of (f, t) in any order: peak_f, peak_t, peak_off, rec_clip0"""
    pf, pt, po = [], [], [0]
    for r in recs:
        r = sorted(r, key=lambda p: (p[1], p[0]))
        pf += [p[0] for p in r]
        pt += [p[1] for p in r]
        po.append(len(pf))
    return pf, pt, po, list(range(len(recs) + 1))


def _check(S, ctx, pf, pt, po, rc0, t16, f16, jobs, max_run=64, cell_shift=5, min_cell_pairs=1):
    """shared_warps_peaks == the twin, under both slicings; returns the twin's result"""
    want = twin.cells(pf, pt, po, rc0, t16, f16, jobs, max_run, cell_shift, min_cell_pairs)
    for n, got in enumerate(_both(S, ctx, lambda: ctx.shared_warps_peaks(pf, pt, po, rc0, t16, f16, jobs, max_run, cell_shift,
                                                                         min_cell_pairs))):
        _same(got, want, f"slicing {n}")
    return want


def _recs(S, ctx, recs, t16, f16, jobs, **kw):
    return _check(S, ctx, *_lists(recs), t16, f16, jobs, **kw)


def _cloud(rng, n, t_hi, f_lo=0, f_hi=2048):
    """n random distinct peaks"""
    return sorted({(int(f), int(t)) for f, t in zip(rng.integers(f_lo, f_hi + 1, n), rng.integers(0, t_hi, n))})


def _warped(peaks, t16, f16, shift=0):
    """the peaks as the warp maps them (and moved by `shift` frames): what the other recording holds when it has the content"""
    f, t = warp_peaks_tf([p[0] for p in peaks], [p[1] for p in peaks], t16, f16)
    return [(int(a), int(b) + shift) for a, b in zip(f, t)]


# ---- built lists ----------------------------------------------------------------------------------------------------------
def test_unit_warp_equals_the_plain_join_on_the_librarys_warped_hashes(S, ctx):
    rng = np.random.default_rng(1)
    a = _cloud(rng, 300, 200, 100, 140)
    recs = [a, [(f, t + 7) for f, t in a[50:250]] + _cloud(rng, 60, 200, 100, 140), _cloud(rng, 100, 200, 100, 140)]
    pf, pt, po, _ = _lists(recs + [a[:40]])
    rc0 = [0, 1, 2, 4]                                                           # recording 2: two clips
    jobs = [(0, 1), (1, 0), (2, 0), (0, 2)]
    want = _check(S, ctx, pf, pt, po, rc0, [S_ONE], [S_ONE], [(a_, b_, 0, *WIDE) for a_, b_ in jobs], max_run=16, cell_shift=3)
    assert want["job_pairs"][0] > 500 and want["job_hashes"] == [want["rec_hashes"][j[0]] for j in jobs]
    k, t1, ho = ctx.warp_pair_hash_tf(pf, pt, po, [S_ONE], [S_ONE])
    plain = ctx.shared_hashes(k, t1, ho, rc0, jobs, *WIDE, 16, 3, 1)
    got = ctx.shared_warps_peaks(pf, pt, po, rc0, [S_ONE], [S_ONE], [(a_, b_, 0, *WIDE) for a_, b_ in jobs], 16, 3, 1)
    for key in KEYS:
        if key != "job_hashes":
            assert [int(x) for x in got[key]] == [int(x) for x in plain[key]], key


def test_peaks_that_leave_and_bins_that_fold(S, ctx):
    rng = np.random.default_rng(2)
    a = _cloud(rng, 400, 120, 900, 1200)
    half, twice = 32768, 131072
    # f16 = 0.5: f' = 2 f, everything above bin 1024 leaves; b holds what stays
    b = _warped(a, S_ONE, half, 11)
    assert 0 < len(b) < len(a)
    # f16 = 2: the bins 2 k - 1 and 2 k land on one f'
    c = [(f, t) for t in range(0, 100, 3) for f in (199, 200, 201, 202, 640)]
    d = _warped(c, S_ONE, twice, 5)
    assert len({p for p in d}) < len(c)
    want = _recs(S, ctx, [a, b, c, d], [S_ONE, S_ONE, S_ONE], [half, twice, S_ONE],
                 [(0, 1, 0, *WIDE), (2, 3, 1, *WIDE), (0, 1, 2, *WIDE), (2, 3, 0, *WIDE)], max_run=64)
    assert want["job_hashes"][0] < want["rec_hashes"][0] and want["job_hashes"][2] == want["rec_hashes"][0]
    assert want["job_pairs"][0] > 300 and want["job_pairs"][1] > 100
    at = want["cell_off"]
    assert set(want["lag"][at[0]:at[1]]) >= {11} and 5 in set(want["lag"][at[1]:at[2]])


def test_neighbour_frames_merge_below_unit_tempo(S, ctx):
    rng = np.random.default_rng(3)
    a = _cloud(rng, 500, 90, 300, 420)                                           # about 5 peaks a frame: merged frames interleave
    t16s = [32768, 40000, 65535, 49152]
    recs = [a] + [_warped(a, t, S_ONE, 9) for t in t16s]
    jobs = [(0, 1 + v, v, *WIDE) for v in range(4)] + [(0, 2, 0, *WIDE)]
    want = _recs(S, ctx, recs, t16s, [S_ONE] * 4, jobs, max_run=32, cell_shift=2)
    for j in range(4):
        at = want["cell_off"]
        assert want["job_pairs"][j] >= want["job_hashes"][j] > 500 and 9 in want["lag"][at[j]:at[j + 1]]


def test_last_warped_frame(S, ctx):
    """t16 = 1.5: own frame 699,050 maps to 2^20 - 1 exactly, 699,051 to 2^20 + 1"""
    F = S._ffi
    t16 = 98304
    assert (699050 * t16 + 32768) >> 16 == T_MAX
    a = [(100, 699046), (200, 699050)]                                           # one hash, at t' = 1048569, dt' = 6
    b = [(100, 50), (200, 56)]
    want = _recs(S, ctx, [a, b], [t16], [S_ONE], [(0, 1, 0, *WIDE), (0, 1, 0, 0, T_MAX)])
    assert want["job_pairs"] == [1, 0] and want["lag"] == [50 - 1048569] and want["first"] == [1048569]
    pf, pt, po, rc0 = _lists([[(100, 699046), (200, 699051)], b])
    rc, out, n = ctx.shared_warps_peaks_raw(pf, pt, po, rc0, [t16], [S_ONE], [(0, 1, 0, *WIDE)], cap_cells=4, fill=FILL)
    assert _untouched(rc, out, n) == F.E_UNSUPPORTED
    # ... as b the same recording is plain, and fine
    rc, out, n = ctx.shared_warps_peaks_raw(pf, pt, po, rc0, [t16], [S_ONE], [(1, 0, 0, *WIDE)], cap_cells=4, fill=FILL)
    assert (rc, n) == (F.OK, 0)


def test_a_window_per_job_inside_one_wave(S, ctx):
    """70 jobs of one item each, their windows alternating: one wave and one 64-thread block hold jobs with different windows"""
    couple = lambda t: [(100, t), (200, t + 3)]                                  # noqa: E731  one hash (100, 200, 3) at t
    a0, a1, a2 = couple(500), couple(0), couple(T_MAX - 3)
    b = [p for t in (0, 300, 500, 505, 800, 1100, T_MAX - 303, T_MAX - 3) for p in couple(t)]
    windows = [(-100, 10), (0, 0), (5, 5), (300, 600), (-500, -200), (-T_MAX, T_MAX), (6, 299), (T_MAX - 600, T_MAX), (-3, 4)]
    jobs = [(0, 3, 0, *windows[j % len(windows)]) for j in range(70)]
    want = _recs(S, ctx, [a0, a1, a2, b], [S_ONE], [S_ONE], jobs, max_run=8)
    assert want["job_pairs"][:9] == [2, 1, 1, 2, 2, 8, 0, 1, 1] and want["job_pairs"][9:18] == want["job_pairs"][:9]
    # windows cut at 0 (a at frame 0, negative lags) and at 2^20 - 1 (a at the last frames, positive lags)
    jobs = [(1, 3, 0, -500, 300), (1, 3, 0, -T_MAX, -1), (2, 3, 0, -300, 500), (2, 3, 0, 1, T_MAX), (1, 3, 0, 301, 499), (2, 3, 0, 0, 0)]
    want = _recs(S, ctx, [a0, a1, a2, b], [S_ONE], [S_ONE], jobs, max_run=8)
    assert want["job_pairs"] == [2, 0, 2, 0, 0, 1]


def test_jobs(S, ctx):
    rng = np.random.default_rng(4)
    t16, f16 = [S_ONE, 70000, 60000], [S_ONE, 62000, 70000]
    a = _cloud(rng, 200, 150, 200, 260)
    b = _cloud(rng, 150, 150, 200, 260)
    r1 = _warped(a, t16[1], f16[1], 20) + [(f, t + 400) for f, t in _cloud(rng, 40, 150, 200, 260)]
    r2 = _warped(b, t16[2], f16[2], 30) + _warped(a, t16[1], f16[1], 300)
    recs = [a, r1, r2, [], b, [(1500, 7)]]                                       # 3: empty; 5: one peak, no hash
    jobs = [(3, 0, 1, *WIDE),                                                    # no item at the head
            (0, 1, 1, *WIDE), (0, 2, 1, *WIDE), (0, 4, 1, *WIDE),                # one (a, v) against three b
            (5, 1, 0, *WIDE),                                                    # no item in the middle
            (1, 0, 1, *WIDE), (0, 1, 1, *WIDE),                                  # (b, a, v); a job twice
            (4, 2, 2, *WIDE), (4, 2, 0, 4000, 5000),                             # pairs, then none (the window misses)
            (0, 3, 2, *WIDE), (3, 3, 2, 1, 50)]                                  # no pair at the end: b empty; a == b, empty
    want = _recs(S, ctx, recs, t16, f16, jobs, max_run=32, cell_shift=3)
    at = want["cell_off"]
    assert want["job_pairs"][1] > 200 and want["job_pairs"][2] > 200 and want["job_pairs"][7] > 150
    assert [want["job_pairs"][j] for j in (0, 4, 8, 9, 10)] == [0] * 5 and want["job_hashes"][0] == 0
    assert [want[k][at[1]:at[2]] for k in twin.CELL_KEYS] == [want[k][at[6]:at[7]] for k in twin.CELL_KEYS]
    assert want["job_hashes"][1] == want["job_hashes"][2] == want["job_hashes"][3] == want["job_hashes"][6]
    # no jobs: rec_hashes all the same; no peaks at all; no recordings
    want = _recs(S, ctx, recs, t16, f16, [])
    assert want["cell_off"] == [0] and want["rec_hashes"][3] == 0 and want["rec_hashes"][0] > 300
    want = _check(S, ctx, [], [], [0, 0, 0], [0, 1, 2], t16, f16, [(0, 1, 1, *WIDE), (1, 1, 2, 1, 9)])
    assert want["cell_off"] == [0, 0, 0] and want["rec_hashes"] == [0, 0] and want["job_hashes"] == [0, 0]
    _check(S, ctx, [], [], [0], [0], t16, f16, [])


def test_self_jobs(S, ctx):
    """(a, a) at unity with [min_lag, max_lag]: the cells of shz_repeats_hashes on the same hashes; at another warp, with both
    signed windows: the twin"""
    rng = np.random.default_rng(5)
    p = _cloud(rng, 120, 60, 300, 360)
    a = p + [(f, t + 83) for f, t in p] + [(f, t + 190) for f, t in p[:70]] + _cloud(rng, 40, 260, 300, 360)
    pf, pt, po, rc0 = _lists([a, _cloud(rng, 50, 100, 300, 360)])
    k, t1, ho = ctx.warp_pair_hash_tf(pf, pt, po, [S_ONE], [S_ONE])
    for lo, hi in ((1, T_MAX), (80, 110), (83, 83)):
        want = _check(S, ctx, pf, pt, po, rc0, [S_ONE], [S_ONE], [(0, 0, 0, lo, hi), (1, 1, 0, lo, hi)], max_run=16, cell_shift=3)
        rep = ctx.repeats_hashes(k, t1, ho, rc0, lo, hi, 16, 3, 1)
        assert len(want["lag"]) >= 6
        for key in ("cell_off",) + twin.CELL_KEYS:                               # (the skip counters are defined differently)
            assert [int(x) for x in rep[key]] == want[key], (key, lo, hi)
    # the content once more at tempo 1.25 and pitch 0.9, 400 frames on: the warped repeat, seen from either airing
    t16, f16 = 81920, 58982
    inv = _warped(p, t16, f16, 400)
    pf, pt, po, rc0 = _lists([a + inv])
    want = _check(S, ctx, pf, pt, po, rc0, [t16, S_ONE], [f16, S_ONE], [(0, 0, 0, 1, T_MAX), (0, 0, 0, -T_MAX, -1), (0, 0, 0, 395, 405)],
                  max_run=16, cell_shift=3)
    at = want["cell_off"]
    assert 400 in want["lag"][at[0]:at[1]] and want["job_pairs"][2] > 100 and all(g < 0 for g in want["lag"][at[1]:at[2]])


def test_runs_of_exactly_max_run_and_one_more_on_either_side(S, ctx):
    """key (100, 200, 6): a holds it at dt = 3, tempo 2 makes it 6; b holds it as it is.  The couples lie 300 frames apart, so
    they pair with nothing else"""
    a_run = lambda m, f1=100: [p for i in range(m) for p in ((f1, 300 * i), (f1 + 100, 300 * i + 3))]    # noqa: E731
    b_run = lambda m, f1=100: [p for i in range(m) for p in ((f1, 600 * i + 50), (f1 + 100, 600 * i + 56))]  # noqa: E731
    for max_run in (2, 5):
        for m_a, m_b, pairs, skipped in ((max_run, max_run, max_run * max_run, 0), (max_run + 1, 1, 0, 1), (1, max_run + 1, 0, 1),
                                         (max_run + 1, max_run + 1, 0, 1)):
            # a second key (400, 500, 6), once on either side, is never skipped
            a, b = a_run(m_a) + [(400, 9000), (500, 9003)], b_run(m_b) + [(400, 20000), (500, 20006)]
            want = _recs(S, ctx, [a, b], [131072], [S_ONE], [(0, 1, 0, *WIDE)], max_run=max_run)
            assert want["job_pairs"] == [pairs + 1] and want["job_skipped_keys"] == [skipped]
            assert want["job_skipped_rows"] == [skipped * (m_a + m_b)]


def test_the_limit_on_virtual_recordings(S, ctx):
    """4,090 recordings and 6 distinct (a, v) fill the 12-bit recording field, 7 do not fit"""
    F = S._ffi
    rng = np.random.default_rng(6)
    a = _cloud(rng, 60, 40, 100, 130)
    recs = [a, _warped(a, 70000, S_ONE, 3), _warped(a, S_ONE, 60000, 2)] + [[(5, 5)]] * 4087
    pf, pt, po, rc0 = _lists(recs)
    t16, f16 = [70000, S_ONE, 66000], [S_ONE, 60000, 66000]
    six = [(0, 1, 0, *WIDE), (0, 2, 1, *WIDE), (1, 0, 2, *WIDE), (4000, 0, 0, *WIDE), (4089, 0, 1, *WIDE), (2, 0, 0, *WIDE),
           (0, 2, 0, *WIDE)]                                                     # (the last: (0, warp 0) again)
    want = twin.cells(pf, pt, po, rc0, t16, f16, six, 64, 5, 1)
    assert want["job_pairs"][0] > 50 and want["job_pairs"][1] > 50
    for got in _both(S, ctx, lambda: ctx.shared_warps_peaks(pf, pt, po, rc0, t16, f16, six, 64, 5, 1)):
        _same(got, want)
    rc, out, n = ctx.shared_warps_peaks_raw(pf, pt, po, rc0, t16, f16, six + [(3, 0, 2, *WIDE)], cap_cells=4, fill=FILL)
    assert _untouched(rc, out, n) == F.E_UNSUPPORTED
    assert b"4090 recordings and 7 distinct" in F.lib().shz_last_error(ctx.h)


def _untouched(rc, out, n):
    assert n == FILL and all(int(x) == FILL for a in out.values() for x in a)
    return rc


def test_refusals_leave_the_outputs_untouched(S, ctx):
    F = S._ffi
    base = dict(pf=[100, 200, 100, 200], pt=[5, 8, 50, 53], po=[0, 2, 4], rc0=[0, 1, 2], t16=[S_ONE, 70000], f16=[S_ONE, 60000],
                jobs=((0, 1, 1, -100, 100),), max_run=64, cell_shift=5, min_cell_pairs=1, fan_value=5, flags=0)

    def raw(**kw):
        p = dict(base, **kw)
        return _untouched(*ctx.shared_warps_peaks_raw(p["pf"], p["pt"], p["po"], p["rc0"], p["t16"], p["f16"], p["jobs"], p["max_run"],
                                                      p["cell_shift"], p["min_cell_pairs"], p["fan_value"], p["flags"], cap_cells=4,
                                                      fill=FILL))
    job = lambda **kw: (tuple(dict(dict(a=0, b=1, v=1, lo=-100, hi=100), **kw)[k] for k in ("a", "b", "v", "lo", "hi")),)   # noqa: E731
    assert raw(rc0=[1, 1, 2]) == F.E_INVALID and raw(rc0=[0, 2, 1]) == F.E_INVALID and raw(rc0=[0, 1, 1]) == F.E_INVALID
    assert raw(po=[1, 2, 4]) == F.E_INVALID and raw(po=[0, 3, 2]) == F.E_INVALID
    assert raw(max_run=1) == F.E_INVALID and raw(max_run=1025) == F.E_INVALID and raw(cell_shift=20) == F.E_INVALID
    assert raw(min_cell_pairs=0) == F.E_INVALID and raw(flags=1) == F.E_INVALID
    assert raw(fan_value=0) == F.E_INVALID and raw(fan_value=65) == F.E_INVALID
    # the table
    assert raw(t16=[], f16=[], jobs=()) == F.E_INVALID                           # no warp
    assert raw(t16=[S_ONE] * 1025, f16=[S_ONE] * 1025) == F.E_INVALID            # 1,025 warps
    assert raw(t16=[S_ONE, 32767]) == F.E_INVALID and raw(t16=[S_ONE, 131073]) == F.E_INVALID
    assert raw(f16=[S_ONE, 32767]) == F.E_INVALID and raw(f16=[131073, S_ONE]) == F.E_INVALID
    # the jobs
    assert raw(jobs=job(v=2)) == F.E_INVALID                                     # a warp that is not there
    assert raw(jobs=job(a=2)) == F.E_INVALID and raw(jobs=job(b=2)) == F.E_INVALID
    assert raw(jobs=job(lo=101)) == F.E_INVALID                                  # inverted
    assert raw(jobs=job(hi=1 << 20)) == F.E_INVALID and raw(jobs=job(lo=-(1 << 20))) == F.E_INVALID
    assert raw(jobs=job() + job(lo=-(1 << 31), hi=(1 << 31) - 1)) == F.E_INVALID
    assert b"job 1" in F.lib().shz_last_error(ctx.h)                                         # the message names the job
    assert raw(jobs=job() * 4097) == F.E_UNSUPPORTED
    # the peaks
    assert raw(pt=[5, 8, 50, 1 << 20]) == F.E_INVALID                            # a time beyond 20 bits
    assert raw(pt=[5, 8, 53, 50]) == F.E_INVALID                                 # time decreases inside a clip
    assert raw(pf=[100, 200, 200, 100], pt=[5, 8, 50, 50]) == F.E_INVALID        # one frame, f descending
    assert raw(pf=[100, 2049, 100, 200]) == F.E_INVALID                          # a bin the spectrogram lacks
    assert raw(po=[0] * 4098, rc0=list(range(4098)), pf=[], pt=[]) == F.E_UNSUPPORTED             # 4,097 recordings
    assert raw(pf=[], pt=[], po=[0, 0, 0], rc0=[0], jobs=()) == F.E_INVALID      # clips that belong to no recording
    # the bounds themselves are fine: 1,024 warps, 4,096 jobs, a == b, time decreasing ACROSS clips, equal peaks
    rc, out, n = ctx.shared_warps_peaks_raw(base["pf"], base["pt"], base["po"], base["rc0"], [S_ONE] * 1023 + [70000],
                                            [S_ONE] * 1023 + [60000], [(0, 1, 1023, *WIDE)] * 4096, 1024, 19, 1, cap_cells=16)
    assert (rc, n) == (F.OK, 0) and [int(x) for x in out["job_hashes"]] == [1] * 4096
    rc, _, n = ctx.shared_warps_peaks_raw([100, 200, 200, 100, 200], [50, 53, 53, 5, 8], [0, 3, 5], [0, 1, 2], [S_ONE], [S_ONE],
                                          [(0, 1, 0, *WIDE), (1, 1, 0, 1, 9)], 64, 5, 1, cap_cells=4)
    assert (rc, n) == (F.OK, 1)
    # NULL handles and arrays, straight at the ABI
    L = F.lib()
    u32, i32 = np.uint32, np.int32
    a = {n_: np.asarray(v, d) for n_, v, d in (("pf", base["pf"], np.uint16), ("pt", base["pt"], u32), ("po", base["po"], np.uint64),
                                               ("rc0", base["rc0"], u32), ("t16", base["t16"], u32), ("f16", base["f16"], u32),
                                               ("ja", [0], u32), ("jb", [1], u32), ("jv", [1], u32), ("lo", [-9], i32), ("hi", [9], i32))}
    # cell_off | lag block pairs first last | rec_hashes | job_hashes | job_pairs | job_skipped_keys | job_skipped_rows
    outs = [np.full(4, FILL, d) for d in (np.uint64, *[u32] * 7, np.uint64, u32, np.uint64)]
    cnt = C.c_uint64(FILL)

    def call(h=ctx.h, out=outs, count=C.byref(cnt), cap=4, **kw):
        p = {k: F.ptr(v) for k, v in a.items()}
        p.update(kw)
        return L.shz_shared_warps_peaks(h, p["pf"], p["pt"], p["po"], 2, p["rc0"], 2, 5, p["t16"], p["f16"], 2, p["ja"], p["jb"], p["jv"],
                                        p["lo"], p["hi"], 1, 64, 5, 1, 0, *[F.ptr(o) for o in out], cap, count)
    assert call(h=None) == F.E_INVALID and call(count=None) == F.E_INVALID
    for name in a:                                                               # every input array, the five job arrays among them
        assert call(**{name: None}) == F.E_INVALID, name
    for i in (0, 1, 6, 7, 8, 10):                                                # cell_off, a cell array, rec_hashes, job_* arrays
        assert call(out=outs[:i] + [None] + outs[i + 1:]) == F.E_INVALID
    assert cnt.value == FILL and all(int(x) == FILL for o in outs for x in o)
    # the fused call: its own refusals, before anything is extracted
    pcm = np.zeros(16384, np.int16)

    def fused(off=(0, 8192, 16384), rc0=(0, 1, 2), jobs=job(), fan_value=5, t16=(S_ONE, 70000), f16=(S_ONE, 60000), **kw):
        p = dict(max_run=64, cell_shift=5, min_cell_pairs=1)
        p.update(kw)
        rc, out, n, ms = ctx.shared_warps_batch_raw(pcm, list(off), list(rc0), list(t16), list(f16), jobs, fan_value=fan_value,
                                                    cap_cells=4, fill=FILL, **p)
        assert ms == (float(np.float32(FILL)),) * 4                              # the four times too
        return _untouched(rc, out, n)
    assert fused(fan_value=0) == F.E_INVALID and fused(max_run=1025) == F.E_INVALID and fused(cell_shift=20) == F.E_INVALID
    assert fused(min_cell_pairs=0) == F.E_INVALID and fused(jobs=job(lo=200)) == F.E_INVALID and fused(jobs=job(v=2)) == F.E_INVALID
    assert fused(jobs=job(a=2)) == F.E_INVALID and fused(t16=(S_ONE, 131073)) == F.E_INVALID
    assert fused(rc0=(1, 1, 2)) == F.E_INVALID and fused(off=(0, 8192, 4096)) == F.E_INVALID
    # a clip of a too long for its tempo: (frames - 1) * 2 reaches 2^20 -- refused from the lengths alone, nothing is read
    long_off = (0, (1 << 19) * HOP + 4096, (1 << 19) * HOP + 8192)
    assert fused(off=long_off, jobs=job(v=1), t16=(S_ONE, 131072)) == F.E_UNSUPPORTED
    # silence: recordings without peaks
    rc, out, n, _ = ctx.shared_warps_batch_raw(pcm, [0, 8192, 16384], [0, 1, 2], [S_ONE, 70000], [S_ONE, 60000], job(), cap_cells=4)
    assert (rc, n) == (F.OK, 0) and [int(x) for x in out["cell_off"]] == [0, 0] and [int(x) for x in out["rec_hashes"]] == [0, 0]


def test_capacity_and_the_two_call_idiom(S, ctx):
    F = S._ffi
    rng = np.random.default_rng(7)
    a = _cloud(rng, 200, 100, 100, 140)
    t16, f16 = [72000, S_ONE], [S_ONE, S_ONE]
    args = (*_lists([a, _warped(a, 72000, S_ONE, 6), a[20:150]]), t16, f16, [(0, 1, 0, *WIDE), (0, 2, 1, -50, 50), (2, 0, 1, *WIDE)], 16, 2, 2)
    want = twin.cells(*args)
    need = len(want["lag"])
    assert need > 8
    for cap in (0, need - 1):
        rc, out, n = ctx.shared_warps_peaks_raw(*args, cap_cells=cap, fill=FILL)
        assert (rc, n) == (F.E_CAPACITY, need)
        for key in ("cell_off", "rec_hashes", "job_hashes", "job_pairs", "job_skipped_keys", "job_skipped_rows"):
            assert _ints(out, key) == want[key]
        for key in twin.CELL_KEYS:
            assert _ints(out, key) == want[key][:cap]
    rc, out, n = ctx.shared_warps_peaks_raw(*args, cap_cells=need, fill=FILL)
    assert (rc, n) == (F.OK, need)
    _same(out, want)
    _same(ctx.shared_warps_peaks(*args), want)                                   # (the two calls)


def test_fuzz(S, ctx):
    rng = np.random.default_rng(8)
    for case in range(240):
        n_recs = int(rng.integers(2, 6))
        pf, pt, po, rc0 = [], [], [0], [0]
        for _ in range(n_recs):
            for _ in range(int(rng.integers(1, 3))):
                peaks = sorted(_cloud(rng, int(rng.integers(0, 61)), int(rng.integers(4, 40)), 20, 20 + int(rng.integers(2, 9))),
                               key=lambda p: (p[1], p[0]))
                pf += [p[0] for p in peaks]
                pt += [p[1] for p in peaks]
                po.append(len(pf))
            rc0.append(len(po) - 1)
        n_warps = int(rng.integers(1, 5))
        t16 = [int(x) for x in rng.integers(32768, 131073, n_warps)]
        f16 = [int(x) for x in rng.integers(32768, 131073, n_warps)]
        if case % 3 == 0:
            t16[0] = f16[0] = S_ONE
        jobs = []
        for _ in range(int(rng.integers(1, 13))):
            lo, hi = sorted(int(x) for x in rng.integers(-45, 46, 2))
            if rng.integers(0, 4) == 0:
                lo, hi = WIDE
            jobs.append((int(rng.integers(0, n_recs)), int(rng.integers(0, n_recs)), int(rng.integers(0, n_warps)), lo, hi))
        _check(S, ctx, pf, pt, po, rc0, t16, f16, jobs, max_run=int(rng.integers(2, 9)), cell_shift=int(rng.integers(0, 7)),
               min_cell_pairs=int(rng.integers(1, 3)))


# ---- the fixture ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(S, ctx):
    """the two recordings, the GPU's peaks of them, and the twin's whole answer on those peaks"""
    recs = K.recordings()
    off = np.zeros(3, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    pcm = np.concatenate(recs)
    pf, pt, po = ctx.peaks(pcm, off)
    cells = K.twin_cells(pf, pt, [int(x) for x in po], K.table_jobs())
    return dict(recs=recs, pcm=pcm, off=off, pf=pf, pt=pt, po=[int(x) for x in po], cells=cells, reps=K.twin_fold(cells))


@pytest.fixture(scope="module")
def found(S, ctx, fx):
    return S.find_shared(fx["recs"], pairs=[(1, 0)], warps=(np.asarray(K.T16, np.uint32), np.asarray(K.F16, np.uint32)), Fs=SR, ctx=ctx)


def test_batch_equals_peaks_equals_the_twin_on_the_gpus_peaks(S, ctx, fx):
    jobs, want = K.table_jobs(), fx["cells"]
    assert min(want["job_pairs"][:3]) > 400

    def run():
        _same(ctx.shared_warps_peaks(fx["pf"], fx["pt"], fx["po"], [0, 1, 2], K.T16, K.F16, jobs, **K.DEFAULTS), want, "peaks")
        got, ms = ctx.shared_warps_batch(fx["pcm"], fx["off"], [0, 1, 2], K.T16, K.F16, jobs, **K.DEFAULTS)
        _same(got, want, "host pcm")
        assert all(m > 0 for m in ms)
        buf = ctx.alloc(fx["pcm"].nbytes)
        try:
            buf.upload(fx["pcm"])
            got, _ = ctx.shared_warps_batch(buf, fx["off"], [0, 1, 2], K.T16, K.F16, jobs, pcm_device=True, cap_cells=len(want["lag"]),
                                            **K.DEFAULTS)
            _same(got, want, "device pcm")
        finally:
            buf.free()
    _both(S, ctx, run)


def test_the_ladder_finds_what_the_plain_join_cannot_see(S, ctx, fx, found):
    """THE test of the feature: the plain join sees the unchanged piece alone; at the ladder the piece sped up 1.03 and the piece
    at tempo 1.04 and pitch 0.97 are there, each at its rung, and the unchanged one stays plain"""
    from shazam_amd.extent import own_frames
    plain = S.find_shared(fx["recs"], pairs=[(1, 0)], Fs=SR, ctx=ctx)
    assert len(plain) == 1 and 270 <= plain[0]["first"] <= plain[0]["last"] <= 410
    for p in found:
        print(p["warp"], p["tempo"], p["pitch"], p["first"], p["last"], p["a_first"], p["a_last"], p["b_first"], p["b_last"], p["lag"],
              p["lag_lo"], p["lag_hi"], p["pairs"], p["tempo_fit"], p["candidates"])
    assert [(p["warp"], p["tempo"], p["pitch"]) for p in found] == [(1, K.T16[1] / 65536, K.F16[1] / 65536), (0, 1.0, 1.0),
                                                                     (2, K.T16[2] / 65536, K.F16[2] / 65536)]
    x, y, z = found
    assert (y["first"], y["last"], y["lag"], y["pairs"]) == tuple(plain[0][k] for k in ("first", "last", "lag", "pairs"))
    assert "speed" in x and "speed" in y and "speed" not in z
    # what the twin and the plain-Python fold give on the GPU's peaks, stretch for stretch; the candidates as the table lists them
    by_warp = {r["rec"]: r for r in fx["reps"]}
    assert sorted(by_warp) == [0, 1, 2, 5, 6, 7]
    for p in found:
        w = by_warp[p["warp"]]
        assert tuple(p[k] for k in ("first", "last", "lag", "lag_lo", "lag_hi", "pairs", "cells")) == \
            tuple(w[k] for k in ("first", "last", "lag", "lag_lo", "lag_hi", "pairs", "cells"))
        sc = K.stretch_cells(fx["cells"], w)
        assert (p["b_first"], p["b_last"]) == (min(f + g for g, f, _, _ in sc), max(l + g for g, _, l, _ in sc))
        assert (p["a_first"], p["a_last"]) == own_frames(w["first"], w["last"], K.T16[p["warp"]])
        assert p["stats"]["hashes_a"] == fx["cells"]["job_hashes"][p["warp"]] and p["stats"]["hashes_b"] == fx["cells"]["rec_hashes"][0]
    cand = lambda v: (v, by_warp[v]["pairs"], by_warp[v]["lag_lo"], by_warp[v]["lag_hi"])                 # noqa: E731
    assert x["candidates"] == [] and y["candidates"] == [cand(7)] and z["candidates"] == [cand(5), cand(6)]
    assert abs(x["tempo_fit"] - 1.03) <= 0.003 and abs(z["tempo_fit"] - 1.04) <= 0.003 and abs(y["tempo_fit"] - 1.0) <= 0.003
    # X in recording 1's own time: inside the planted span widened by a frame on either side, covering 0.9 of its whole frames
    frames = lambda sec: sec * SR / HOP                                          # noqa: E731
    start, end = K.X_START, K.X_START + K.X_SECONDS
    whole = int((end - start) * SR - 4096) // HOP + 1
    assert math.floor(frames(start)) - 1 <= x["a_first"] <= x["a_last"] <= frames(end) + 1
    print("   cover", x["a_last"] - x["a_first"] + 1, "of", whole)
    assert x["a_last"] - x["a_first"] + 1 >= 0.9 * whole
    secs = lambda f: round(f * HOP / SR, 5)                                      # noqa: E731
    assert (x["a_start_seconds"], x["a_end_seconds"]) == (secs(x["a_first"]), secs(x["a_last"] + 1))
    assert (x["b_start_seconds"], x["b_end_seconds"]) == (secs(x["b_first"]), secs(x["b_last"] + 1))
    # X lies at 3 s of recording 0, 8 s long
    assert math.floor(frames(3)) - 1 <= x["b_first"] <= x["b_last"] <= frames(11) + 1


def test_find_shared_peaks_and_occurrences(S, ctx, fx, found):
    warps = (np.asarray(K.T16, np.uint32), np.asarray(K.F16, np.uint32))
    assert S.find_shared_peaks(fx["pf"], fx["pt"], fx["po"], pairs=[(1, 0)], warps=warps, Fs=SR, ctx=ctx) == found
    groups = S.shared_occurrences(found)
    assert [g["airings"] for g in groups] == sorted([[(0, p["b_first"], p["b_last"]), (1, p["a_first"], p["a_last"])] for p in found])


def test_self_pairs(S, ctx, fx):
    s103 = [K.q16(1.03)]
    # no warped repeat is planted in recording 1
    assert S.find_shared(fx["recs"], pairs=[(1, 1)], speeds=s103, Fs=SR, ctx=ctx) == []
    # X at 2 s and X sped up 1.03 at 13 s: the later airing, played 1.03 times as fast as the earlier one
    rec = K.self_recording()
    got = S.find_shared([rec], pairs=[(0, 0)], speeds=s103, Fs=SR, ctx=ctx)
    for p in got:
        print(p["warp"], p["first"], p["last"], p["a_first"], p["a_last"], p["b_first"], p["b_last"], p["lag"], p["pairs"], p["tempo_fit"])
    assert len(got) == 1
    p, = got
    frames = lambda sec: sec * SR / HOP                                          # noqa: E731
    assert (p["warp"], p["rec_a"], p["rec_b"], p["job"]) == (0, 0, 0, 0) and p["lag"] < 0
    assert frames(13) - 1 <= p["a_first"] <= p["a_last"] <= frames(13 + 8 / 1.03) + 1
    assert frames(2) - 1 <= p["b_first"] <= p["b_last"] <= frames(10) + 1
    assert abs(p["tempo_fit"] - 1.03) <= 0.003


def test_resample_to_goes_through_the_device_resampler(S, ctx, fx):
    """find_shared(resample_to=) at a ladder: the recordings, taken as 48 kHz audio, are resampled on the device; the stretches are
    those of the peaks Context.peaks gives for the same resampled audio"""
    warps = (np.asarray(K.T16[:3], np.uint32), np.asarray(K.F16[:3], np.uint32))
    got = S.find_shared(fx["recs"], pairs=[(1, 0)], warps=warps, Fs=48000, resample_to=SR, ctx=ctx)
    buf, off = S.resample_to_device(fx["recs"], 48000, SR, ctx)
    try:
        pf, pt, po = ctx.peaks(buf, off, pcm_device=True)
    finally:
        buf.free()
    assert got == S.find_shared_peaks(pf, pt, po, pairs=[(1, 0)], warps=warps, Fs=SR, ctx=ctx)
    print([(p["warp"], p["first"], p["last"], p["lag"], p["pairs"]) for p in got])
    assert 0 in [p["warp"] for p in got]                                         # the unchanged piece, at the least


def test_more_jobs_than_a_call_holds_are_split(S, ctx, fx, found, monkeypatch):
    warps = (np.asarray(K.T16, np.uint32), np.asarray(K.F16, np.uint32))
    for name, most in (("MAX_JOBS", 3), ("MAX_WARPS", 2), ("MAX_RECS", 4), ("MAX_JOBS", 1)):
        with monkeypatch.context() as m:
            m.setattr(S.shared, name, most)
            assert S.find_shared(fx["recs"], pairs=[(1, 0)], warps=warps, Fs=SR, ctx=ctx) == found, (name, most)
