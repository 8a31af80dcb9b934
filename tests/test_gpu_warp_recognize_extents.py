"""GPU: Context.recognize_warps(..., extents=True) (shz_recognize_warps_extents) -- the extent pass and the moments on the
hashes of every query's best variant, which exist on the device only -- against the plain-Python definitions
(tests/extent_twin.py, tests/fit_twin.py) on the CPU pipeline's hashes of that variant: the oracle's peaks through the numpy
twin of the two-factor warp (tests/warp_twin.py).  The songs, the queries and the table are those of
tests/test_gpu_warp_recognize.py; the pair list is small: tempo rungs 65536 + 2753 k, k in -1 .. 1, x the pitch rungs within
one 92-step of a true pitch or of 65536 -- 3 x 9 = 27 pairs.  The true tempos 1.04, 0.95, 1.03 lie 0.2 %, 0.8 % and 1.2 % off
their nearest rungs.

The fitted tempo, the rung and the true tempo of every query are printed (run with -s); their distance is not asserted."""
import numpy as np
import pytest

import warp_twin as W
from extent_twin import SCALARS, assert_extents, expected_extents
from fit_twin import SUMS, assert_moments, expected_moments, warp_map
from test_gpu_warp_recognize import SILENT, SONG, TOPN, TRUE, S, ctx, db, peaks, queries, songs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

T_STEP, F_STEP = 2753, 92
REC = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "best", "profile")
EXT = SCALARS + SUMS + ("hist", "shift")


@pytest.fixture(scope="module")
def pairs(S):
    tl = np.asarray([65536 + T_STEP * k for k in (-1, 0, 1)], np.uint32)
    ks = set()
    for p in sorted({p for _, p in TRUE} | {1.0}):
        mid = int(round((W.q16(p) - 65536) / F_STEP))
        ks |= {mid - 1, mid, mid + 1}
    pl = np.asarray([65536 + F_STEP * k for k in sorted(ks)], np.uint32)
    assert len(pl) == 9
    return S.warp_grid(tl, pl)


def _pcm(S, queries):
    chans, first = [], [0]
    for q in queries:
        cs = [q] if isinstance(q, np.ndarray) else list(q)
        chans.extend(S._as_pcm(c) for c in cs)
        first.append(len(chans))
    off = np.zeros(len(chans) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chans])
    return np.concatenate(chans), off, np.asarray(first, np.uint32)


@pytest.fixture(scope="module")
def runs(S, ctx, db, queries, pairs):
    """the plain call, and the call with extents at drift_bins 0 and 5 and under both small switches at 5"""
    from shazam_amd import _ffi
    pcm, off, first = _pcm(S, queries)
    assert ctx.vote_tolerance == 0
    out = {"plain": ctx.recognize_warps(db[0].table, pcm, off, first, *pairs, topn=TOPN)[0]}
    for drift in (0, 5):
        out[drift], ms = ctx.recognize_warps(db[0].table, pcm, off, first, *pairs, topn=TOPN, extents=True, drift_bins=drift)
        assert len(ms) == 4
    ctx.set_debug(_ffi.DEBUG_SPEED_SMALL_SLICES | _ffi.DEBUG_EXTENT_SMALL_TILES)     # 7 queries: slices of 2, sub-batches of 3
    try:
        out["small"], _ = ctx.recognize_warps(db[0].table, pcm, off, first, *pairs, topn=TOPN, extents=True, drift_bins=5)
    finally:
        ctx.set_debug(0)
    return out


def test_the_recognition_outputs_are_those_of_recognize_warps(runs):
    for run in (0, 5, "small"):
        for name in REC:
            assert np.array_equal(runs[run][name], runs["plain"][name]), (run, name)
    assert runs["plain"]["nres"][:5].min() >= 1 and int(runs["plain"]["nres"][SILENT]) == 0


def _assert_equals_the_twins(db, peaks, pairs, res, w, what):
    """the extent arrays of res against the twins on the CPU pipeline's hashes of every query's best variant, candidates
    (sid, delta - w, delta + w) from res"""
    drift = w
    tk, ts, to = db[0].table.export()
    for q, chans in enumerate(peaks):
        b = int(res["best"][q])
        hk = [W.warp_pair_tf(f, t, int(pairs[0][b]), int(pairs[1][b])) for f, t in chans]
        qk, qo = np.concatenate([k for k, _ in hk]), np.concatenate([t for _, t in hk])
        n = int(res["nres"][q])
        sid = [[int(res["sid"][q, c]) for c in range(TOPN)]]
        lo = [[int(res["delta"][q, c]) - drift for c in range(TOPN)]]
        hi = [[int(res["delta"][q, c]) + drift for c in range(TOPN)]]
        args = (tk, ts, to, qk, qo, np.asarray([0, len(qk)], np.uint64), sid, lo, hi, [n])
        one = {k: res[k][q:q + 1] for k in EXT}
        assert_extents(one, expected_extents(*args), ("extents", what, q))
        assert_moments(one, expected_moments(*args), ("sums", what, q))


@pytest.mark.parametrize("drift", [0, 5])
def test_extents_and_sums_equal_the_twin_on_the_cpu_pipelines_hashes(db, peaks, pairs, runs, drift):
    _assert_equals_the_twins(db, peaks, pairs, runs[drift], drift, drift)


def test_the_vote_tolerance_widens_the_candidates(S, ctx, db, queries, peaks, pairs):
    """tolerance 2, drift_bins 1: w = 3, and the recognition outputs are those of the tolerant recognize_warps"""
    pcm, off, first = _pcm(S, queries)
    with ctx.tolerance(2):
        plain, _ = ctx.recognize_warps(db[0].table, pcm, off, first, *pairs, topn=TOPN)
        res, _ = ctx.recognize_warps(db[0].table, pcm, off, first, *pairs, topn=TOPN, extents=True, drift_bins=1)
    assert ctx.vote_tolerance == 0
    for name in REC:
        assert np.array_equal(res[name], plain[name]), name
    _assert_equals_the_twins(db, peaks, pairs, res, 3, "tolerance 2 + drift 1")
    assert (res["count"] >= res["aligned"]).all()


def test_a_diagonal_list_is_recognize_speeds_extents(S, ctx, db, queries):
    lad = np.asarray([62259, 65536 - 92, 65536, 65536 + 92, 68157, 68813], np.uint32)
    pcm, off, first = _pcm(S, queries)
    a, ms = ctx.recognize_speeds(db[0].table, pcm, off, first, lad, topn=TOPN, extents=True, drift_bins=2)
    b, _ = ctx.recognize_warps(db[0].table, pcm, off, first, lad, lad, topn=TOPN, extents=True, drift_bins=2)
    assert len(ms) == 4 and set(a) == set(b)
    for name in REC + EXT:
        assert np.array_equal(a[name], b[name]), name
    assert int(a["count"][0, 0]) >= int(a["aligned"][0, 0]) > 0
    results, tm = S.recognize_speeds(queries, db[0], speeds=lad, topn=TOPN, extents=True)
    assert results[SILENT] == [] and tm["drift_bins"] >= 1
    top = results[0][0]
    assert top["speed"] == float(lad[int(tm["speed_best"][0])]) / 65536 == 1.0 and top["fit"]["count"] >= 2
    t16 = int(lad[int(tm["speed_best"][0])])
    assert warp_map(top["query_first"], t16) >= top["warped_first"] and warp_map(top["query_last"], t16) <= top["warped_last"]


def test_the_separable_search_reports_the_second_stages_extents(S, db, queries, pairs):
    tl, pl = np.unique(pairs[0]), np.unique(pairs[1])
    plain, _ = S.recognize_warps(queries, db[0], tempos=tl, pitches=pl, topn=TOPN, search="separable")
    results, tm = S.recognize_warps(queries, db[0], tempos=tl, pitches=pl, topn=TOPN, search="separable", extents=True, drift_bins=5)
    assert tm["drift_bins"] == 5 and "stage1" in tm and results[SILENT] == []
    for q, dicts in enumerate(results):
        assert len(dicts) == len(plain[q])
        for d, p in zip(dicts, plain[q]):
            assert {k: d[k] for k in p} == p and d["fit"]["d_lo"] == d["offset"] - 5 and d["fit"]["count"] >= 1
            assert d["warped_first"] <= d["warped_last"] and d["query_first"] <= d["query_last"]


def test_48k_queries_go_through_resample_to(S, db, queries, pairs):
    import speed_twin as T
    qs = [T.speed_up(queries[1], 44100 / 48000), T.speed_up(queries[0], 44100 / 48000)]   # the same audio sampled at 48 kHz
    plain, _ = S.recognize_warps(qs, db[0], warps=pairs, Fs=48000, topn=TOPN, resample_to=44100)
    results, tm = S.recognize_warps(qs, db[0], warps=pairs, Fs=48000, topn=TOPN, resample_to=44100, extents=True)
    assert tm["drift_bins"] == 5                                                # (from the resampled lengths: 10 s)
    for dicts, p, sid in zip(results, plain, (SONG[1] + 1, SONG[0] + 1)):
        assert dicts and dicts[0]["song_id"] == sid and len(dicts) == len(p)
        for d, e in zip(dicts, p):
            assert {k: d[k] for k in e} == e and d["fit"]["d_lo"] == d["offset"] - 5
        top = dicts[0]
        assert isinstance(top["tempo_fit"], float) and top["query_first"] <= top["query_last"] < 216
        print(f"48 kHz: rung {top['tempo']:.5f}, tempo_fit {top['tempo_fit']:.5f}")


def test_refusals_of_the_fused_call(S, ctx, db, queries, pairs):
    from shazam_amd import _ffi
    pcm, off, first = _pcm(S, queries[:1])
    call = lambda **kw: ctx.recognize_warps(db[0].table, pcm, off, first, *pairs, extents=True, **kw)
    res, _ = call(topn=TOPN, drift_bins=2047)                                   # 2 w + 1 = 4,095 bins: the widest allowed
    assert int(res["count"][0, 0]) >= int(res["aligned"][0, 0]) > 0
    with pytest.raises(_ffi.ShzError):
        call(topn=TOPN, drift_bins=2048)                                        # 4,097 bins
    with ctx.tolerance(1):
        with pytest.raises(_ffi.ShzError):
            call(topn=TOPN, drift_bins=2047)                                    # the tolerance counts
    with pytest.raises(_ffi.ShzError):
        call(topn=65, drift_bins=0)


def test_count_is_aligned_at_tolerance_0_and_drift_0(runs):
    assert np.array_equal(runs[0]["count"], runs[0]["aligned"])
    assert np.array_equal(runs[0]["hist"].sum(axis=2), runs[0]["aligned"])
    assert (runs[5]["count"] >= runs[0]["count"]).all() and (runs[5]["count"] > runs[0]["count"]).any()


def test_small_slices_and_small_tiles_give_the_same(runs):
    for name in EXT:
        assert np.array_equal(runs["small"][name], runs[5][name]), name


def test_the_silent_query_is_all_zero(runs):
    for run in (0, 5, "small"):
        for name in EXT:
            assert not runs[run][name][SILENT].any(), (run, name)


def test_recognize_warps_extents_end_to_end(S, db, queries, pairs, runs):
    from shazam_amd.extent import line_fit, tempo_of
    plain, _ = S.recognize_warps(queries, db[0], warps=pairs, topn=TOPN)
    results, tm = S.recognize_warps(queries, db[0], warps=pairs, topn=TOPN, extents=True)
    # three distinct tempo rungs 2,753 apart (h = 1376.5), 10 s queries: t_max = 223 warped frames, ceil(223 * 1376.5 / 65536) = 5
    assert tm["drift_bins"] == 5 and tm["extent_time"] > 0
    keys = ("query_first", "query_last", "song_first", "song_last", "query_start_secs", "query_end_secs", "song_start_secs",
            "song_end_secs", "extent_hist", "extent_shift", "warped_first", "warped_last", "fit", "tempo_fit")
    truth = [a for a, _ in TRUE] + [None, 1.04]
    assert results[SILENT] == []
    for q, dicts in enumerate(results):
        assert len(dicts) == len(plain[q]) == int(runs[5]["nres"][q])
        for n, d in enumerate(dicts):
            assert all(k in d for k in keys) and {k: d[k] for k in plain[q][n]} == plain[q][n]
            t16 = int(round(d["tempo"] * 65536))
            wf, wl = d["warped_first"], d["warped_last"]
            assert (wf, wl, d["song_first"], d["song_last"]) == tuple(int(runs[5][k][q, n]) for k in SCALARS[1:])
            assert warp_map(d["query_first"], t16) >= wf and (d["query_first"] == 0 or warp_map(d["query_first"] - 1, t16) < wf)
            assert warp_map(d["query_last"], t16) <= wl < warp_map(d["query_last"] + 1, t16)
            fit = d["fit"]
            assert fit == {"count": int(runs[5]["count"][q, n]), **{f: int(runs[5][f][q, n]) for f in SUMS},
                           "d_lo": d["offset"] - 5}
            assert all(type(v) is int for v in fit.values())
            line = line_fit(**fit)
            assert d["tempo_fit"] == (None if line is None else float(tempo_of(t16, line[0])))
            assert np.array_equal(d["extent_hist"], runs[5]["hist"][q, n]) and d["extent_shift"] == int(runs[5]["shift"][q])
        if dicts:
            top = dicts[0]
            print(f"query {q}: true tempo {truth[q]}, rung {top['tempo']:.5f}, tempo_fit "
                  f"{'none' if top['tempo_fit'] is None else format(top['tempo_fit'], '.5f')} ({top['fit']['count']} pairs)")
