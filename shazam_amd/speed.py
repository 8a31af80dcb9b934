"""Speed-tolerant recognition: audio played slightly fast or slow (csrc/shz_speed.hip).

The reference's hash is an exact (f1, f2, dt) triple (recognizer.py:100-114): a query that plays 1 % faster than the table's
copy has already lost the match.  Here the query's constellation peaks are extracted ONCE; for every factor of a ladder their
integer coordinates are mapped back to the table's domain (f' = round(f / s), t' = round(t s)), paired, hashed and matched
on the device, and the factor with the most aligned hashes wins.  A variant costs no FFT.

A speed is one factor for both axes.  A time-stretch that keeps the pitch (a deck with key-lock), a pitch shift that keeps
the tempo, or both by different amounts are a WARP, a pair of Q16 factors (t16, f16): t' is formed with t16,
f' with f16.  recognize_warps matches a list of pairs -- the product of a tempo ladder and a pitch ladder (search="grid"), or
the pitch ladder at tempo 1 followed by the tempo ladder at every query's best pitch (search="separable", a heuristic).

Limits: the hop is fixed, so a warped time is a rounded frame; a peak near the edge of its 21x21 neighbourhood may move when
the audio is stretched; the smearing a real phase-vocoder time-stretch adds is not modelled by the corpus the tolerances were
measured on.  The scan (scan.py) and the device-resident listeners (stream.py) take speed ladders and warp pairs alike."""
from __future__ import annotations

from time import time

import numpy as np

from ._ffi import HOP, NFFT, takes_delta_tol

S_ONE = 65536              # the factor 1.0 in Q16
S_MIN, S_MAX = 32768, 131072
# Twice the factor mismatch at which the right song's aligned count has fallen to half of its value at the true factor:
# 0.07 % measured on the CPU (oracle + tests/speed_twin.py, music-like corpus, true speeds 0.95 .. 1.05), so
# a true speed is never further than that half-width from a rung.  In Q16: round(0.0014 * 65536).
DEFAULT_STEP_Q16 = 92


MAX_WARPS = 1024           # variants of one library call (SP_MAX_SPEEDS)
# The two axes of a warp (scripts/warp_curves.py: oracle + tests/warp_twin.py, note corpus, 4 x 30 s in the
# table, 10 s queries, 24 curves an axis).  Each step is twice the miss at which the mean aligned count of the right song
# has fallen to half of its value at the true pair.
#   pitch: half-width 0.06 % at any query length; step 0.12 % = round(0.0012 * 65536)
#   tempo: half-width 2.1 % on 10 s queries; step 4.2 % = round(0.042 * 65536).  A wrong tempo lets the offset drift over the
#          query, so the half-width scales inversely with the query's length (5.2 % at 5 s, 0.97 % at 20 s): queries much
#          longer than 10 s want a proportionally finer tempo step
DEFAULT_PITCH_STEP_Q16 = 79
DEFAULT_TEMPO_STEP_Q16 = 2753


def _ladder(name: str, lo: float, hi: float, st: int) -> np.ndarray:
    if st < 1:
        raise ValueError("step must be at least 1 / 65536")
    lo16, hi16 = int(np.ceil(float(lo) * S_ONE)), int(np.floor(float(hi) * S_ONE))
    if lo16 < S_MIN or hi16 > S_MAX or lo16 > hi16:
        raise ValueError(f"{name}: 0.5 <= lo <= hi <= 2.0")
    k_lo, k_hi = -((S_ONE - lo16) // st), (hi16 - S_ONE) // st      # ceil((lo16 - S_ONE) / st), floor((hi16 - S_ONE) / st)
    rungs = S_ONE + st * np.arange(k_lo, k_hi + 1, dtype=np.int64)
    return np.unique(np.concatenate([rungs, [S_ONE]])).astype(np.uint32)


def speed_ladder(lo: float = 0.95, hi: float = 1.05, step: float = None) -> np.ndarray:
    """The factors tried for a query of unknown speed, as Q16 (uint32, sorted, no duplicates): 65536 + k * step for every k
    that keeps the rung inside [lo, hi], and always 65536 itself.  step=None: the measured default, 92 / 65536 = 0.14 % --
    twice the half-width (0.07 %) of the tolerance curve in DESIGN.md 3.7c, at which the aligned count of the right song
    is half of what the true factor gives."""
    return _ladder("speed_ladder", lo, hi, DEFAULT_STEP_Q16 if step is None else int(round(float(step) * S_ONE)))


def tempo_ladder(lo: float = 0.95, hi: float = 1.05, step: float = None) -> np.ndarray:
    """The time factors tried for a query of unknown tempo, Q16 like speed_ladder's rungs (sorted, always with 65536).
    step=None: DEFAULT_TEMPO_STEP_Q16 / 65536, measured on 10 s queries."""
    return _ladder("tempo_ladder", lo, hi, DEFAULT_TEMPO_STEP_Q16 if step is None else int(round(float(step) * S_ONE)))


def pitch_ladder(lo: float = 0.95, hi: float = 1.05, step: float = None) -> np.ndarray:
    """The frequency factors tried for a query of unknown pitch, Q16 like speed_ladder's rungs (sorted, always with 65536).
    step=None: DEFAULT_PITCH_STEP_Q16 / 65536."""
    return _ladder("pitch_ladder", lo, hi, DEFAULT_PITCH_STEP_Q16 if step is None else int(round(float(step) * S_ONE)))


def warp_grid(tempos, pitches):
    """(tempo_q16, pitch_q16) of every pair of the two ladders, tempo-major: pair i * len(pitches) + j is (tempos[i],
    pitches[j]), so a row of the grid is one tempo at every pitch."""
    t, f = _check_speeds(tempos, "tempos"), _check_speeds(pitches, "pitches")
    return np.repeat(t, len(f)), np.tile(f, len(t))


def warp_chunks(n_pairs: int, row: int = 1, limit: int = MAX_WARPS):
    """[(a, b)]: the pair list [0, n_pairs) cut into library calls of at most `limit` pairs, each a whole number of rows of
    `row` pairs (a grid's row: one tempo at every pitch; an explicit pair list: rows of 1)."""
    if row < 1 or row > limit:
        raise ValueError(f"a row of {row} pairs does not fit one call of at most {limit}: shorten the pitch ladder")
    if n_pairs % row:
        raise ValueError("the pair list is no whole number of rows")
    per = (limit // row) * row
    return [(a, min(a + per, n_pairs)) for a in range(0, n_pairs, per)]


def _check_speeds(speeds, name: str = "speeds") -> np.ndarray:
    sp = np.ascontiguousarray(speeds)
    if sp.dtype.kind not in "iu" or sp.ndim != 1:
        raise TypeError(f"{name} are Q16 integers (round(s * 65536)); see speed_ladder")
    return sp.astype(np.uint32)


def warp_hashes(peaks_f, peaks_t, peak_off, speeds, fan_value: int = 5, ctx=None, query_clip0=None):
    """The hashes of every clip at every factor (shz_warp_pair_hash): peaks in (time asc, freq asc) order per clip, peak_off
    their CSR, speeds in Q16.  Returns (key32, t1, hash_off): for query q, for speed v, for every clip c of q the hashes of
    (c, v); hash_off has n_clips * n_speeds + 1 entries in that order.  query_clip0=None: every clip is its own query, so
    segment c * n_speeds + v is clip c at speed v.  t1 is in the table's frames."""
    from . import get_context
    return (ctx or get_context()).warp_pair_hash(peaks_f, peaks_t, peak_off, _check_speeds(speeds), query_clip0, int(fan_value))


def warp_hashes_tf(peaks_f, peaks_t, peak_off, tempos, pitches, fan_value: int = 5, ctx=None, query_clip0=None):
    """warp_hashes with a time and a frequency factor of its own for every variant (shz_warp_pair_hash_tf): warp v is
    (tempos[v], pitches[v]), Q16, two lists of one length (warp_grid makes them from two ladders).  Returns (key32, t1,
    hash_off) in the order query, warp, clip."""
    from . import get_context
    return (ctx or get_context()).warp_pair_hash_tf(peaks_f, peaks_t, peak_off, _check_speeds(tempos, "tempos"),
                                                    _check_speeds(pitches, "pitches"), query_clip0, int(fan_value))


def default_drift_bins(ctx, clip_samples, tempos, tol: int = 0) -> int:
    """drift_bins=None of recognize_speeds / recognize_warps: ceil(t_max * h / 65536), clamped so that a candidate's
    2 (tol + drift) + 1 bins stay within the 4,096 the moments allow.  t_max: the call's largest warped frame as the library
    computes it, round((max_frames - 1) * largest tempo rung); h: half the largest gap between neighbouring DISTINCT tempo
    rungs (Q16), 0 for one rung.  Derivation: a query of true tempo a warped at rung r puts its aligned pairs on the line
    d = t' (a / r - 1) + c (extent.tempo_of).  The best rung is the nearest one, so |a - r| <= h / 65536, and over the warped
    frames 0 .. t_max the line moves by at most t_max h / 65536 bins.  The match's delta is one bin ON that line, so the
    range delta +- that many bins holds all of it."""
    rungs = np.unique(np.asarray(tempos, np.int64))
    if len(rungs) < 2 or len(clip_samples) == 0:
        return 0
    gap = int(np.max(np.diff(rungs)))                                 # 2 h
    t_max = ((max(max(ctx.frames_of(int(n)) for n in clip_samples), 1) - 1) * int(rungs[-1]) + 32768) >> 16
    drift = -((-t_max * gap) // (2 * S_ONE))
    return max(0, min(drift, (4096 - 1) // 2 - int(tol)))


def _drift_of(ctx, chans, Fs, resample_to, tempos, drift_bins):
    """drift_bins of a call over the channels `chans`: the caller's, or default_drift_bins at the lengths the library sees"""
    if drift_bins is not None:
        return int(drift_bins)
    n = [len(c) for c in chans]
    if resample_to is not None and int(resample_to) != int(Fs):
        from .resample import out_len, resample_plan
        L, M = resample_plan(int(Fs), int(resample_to))[:2]
        n = [out_len(x, L, M) for x in n]
    return default_drift_bins(ctx, n, tempos, ctx.vote_tolerance)


def _add_warp_extents(results, res, q_t16, w: int):
    """the extent keys of recognize_speeds / recognize_warps(extents=True) from Context.recognize_warps' extent arrays; q_t16:
    the time factor of every query's best variant; w: vote tolerance + drift_bins, the half-width of every candidate"""
    from . import _frames_secs
    from .extent import line_fit, own_frames, tempo_of
    for q, dicts in enumerate(results):
        t16 = int(q_t16[q])
        for n, d in enumerate(dicts):
            wf, wl, tf, tl = (int(res[f][q, n]) for f in ("q_first", "q_last", "t_first", "t_last"))
            qf, ql = own_frames(wf, wl, t16)
            fit = {"count": int(res["count"][q, n]), **{k: int(res[k][q, n]) for k in ("sum_q", "sum_u", "sum_qq", "sum_qu")},
                   "d_lo": int(res["delta"][q, n]) - int(w)}
            line = line_fit(**fit)
            d.update({"query_first": qf, "query_last": ql, "song_first": tf, "song_last": tl,
                      "query_start_secs": _frames_secs(qf), "query_end_secs": _frames_secs(ql + 1),
                      "song_start_secs": _frames_secs(tf), "song_end_secs": _frames_secs(tl + 1),
                      "extent_hist": res["hist"][q, n].copy(), "extent_shift": int(res["shift"][q]),
                      "warped_first": wf, "warped_last": wl, "fit": fit,
                      "tempo_fit": None if line is None else float(tempo_of(t16, line[0]))})


@takes_delta_tol(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
def recognize_speeds(queries, db, speeds=None, Fs: int = 44100, topn: int = 2, resample_to: int = None, extents: bool = False,
                     drift_bins: int = None):
    """recognize_batch for queries of unknown speed.  Returns (results_per_query, timings) like recognize_batch; every
    result dict carries "speed" (the chosen factor as a float), OFFSET / OFFSET_SECS are in the TABLE's time, and timings
    carries "speeds" (the ladder, Q16), "speed_best" (index per query) and "speed_profile" ([n_queries, K]: the aligned count
    of the top answer of every factor).  speeds=None: speed_ladder().  The chosen factor is the one with the greatest
    aligned count; ties go to the factor nearest 1.0, then to the lower index.
    delta_tol= (keyword): the vote tolerance in offset bins while the call runs (Context.tolerance); None: the context's.
    A song filter is taken from the context: run the call inside `with ctx.songs(only=...)` / `ctx.songs(exclude=...)` to match
    within / without a set of songs (every variant, every listed song uses the one set).
    The key cap is taken from the context too: run the call inside `with ctx.key_cap(rows):` to leave out the keys that hold
    more than `rows` table rows (Context.key_cap).
    extents / drift_bins: as recognize_warps' -- the chosen speed is the rung of both axes, "tempo_fit" the fitted TIME factor."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, _as_pcm, _result_dicts, resample_to_device
    if not hasattr(db.table, "h"):
        raise NotImplementedError("fused recognition takes the unsharded table (shards=1)")
    sp = speed_ladder() if speeds is None else _check_speeds(speeds)
    ctx = db.ctx
    if getattr(ctx, "hop", HOP) != HOP:
        ctx.set_overlap(NFFT - HOP)
    db.finalize()
    chans, first = [], [0]
    for q in queries:
        cs = [q] if (isinstance(q, np.ndarray) and q.ndim == 1) else list(q)
        chans.extend(cs)
        first.append(len(chans))
    first = np.asarray(first, np.uint32)
    kw = dict(amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, topn=int(topn))
    if extents:
        kw.update(extents=True, drift_bins=_drift_of(ctx, chans, Fs, resample_to, sp, drift_bins))
    if resample_to is not None and int(resample_to) != int(Fs):   # resampled on the device and handed on there
        buf, off = resample_to_device(chans, int(Fs), int(resample_to), ctx)
        try:
            res, ms = ctx.recognize_speeds(db.table, buf, off, first, sp, fs=int(resample_to), pcm_device=True, **kw)
        finally:
            buf.free()
    else:
        arrs = [_as_pcm(c) for c in chans]
        off = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)
        res, ms = ctx.recognize_speeds(db.table, pcm, off, first, sp, fs=int(Fs), **kw)
    t0 = time()
    results = []
    for q in range(len(queries)):
        dicts = _result_dicts(db, res, q, int(res["nhash"][q]))
        for d in dicts:
            d["speed"] = float(sp[int(res["best"][q])]) / S_ONE
        results.append(dicts)
    extra = {}
    if extents:
        _add_warp_extents(results, res, sp[res["best"]], ctx.vote_tolerance + kw["drift_bins"])
        extra = {"extent_time": ms[3] * 1e-3, "drift_bins": kw["drift_bins"]}
    align_time = time() - t0
    return results, {"fingerprint_time": ms[0] * 1e-3, "warp_time": ms[1] * 1e-3, "query_time": ms[2] * 1e-3,
                     "align_time": align_time, "n_hashes": res["nhash"], "speeds": sp, "speed_best": res["best"],
                     "speed_profile": res["profile"], **extra}


def _warp_dist(t16, f16):
    return np.abs(t16.astype(np.int64) - S_ONE) + np.abs(f16.astype(np.int64) - S_ONE)


def merge_warp_chunks(parts, t16, f16):
    """The results of one set of queries over consecutive chunks of a pair list (Context.recognize_warps' res, in the list's
    order), as one call over the whole list would give them: per query the chunk whose best variant has the greatest
    rank-0 aligned count, ties to the smaller |t16 - 65536| + |f16 - 65536|, then to the lower index; the profiles side by
    side."""
    if len(parts) == 1:
        return parts[0]
    profile = np.concatenate([p["profile"] for p in parts], axis=1)
    starts = np.cumsum([0] + [p["profile"].shape[1] for p in parts])
    dist = _warp_dist(t16, f16)
    out = {k: v.copy() for k, v in parts[0].items()}
    out["profile"] = profile
    for q in range(len(out["best"])):
        cand = [int(starts[i] + p["best"][q]) for i, p in enumerate(parts)]
        g = min(cand, key=lambda v: (-int(profile[q, v]), int(dist[v]), v))
        i = cand.index(g)
        for k in out:
            if k not in ("profile", "best"):
                out[k][q] = parts[i][k][q]
        out["best"][q] = g
    return out


def _match_pairs(ctx, table, chans, first, t16, f16, row, Fs, resample_to, kw, drift=None):
    """Context.recognize_warps of the queries (chans: every channel, first: the CSR of the queries over them) over the
    whole pair list, in chunks of whole rows: (res, [ms_extract, ms_warp, ms_match, ms_extent] summed over the chunks).
    drift: None for no extents, else drift_bins (the same in every chunk: merge_warp_chunks then copies the extent arrays of
    the winning chunk like any other per-query key)."""
    from . import _as_pcm, resample_to_device
    buf = None
    if resample_to is not None and int(resample_to) != int(Fs):   # resampled on the device and handed on there
        buf, off = resample_to_device(chans, int(Fs), int(resample_to), ctx)
        pcm, fs, dev = buf, int(resample_to), True
    else:
        arrs = [_as_pcm(c) for c in chans]
        off = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        pcm, fs, dev = (np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)), int(Fs), False
    parts, ms = [], np.zeros(4)
    xkw = {} if drift is None else dict(extents=True, drift_bins=int(drift))
    try:
        for a, b in warp_chunks(len(t16), row):
            res, m = ctx.recognize_warps(table, pcm, off, first, t16[a:b], f16[a:b], fs=fs, pcm_device=dev, **kw, **xkw)
            parts.append(res)
            ms[:len(m)] += m
    finally:
        if buf is not None:
            buf.free()
    return merge_warp_chunks(parts, t16, f16), ms


def _warp_list(tempos, pitches, warps, search):
    """What recognize_warps and the scan make of tempos= / pitches= / warps= / search=: (tempo ladder, pitch ladder, t16, f16,
    row) -- the pair list tempo-major and the pairs of one row of it (an explicit pair list: no ladders, rows of 1)."""
    tl = pl = None
    if search not in ("grid", "separable"):
        raise ValueError('search is "grid" or "separable"')
    if warps is not None:
        if tempos is not None or pitches is not None:
            raise TypeError("warps= is an explicit pair list: it excludes tempos= and pitches=")
        if search != "grid":
            raise TypeError('search="separable" takes the two ladders, not a pair list')
        t16, f16 = _check_speeds(warps[0], "warps[0]"), _check_speeds(warps[1], "warps[1]")
        if len(t16) != len(f16):
            raise ValueError("warps=(t16, f16): two lists of one length")
        row = 1
    else:
        tl = np.asarray([S_ONE], np.uint32) if tempos is None else _check_speeds(tempos, "tempos")
        pl = np.asarray([S_ONE], np.uint32) if pitches is None else _check_speeds(pitches, "pitches")
        t16, f16 = warp_grid(tl, pl)
        row = max(len(pl), 1)
    return tl, pl, t16, f16, row


@takes_delta_tol(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
def recognize_warps(queries, db, tempos=None, pitches=None, warps=None, search: str = "grid", Fs: int = 44100, topn: int = 2,
                    resample_to: int = None, extents: bool = False, drift_bins: int = None):
    """recognize_speeds for queries whose tempo and pitch changed by factors of their own.  Returns (results_per_query,
    timings) like recognize_speeds; every result dict carries "tempo" and "pitch" (the chosen factors as floats: the query
    runs `tempo` times as fast and sounds `pitch` times as high as the table's copy), OFFSET / OFFSET_SECS are in the
    TABLE's time.  The variants:
      tempos / pitches   two Q16 ladders (tempo_ladder, pitch_ladder); None means [65536]
      warps=(t16, f16)   an explicit pair list instead of the two ladders (TypeError with either of them)
      search="grid"      every pair of the two ladders (warp_grid, tempo-major).  More than 1,024 pairs go to the library in
                         chunks of whole rows and are merged by the best-variant rule
      search="separable" two library calls: the pitch ladder at tempo 65536, then the tempo ladder at every query's best
                         pitch rung (queries that share a rung go together).  The answer is the second stage's.
                         len(tempos) + len(pitches) variants instead of their product.  A HEURISTIC: it relies on the
                         pitch axis being found while the tempo is still wrong, which holds while the first stage's top
                         answer is the right song -- measured up to a tempo
                         deviation of 5 %, where the first stage still named the right song with 106 .. 160 votes against
                         452 .. 584 at the true pair, and 59 .. 92 against 253 .. 347 at (1.03, 0.97) / (0.97, 1.03); beyond that, or against a table in
                         which a wrong song collects more votes than the drifting right one, it can miss what the grid finds.
    The chosen pair is the one with the greatest aligned count; ties go to the smaller |t16 - 65536| + |f16 - 65536|, then to
    the lower index.  timings carries "warps" (the two Q16 arrays of the pairs matched), "warp_best" (index per query) and
    "warp_profile" (the aligned count of the top answer of every pair): [n_pairs] / [n_queries, n_pairs] for the grid and
    for a pair list; for the separable search the pairs differ per query, and the three are those of the second stage --
    "warps" two [n_queries, len(tempos)] arrays, "warp_profile" of that shape -- with the first stage under "stage1"
    ("warps", "warp_best", "warp_profile").
    delta_tol= (keyword): the vote tolerance in offset bins while the call runs (Context.tolerance); None: the context's.
    A song filter is taken from the context: run the call inside `with ctx.songs(only=...)` / `ctx.songs(exclude=...)` to match
    within / without a set of songs (every variant, every listed song uses the one set).
    The key cap is taken from the context too: run the call inside `with ctx.key_cap(rows):` to leave out the keys that hold
    more than `rows` table rows (Context.key_cap).
    extents: every result dict also says WHERE the match holds and what tempo its pairs fit (shz_recognize_warps_extents,
    DESIGN.md 3.7m): the keys of recognize_batch(extents=True) -- "query_first" / "query_last" and the "query_*_secs" in the
    QUERY's own frames (extent.own_frames at the chosen time factor), "song_*", "extent_hist", "extent_shift" as the extent
    pass delivers them (the histogram over WARPED frames) --, "warped_first" / "warped_last" (the table's domain), "fit" (the
    pairs' count and moments sum_q, sum_u, sum_qq, sum_qu as Python ints, and d_lo) and "tempo_fit" (extent.tempo_of of
    extent.line_fit on them, a float; None where there is no line).  The candidate of a result is delta +- (the vote
    tolerance + drift_bins).  drift_bins=None: default_drift_bins of the call's tempo rungs -- the true tempo lies within half
    a step of the best rung, and the range must hold the drift that leaves (derivation there).  The separable search reports
    the second stage's extents.  The fit is an unweighted least-squares line: chance pairs inside the range pull it.
    Measured on an MI355X (scripts/fit_bench.py, profiles/fit_bench.json): note corpus, 8 songs of 30 s, 48
    queries of 10 s at true tempos 0.97 .. 1.03 against the default tempo ladder -- |tempo_fit - true| 0.00063 at the median,
    0.0021 at the worst, where |rung - true| is 0.012 and 0.022; every query had a fit; the extent stage took 0.37 ms beside a
    match of 0.61 ms.  Synthetic notes and a small table: not measured on real time-stretched audio.
    timings gains "extent_time" and "drift_bins"."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, _result_dicts
    if not hasattr(db.table, "h"):
        raise NotImplementedError("fused recognition takes the unsharded table (shards=1)")
    tl, pl, t16, f16, row = _warp_list(tempos, pitches, warps, search)
    ctx = db.ctx
    if getattr(ctx, "hop", HOP) != HOP:
        ctx.set_overlap(NFFT - HOP)
    db.finalize()
    per_query = [[q] if (isinstance(q, np.ndarray) and q.ndim == 1) else list(q) for q in queries]
    nq = len(per_query)

    def csr(idx):
        chans, first = [], [0]
        for q in idx:
            chans.extend(per_query[q])
            first.append(len(chans))
        return chans, np.asarray(first, np.uint32)

    kw = dict(amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, topn=int(topn))
    drift = None
    if extents:   # (from the whole call's clips and tempo rungs, whatever chunk or stage a library call holds)
        drift = _drift_of(ctx, [c for cs in per_query for c in cs], Fs, resample_to, t16 if search == "grid" else tl, drift_bins)
    run = lambda idx, a, b, r, x=None: _match_pairs(ctx, db.table, *csr(idx), a, b, r, Fs, resample_to, kw, x)
    extra = {}
    if search == "grid":
        res, ms = run(range(nq), t16, f16, row, drift)
        q_t16, q_f16 = t16[res["best"]], f16[res["best"]]
        shown = (t16, f16)
    else:
        one = np.full(len(pl), S_ONE, np.uint32)
        res1, ms = run(range(nq), one, pl, 1)
        extra["stage1"] = {"warps": (one, pl), "warp_best": res1["best"], "warp_profile": res1["profile"]}
        res = None
        for rung in np.unique(res1["best"]).tolist() if nq else []:
            idx = np.flatnonzero(res1["best"] == rung).tolist()
            part, m = run(idx, tl, np.full(len(tl), pl[rung], np.uint32), 1, drift)
            ms = ms + m
            if res is None:
                res = {k: np.zeros((nq,) + v.shape[1:], v.dtype) for k, v in part.items()}
            for k in res:
                res[k][idx] = part[k]
        if res is None:
            res = {k: np.zeros((nq,) + v.shape[1:], v.dtype) for k, v in res1.items() if k != "profile"}
            res["profile"] = np.zeros((nq, len(tl)), np.uint32)
        q_t16, q_f16 = tl[res["best"]], pl[res1["best"]]
        shown = (np.tile(tl, (nq, 1)), np.repeat(q_f16[:, None], len(tl), axis=1))
    t0 = time()
    results = []
    for q in range(nq):
        dicts = _result_dicts(db, res, q, int(res["nhash"][q]))
        for d in dicts:
            d["tempo"], d["pitch"] = float(q_t16[q]) / S_ONE, float(q_f16[q]) / S_ONE
        results.append(dicts)
    if extents:
        _add_warp_extents(results, res, q_t16, ctx.vote_tolerance + drift)
        extra.update({"extent_time": ms[3] * 1e-3, "drift_bins": drift})
    align_time = time() - t0
    return results, {"fingerprint_time": ms[0] * 1e-3, "warp_time": ms[1] * 1e-3, "query_time": ms[2] * 1e-3,
                     "align_time": align_time, "n_hashes": res["nhash"], "warps": shown, "warp_best": res["best"],
                     "warp_profile": res["profile"], **extra}
