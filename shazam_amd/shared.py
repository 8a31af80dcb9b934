"""Content shared between recordings, without a catalogue (csrc/shz_repeat.hip: shz_shared_*): "which
stretches of station A also aired on station B?", "which of Monday's adverts came back on Tuesday?", "where does this tape
overlap that one?" -- and, with a day cut into two recordings, the night re-run of daytime content that find_repeats cannot
see because no pair crosses recordings there.

A JOB is a pair of recordings (a, b).  A hash of a at time t_a and a hash of b with the same key at time t_b vote for the
SIGNED lag t_b - t_a; a stretch that airs in both piles its votes on one lag over a contiguous stretch of t_a.  The device
counts the votes per cell (job, lag, block of 2^cell_shift frames of a), the host joins neighbouring cells into shared
stretches with the fold of find_repeats (shz_repeats_fold), the jobs standing in for its recordings.  Every recording of a
call is fingerprinted once, however many jobs name it, and its hashes never leave the device.

ALTERED content (shz_shared_warps_*): with speeds= / tempos= / pitches= / warps= a job is (a, b, warp) -- "what of
a, played tempo times as fast and sounding pitch times as high as b's copy, airs in b".  The peaks of every recording are taken
once, one warp pass maps the peaks of a to every rung the jobs name, and the warped hashes go through the same join as virtual
recordings.  A stretch that shows at several rungs is reported once (choose_rungs), with its place in a's own frames and a tempo
fit from its cells (cells_fit)."""
from __future__ import annotations

import numpy as np

from ._ffi import HOP, SHARED_LAG_BIAS
from .repeats import FIRST_ROOM, MAX_LAG, _airing_groups, _fold

MAX_JOBS = 4096          # jobs of one library call (shz_shared_*): more are split
MAX_RECS = 4096          # recordings of one library call: a call carries only those its jobs name


def _all_pairs(n_recs: int) -> list:
    """pairs=None: every a < b"""
    return [(a, b) for a in range(n_recs) for b in range(a + 1, n_recs)]


def _check_pairs(pairs, n_recs: int) -> list:
    pairs = _all_pairs(n_recs) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if a == b or not (0 <= a < n_recs and 0 <= b < n_recs):
            raise ValueError(f"pair ({a}, {b}): two different recordings below {n_recs} are needed")
    return pairs


def _lag_window(min_lag_seconds, max_lag_seconds, fs: int, hop: int):
    """Signed seconds -> signed frames; None: that end of the range the library holds, -+(2^20 - 1) frames."""
    frames = lambda s: max(-MAX_LAG, min(MAX_LAG, int(round(float(s) * fs / hop))))   # noqa: E731
    lo = -MAX_LAG if min_lag_seconds is None else frames(min_lag_seconds)
    hi = MAX_LAG if max_lag_seconds is None else frames(max_lag_seconds)
    if hi < lo:
        raise ValueError(f"max_lag_seconds gives {hi} frames, below min_lag_seconds' {lo}")
    return lo, hi


def _plan_calls(pairs) -> list:
    """The job list cut into library calls: consecutive jobs, at most MAX_JOBS of them naming at most MAX_RECS recordings.
    Returns (first job, jobs of the call, the recordings they name in ascending order) per call."""
    calls, j0, named = [], 0, set()
    for j, (a, b) in enumerate(pairs):
        if j - j0 >= MAX_JOBS or len(named | {a, b}) > MAX_RECS:
            calls.append((j0, pairs[j0:j], sorted(named)))
            j0, named = j, set()
        named |= {a, b}
    if j0 < len(pairs):
        calls.append((j0, pairs[j0:], sorted(named)))
    return calls


def _shared_dicts(cells, rep, job0: int, jobs, recs, fs: int, hop: int) -> list:
    """jobs: the call's (a, b) in the caller's numbering; recs: the caller's number of every recording of the call"""
    secs = lambda frames: round(float(frames) * hop / fs, 5)                      # noqa: E731
    local = {r: i for i, r in enumerate(recs)}
    out = []
    for i in range(len(rep["rec"])):
        j, first, last = (int(rep[k][i]) for k in ("rec", "first", "last"))
        lag, lag_lo, lag_hi = (int(rep[k][i]) - SHARED_LAG_BIAS for k in ("lag", "lag_lo", "lag_hi"))
        a, b = jobs[j]
        out.append({
            "recording_a": a, "recording_b": b,
            "a_start_seconds": secs(first), "a_end_seconds": secs(last + 1),
            "b_start_seconds": secs(max(0, first + lag)), "b_end_seconds": secs(last + lag + 1),
            "lag_seconds": secs(lag),
            "job": job0 + j, "rec_a": a, "rec_b": b, "first": first, "last": last, "lag": lag, "lag_lo": lag_lo, "lag_hi": lag_hi,
            "pairs": int(rep["pairs"][i]), "cells": int(rep["cells"][i]),
            "stats": {"hashes_a": int(cells["rec_hashes"][local[a]]), "hashes_b": int(cells["rec_hashes"][local[b]]),
                      "pairs": int(cells["job_pairs"][j]), "skipped_keys": int(cells["job_skipped_keys"][j]),
                      "skipped_rows": int(cells["job_skipped_rows"][j])},
        })
    return out


# ---- altered content: the join at a ladder of warps (shz_shared_warps_*) -----------------------------------------
S_ONE = 65536
MAX_WARPS = 1024         # warps of one library call


def _warp_table(speeds, tempos, pitches, warps):
    """None without a ladder keyword, else (t16, f16): the pair list as catalog._ladder_of reads the keywords (speeds=True:
    speed_ladder()), with (65536, 65536) appended where the list lacks it -- the plain answer is always among the rungs."""
    from .catalog import _ladder_of
    from .speed import speed_ladder
    lad = _ladder_of(speed_ladder() if speeds is True else speeds, tempos, pitches, warps)
    if lad is None:
        return None
    t16, f16 = np.asarray(lad[0], np.uint32), np.asarray(lad[1], np.uint32)
    if not np.any((t16 == S_ONE) & (f16 == S_ONE)):
        t16, f16 = np.append(t16, np.uint32(S_ONE)), np.append(f16, np.uint32(S_ONE))
    return t16, f16


def _check_warp_pairs(pairs, n_recs: int) -> list:
    """as _check_pairs, but (a, a) is a job: the warped repeat inside one recording"""
    pairs = _all_pairs(n_recs) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if not (0 <= a < n_recs and 0 <= b < n_recs):
            raise ValueError(f"pair ({a}, {b}): recordings below {n_recs} are needed")
    return pairs


def _warp_jobs(pairs, t16, f16, lo: int, hi: int, self_min: int) -> list:
    """The library jobs (a, b, v, lag_lo, lag_hi, index into pairs), pair-major: every pair at every warp.  A pair (a, a) at a
    warp is two jobs, the lags [self_min, hi] and [lo, -self_min] (whichever of them the window leaves); at (65536, 65536) it is
    find_repeats' question and gives no job."""
    self_min = max(1, int(self_min))
    jobs = []
    for p, (a, b) in enumerate(pairs):
        for v in range(len(t16)):
            if a != b:
                jobs.append((a, b, v, lo, hi, p))
            elif int(t16[v]) != S_ONE or int(f16[v]) != S_ONE:
                jobs += [(a, a, v, w_lo, w_hi, p) for w_lo, w_hi in ((max(lo, self_min), hi), (lo, min(hi, -self_min))) if w_lo <= w_hi]
    return jobs


def _plan_warp_calls(jobs) -> list:
    """The job list cut into library calls of consecutive jobs under the three limits of a call: MAX_JOBS jobs, MAX_RECS
    recordings of the join -- the recordings named plus the distinct (a, warp) --, MAX_WARPS warps.  Returns (first job, end,
    recordings named ascending, warps named ascending) per call."""
    calls, j0, recs, virt, warps = [], 0, set(), set(), set()
    for j, (a, b, v, *_) in enumerate(jobs):
        if j - j0 >= MAX_JOBS or len(recs | {a, b}) + len(virt | {(a, v)}) > MAX_RECS or len(warps | {v}) > MAX_WARPS:
            calls.append((j0, j, sorted(recs), sorted(warps)))
            j0, recs, virt, warps = j, set(), set(), set()
        recs |= {a, b}
        virt.add((a, v))
        warps.add(v)
    if j0 < len(jobs):
        calls.append((j0, len(jobs), sorted(recs), sorted(warps)))
    return calls


def cells_fit(cells):
    """The weighted least-squares line lag = c + slope * mid through the cells of a stretch: cells is an iterable of (lag,
    first, last, pairs), mid = (first + last) / 2 and the weight of a cell its pairs.  Exact arithmetic, as extent.line_fit:
    returns (slope, c) as two fractions.Fraction, None with fewer than two distinct mid.  find_shared hands it the cells of
    the stretch's job inside the stretch's RECTANGLE -- lag_lo <= lag <= lag_hi, first >= the stretch's first, last <= its
    last --, which is what the fold's result names; a cell of the job that lies inside the rectangle without being linked to
    the stretch (a foreign cell: another stretch's, or chance) is taken in and pulls the line.  extent.tempo_of(t16, slope) is
    the tempo the line stands for."""
    from fractions import Fraction
    W = Sx = Sy = Sxx = Sxy = 0
    for lag, first, last, pairs in cells:
        x, y, w = int(first) + int(last), int(lag), int(pairs)             # x = 2 mid
        W, Sx, Sy, Sxx, Sxy = W + w, Sx + w * x, Sy + w * y, Sxx + w * x * x, Sxy + w * x * y
    den = W * Sxx - Sx * Sx
    if den == 0:
        return None
    half = Fraction(W * Sxy - Sx * Sy, den)                                # the slope over x = 2 mid
    return 2 * half, Fraction(Sy, W) - half * Fraction(Sx, W)


def _rect_cells(cells, j: int, first: int, last: int, lag_lo: int, lag_hi: int) -> list:
    """(lag, first, last, pairs) of job j's cells inside the rectangle; lags signed"""
    a, b = int(cells["cell_off"][j]), int(cells["cell_off"][j + 1])
    out = []
    for i in range(a, b):
        g, f, l = int(cells["lag"][i]) - SHARED_LAG_BIAS, int(cells["first"][i]), int(cells["last"][i])
        if lag_lo <= g <= lag_hi and f >= first and l <= last:
            out.append((g, f, l, int(cells["pairs"][i])))
    return out


def _overlap(s0: int, e0: int, s1: int, e1: int) -> bool:
    """two intervals (ends inclusive) overlap by at least half of the shorter one"""
    return 2 * (min(e0, e1) - max(s0, s1) + 1) >= min(e0 - s0 + 1, e1 - s1 + 1)


def choose_rungs(stretches) -> list:
    """The rung choice: of the stretches one (a, b) pair shows at different warps, the one to report.  stretches: dicts with
    job (the pair's index), warp, t16, f16, pairs, lag_lo, lag_hi, a_first / a_last (a's OWN frames) and b_first / b_last.
    Two stretches of one job at different warps are the same stretch when their a intervals overlap by at least half of the
    shorter one and their b intervals do as well; what is the same through a chain of others is the same.  The winner has the
    most pairs; ties go to the smaller lag_hi - lag_lo, then to the smaller |t16 - 65536| + |f16 - 65536|, then to the lower
    warp index.  Returns the winners in the order given, each a copy with candidates = [(warp, pairs, lag_lo, lag_hi)] of the
    stretches it beat.  A heuristic: the pair count grows with the length of a stretch and with the rung's fit alike."""
    up = list(range(len(stretches)))

    def root(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    by_job = {}
    for n, s in enumerate(stretches):
        by_job.setdefault(s["job"], []).append(n)
    for members in by_job.values():
        for i, x in enumerate(members):
            for y in members[i + 1:]:
                p, q = stretches[x], stretches[y]
                if p["warp"] != q["warp"] and _overlap(p["a_first"], p["a_last"], q["a_first"], q["a_last"]) \
                        and _overlap(p["b_first"], p["b_last"], q["b_first"], q["b_last"]):
                    rx, ry = root(x), root(y)
                    up[max(rx, ry)] = min(rx, ry)
    rank = lambda s: (-s["pairs"], s["lag_hi"] - s["lag_lo"], abs(s["t16"] - S_ONE) + abs(s["f16"] - S_ONE), s["warp"])  # noqa: E731
    groups = {}
    for n in range(len(stretches)):
        groups.setdefault(root(n), []).append(n)
    out = []
    for members in groups.values():
        best = min(members, key=lambda n: rank(stretches[n]))
        out.append((best, dict(stretches[best], candidates=[(stretches[n]["warp"], stretches[n]["pairs"], stretches[n]["lag_lo"],
                                                             stretches[n]["lag_hi"]) for n in members if n != best])))
    return [s for _, s in sorted(out, key=lambda x: x[0])]


def _warp_stretches(cells, rep, jobs, recs, t16, f16, fs: int, hop: int) -> list:
    """One dict per stretch of a library call, before the rung choice.  jobs: the call's (a, b, v, lag_lo, lag_hi, pair) in the
    caller's numbering; recs: the caller's number of every recording of the call."""
    from .extent import own_frames, tempo_of
    secs = lambda frames: round(float(frames) * hop / fs, 5)                      # noqa: E731
    local = {r: i for i, r in enumerate(recs)}
    out = []
    for i in range(len(rep["rec"])):
        j, first, last = (int(rep[k][i]) for k in ("rec", "first", "last"))
        lag, lag_lo, lag_hi = (int(rep[k][i]) - SHARED_LAG_BIAS for k in ("lag", "lag_lo", "lag_hi"))
        a, b, v, _, _, pair = jobs[j]
        tv, fv = int(t16[v]), int(f16[v])
        inside = _rect_cells(cells, j, first, last, lag_lo, lag_hi)
        a_first, a_last = own_frames(first, last, tv)
        b_first, b_last = min(f + g for g, f, _, _ in inside), max(l + g for g, _, l, _ in inside)
        fit = cells_fit(inside)
        d = {
            "recording_a": a, "recording_b": b,
            "a_start_seconds": secs(a_first), "a_end_seconds": secs(a_last + 1),
            "b_start_seconds": secs(max(0, b_first)), "b_end_seconds": secs(b_last + 1),
            "lag_seconds": secs(lag),
            "job": pair, "rec_a": a, "rec_b": b, "first": first, "last": last, "lag": lag, "lag_lo": lag_lo, "lag_hi": lag_hi,
            "pairs": int(rep["pairs"][i]), "cells": int(rep["cells"][i]),
            "warp": v, "t16": tv, "f16": fv, "tempo": tv / 65536.0, "pitch": fv / 65536.0,
            "a_first": a_first, "a_last": a_last, "b_first": b_first, "b_last": b_last,
            "tempo_fit": None if fit is None else float(tempo_of(tv, fit[0])),
            "stats": {"hashes_a": int(cells["job_hashes"][j]), "hashes_b": int(cells["rec_hashes"][local[b]]),
                      "pairs": int(cells["job_pairs"][j]), "skipped_keys": int(cells["job_skipped_keys"][j]),
                      "skipped_rows": int(cells["job_skipped_rows"][j])},
        }
        if tv == fv:
            d["speed"] = tv / 65536.0
        out.append(d)
    return out


def _find_warped(call, n_recs: int, pairs, table, lo: int, hi: int, self_min: int, lag_tol, max_gap, min_pairs, fs: int, hop: int):
    """The driver both forms share: the jobs, the calls, the fold of every call, the rung choice over all of them.
    call(recs, t16, f16, jobs) -> the cells of one library call, recs / jobs in the call's numbering."""
    t16, f16 = table
    jobs = _warp_jobs(pairs, t16, f16, lo, hi, self_min)
    found = []
    for j0, j1, recs, warps in _plan_warp_calls(jobs):
        lrec, lwarp = {r: i for i, r in enumerate(recs)}, {v: i for i, v in enumerate(warps)}
        ljobs = [(lrec[a], lrec[b], lwarp[v], w_lo, w_hi) for a, b, v, w_lo, w_hi, _ in jobs[j0:j1]]
        cells = call(recs, t16[warps], f16[warps], ljobs)
        found.extend(_warp_stretches(cells, _fold(cells, lag_tol, max_gap, min_pairs), jobs[j0:j1], recs, t16, f16, fs, hop))
    out = choose_rungs(found)
    out.sort(key=lambda s: (s["job"], s["a_first"], s["lag"]))
    return out


_SHARED_WARP_DOC = """
    ALTERED content: speeds= / tempos= / pitches= / warps= (Q16, read as catalog.find_duplicates reads them; speeds=True:
    speed_ladder()) join every pair at every rung of the ladder -- "what of a, played tempo times as fast and sounding pitch
    times as high as b's copy, airs in b" (shz_shared_warps_*, DESIGN.md 3.7r).  (65536, 65536) is always among the rungs
    (appended where the list lacks it), so the plain answer is among the candidates.  pairs may then hold (a, a), the warped
    repeat inside one recording: every rung but (65536, 65536) -- that one is find_repeats' -- is asked for the lags from
    self_min_lag_seconds up and from -self_min_lag_seconds down.  Long job lists are cut into library calls under the three
    limits of a call: 4,096 jobs, 4,096 recordings plus distinct (a, warp), 1,024 warps.
    How fine a ladder: the tables of DESIGN.md 3.7r (an 8 s piece of rendered notes, find_shared's defaults, computed by
    scripts/shared_warp_curves.py) have the numbers.  A SPEED rung is sharp, because it moves the frequency bins: of the 415
    pairs at the true rung about 250 are left 0.05 % beside it and about 120 at 0.10 %, the fold returns the piece up to
    0.10 % off and no longer at 0.15 %, and at 0.25 % nothing but chance is left.  A TEMPO rung with the pitch hit is blunt:
    2 % off, the piece still has its 500 pairs, the lag drifts over four or five bins and tempo_fit names the tempo to 0.002.
    So: speed and pitch ladders in speed_ladder()'s default step of 0.14 % (every true factor is then at most 0.07 % from a
    rung) -- a ladder of 1 % steps finds only what happens to sit on a rung --, tempo ladders in steps of 2 to 4 %.
    A stretch that shows at several rungs is reported once (choose_rungs: most pairs).  Its dict holds what the plain one
    holds -- first, last, lag, lag_lo, lag_hi in a's WARPED frames -- and: warp (index into the pair list), tempo, pitch,
    speed (where tempo == pitch); a_first / a_last and a_start_seconds / a_end_seconds in a's OWN frames; b_first / b_last and
    b_start_seconds / b_end_seconds from the stretch's cells (min of first + lag, max of last + lag); tempo_fit, the tempo
    cells_fit's line through those cells stands for (None: one cell); candidates, [(warp, pairs, lag_lo, lag_hi)] of the
    rungs it beat; stats.hashes_a is a's hashes AT the warp.  Ordered by (job, a_first, lag)."""


def find_shared(recordings, pairs=None, Fs: int = 44100, min_lag_seconds: float = None, max_lag_seconds: float = None,
                cell_shift: int = 5, min_cell_pairs: int = 8, lag_tol: int = 1, max_gap: int = 1, min_pairs: int = 100,
                max_run: int = 64, resample_to: int = None, ctx=None, speeds=None, tempos=None, pitches=None, warps=None,
                self_min_lag_seconds: float = 1.0) -> list:
    """The stretches that pairs of recordings share.  recordings: 1-D int16 arrays, or lists of channels, as find_repeats takes
    them.  pairs: the jobs (a, b), "what of recording a also airs in recording b" (None: every a < b); a recording may be named
    any number of times, (a, b) and (b, a) may both be listed, and a pair listed twice is answered twice.  The lag is t_b - t_a,
    SIGNED: min_lag_seconds .. max_lag_seconds bound it (None: that end of what the library holds, -+(2^20 - 1) frames).
    cell_shift, min_cell_pairs, lag_tol, max_gap, min_pairs, max_run and resample_to as find_repeats; a key with more than
    max_run times in either recording of a job is a stop hash there.
    More than 4,096 jobs, or jobs that name more than 4,096 recordings, are cut into library calls of consecutive jobs; a call
    carries only the recordings its jobs name, so a recording named by jobs of two calls is fingerprinted twice.
    Returns one dict per shared stretch, ordered by (job, first, lag): recording_a, recording_b; a_start_seconds /
    a_end_seconds (the stretch in a), b_start_seconds / b_end_seconds (in b; the start not below 0), lag_seconds (signed); the
    integers job (index into pairs), rec_a, rec_b, first, last (frames of a, inclusive), lag (the lag with the most pairs),
    lag_lo, lag_hi (signed), pairs, cells; and stats: hashes_a, hashes_b, and the job's pairs, skipped_keys, skipped_rows."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, get_context, resample_to_device
    from .scan import _flatten
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP))
    recordings = list(recordings)
    table = _warp_table(speeds, tempos, pitches, warps)
    pairs = _check_pairs(pairs, len(recordings)) if table is None else _check_warp_pairs(pairs, len(recordings))
    resampled = resample_to is not None and int(resample_to) != int(Fs)
    fs = int(resample_to) if resampled else int(Fs)
    lo, hi = _lag_window(min_lag_seconds, max_lag_seconds, fs, hop)
    kw = dict(max_run=int(max_run), cell_shift=int(cell_shift), min_cell_pairs=int(min_cell_pairs), fs=fs,
              amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, cap_cells=FIRST_ROOM)
    if table is not None:
        def call(recs, t16, f16, ljobs):
            chans, first = _flatten([recordings[r] for r in recs])
            if resampled:
                buf, off = resample_to_device(chans, int(Fs), fs, ctx)
                try:
                    return ctx.shared_warps_batch(buf, off, first, t16, f16, ljobs, pcm_device=True, **kw)[0]
                finally:
                    buf.free()
            off = np.zeros(len(chans) + 1, np.uint64)
            off[1:] = np.cumsum([len(c) for c in chans])
            pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
            return ctx.shared_warps_batch(pcm, off, first, t16, f16, ljobs, **kw)[0]
        return _find_warped(call, len(recordings), pairs, table, lo, hi, int(round(float(self_min_lag_seconds) * fs / hop)), lag_tol,
                            max_gap, min_pairs, fs, hop)
    out = []
    for job0, jobs, recs in _plan_calls(pairs):
        local = {r: i for i, r in enumerate(recs)}
        ljobs = [(local[a], local[b]) for a, b in jobs]
        chans, first = _flatten([recordings[r] for r in recs])
        if resampled:
            buf, off = resample_to_device(chans, int(Fs), fs, ctx)
            try:
                cells, _ = ctx.shared_batch(buf, off, first, ljobs, lo, hi, pcm_device=True, **kw)
            finally:
                buf.free()
        else:
            off = np.zeros(len(chans) + 1, np.uint64)
            off[1:] = np.cumsum([len(c) for c in chans])
            pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
            cells, _ = ctx.shared_batch(pcm, off, first, ljobs, lo, hi, **kw)
        out.extend(_shared_dicts(cells, _fold(cells, lag_tol, max_gap, min_pairs), job0, jobs, recs, fs, hop))
    return out


find_shared.__doc__ += _SHARED_WARP_DOC


def find_shared_peaks(peak_f, peak_t, peak_off, rec_clip0=None, pairs=None, Fs: int = 44100, min_lag_seconds: float = None,
                      max_lag_seconds: float = None, cell_shift: int = 5, min_cell_pairs: int = 8, lag_tol: int = 1, max_gap: int = 1,
                      min_pairs: int = 100, max_run: int = 64, ctx=None, hop: int = None, speeds=None, tempos=None, pitches=None,
                      warps=None, self_min_lag_seconds: float = 1.0, fan_value: int = None) -> list:
    """find_shared at a ladder for callers who hold PEAKS (Context.peaks): peak_f / peak_t the peaks of all clips in (t asc, f
    asc) order per clip, peak_off their CSR over the clips, rec_clip0 the CSR of the recordings over the clips (None: every
    clip a recording of its own).  Fs and hop (None: the context's) are what the peaks' frames were counted at.  Without a
    ladder keyword the one rung is (65536, 65536).  A call carries the peaks of the recordings its jobs name, gathered on the
    host; the dicts are those of find_shared at a ladder."""
    from . import DEFAULT_FAN_VALUE, get_context
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP)) if hop is None else int(hop)
    fan = DEFAULT_FAN_VALUE if fan_value is None else int(fan_value)
    peak_off = np.ascontiguousarray(peak_off, np.uint64)
    rec_clip0 = np.arange(len(peak_off), dtype=np.uint32) if rec_clip0 is None else np.ascontiguousarray(rec_clip0, np.uint32)
    table = _warp_table(speeds, tempos, pitches, warps) or (np.asarray([S_ONE], np.uint32),) * 2
    pairs = _check_warp_pairs(pairs, len(rec_clip0) - 1)
    lo, hi = _lag_window(min_lag_seconds, max_lag_seconds, int(Fs), hop)
    peak_f, peak_t = np.asarray(peak_f, np.uint16), np.asarray(peak_t, np.uint32)

    def call(recs, t16, f16, ljobs):
        fs_, ts_, po, rc = [np.zeros(0, np.uint16)], [np.zeros(0, np.uint32)], [0], [0]
        for r in recs:                                                            # the named recordings, one behind the other
            for c in range(int(rec_clip0[r]), int(rec_clip0[r + 1])):
                a, b = int(peak_off[c]), int(peak_off[c + 1])
                fs_.append(peak_f[a:b])
                ts_.append(peak_t[a:b])
                po.append(po[-1] + b - a)
            rc.append(len(po) - 1)
        return ctx.shared_warps_peaks(np.concatenate(fs_), np.concatenate(ts_), po, rc, t16, f16, ljobs, int(max_run), int(cell_shift),
                                      int(min_cell_pairs), fan)
    return _find_warped(call, len(rec_clip0) - 1, pairs, table, lo, hi, int(round(float(self_min_lag_seconds) * int(Fs) / hop)), lag_tol,
                        max_gap, min_pairs, int(Fs), hop)


def find_shared_hashes(key32, t1, hash_off, rec_clip0=None, pairs=None, Fs: int = 44100, min_lag_seconds: float = None,
                       max_lag_seconds: float = None, cell_shift: int = 5, min_cell_pairs: int = 8, lag_tol: int = 1,
                       max_gap: int = 1, min_pairs: int = 100, max_run: int = 64, ctx=None, hop: int = None) -> list:
    """find_shared for callers who hold fingerprints: key32 / t1 the hashes of all clips (as fingerprint_batch returns them),
    hash_off their CSR over the clips, rec_clip0 the CSR of the recordings over the clips (None: every clip a recording of
    its own).  Fs and hop (None: the context's) are what the hashes' frames were counted at.  A call carries the hashes of the
    recordings its jobs name, gathered on the host."""
    from . import get_context
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP)) if hop is None else int(hop)
    hash_off = np.ascontiguousarray(hash_off, np.uint64)
    rec_clip0 = np.arange(len(hash_off), dtype=np.uint32) if rec_clip0 is None else np.ascontiguousarray(rec_clip0, np.uint32)
    pairs = _check_pairs(pairs, len(rec_clip0) - 1)
    lo, hi = _lag_window(min_lag_seconds, max_lag_seconds, int(Fs), hop)
    key32, t1 = np.asarray(key32, np.uint32), np.asarray(t1, np.uint32)
    out = []
    for job0, jobs, recs in _plan_calls(pairs):
        local = {r: i for i, r in enumerate(recs)}
        ks, ts, ho, rc = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [0], [0]
        for r in recs:                                                            # the named recordings, one behind the other
            for c in range(int(rec_clip0[r]), int(rec_clip0[r + 1])):
                a, b = int(hash_off[c]), int(hash_off[c + 1])
                ks.append(key32[a:b])
                ts.append(t1[a:b])
                ho.append(ho[-1] + b - a)
            rc.append(len(ho) - 1)
        cells = ctx.shared_hashes(np.concatenate(ks), np.concatenate(ts), ho, rc, [(local[a], local[b]) for a, b in jobs], lo, hi,
                                  int(max_run), int(cell_shift), int(min_cell_pairs))
        out.extend(_shared_dicts(cells, _fold(cells, lag_tol, max_gap, min_pairs), job0, jobs, recs, int(Fs), hop))
    return out


def shared_occurrences(shared, repeats=()) -> list:
    """The airings behind shared stretches and repeats, across recordings (host only): the cross-recording form of
    occurrences().  Every shared stretch names the intervals (rec_a, first, last) and (rec_b, first + lag, last + lag); every
    repeat names (rec, first, last) and (rec, first + lag, last + lag).  Two intervals of ONE recording are the same airing
    when they overlap by at least half of the shorter one; airings joined by a shared stretch or a repeat form a group -- an
    advert aired twice on Monday and once on Tuesday comes back as one group of three airings.  shared: find_shared's dicts
    (rec_a, rec_b, first, last, lag are read); repeats: find_repeats' (rec, first, last, lag), over the same numbering of the
    recordings.  Returns a list of dicts ordered by first airing: airings (sorted (recording, first, last), each the hull of
    the intervals merged into it), shared and repeats (indices into the lists given).
    A stretch found at a ladder (find_shared(speeds= / tempos= / pitches= / warps=)) names its intervals itself: (rec_a, a_first,
    a_last), a's OWN frames, and (rec_b, b_first, b_last) -- its first / last are warped frames, which are no place in a."""
    items = []                                      # two intervals per stretch, then two per repeat
    for p in shared:
        f, l, g = int(p["first"]), int(p["last"]), int(p["lag"])
        if "a_first" in p:
            items += [(int(p["rec_a"]), int(p["a_first"]), int(p["a_last"])), (int(p["rec_b"]), int(p["b_first"]), int(p["b_last"]))]
        else:
            items += [(int(p["rec_a"]), f, l), (int(p["rec_b"]), f + g, l + g)]
    ns = len(items) // 2
    for p in repeats:
        r, f, l, g = int(p["rec"]), int(p["first"]), int(p["last"]), int(p["lag"])
        items += [(r, f, l), (r, f + g, l + g)]
    out = [{"airings": sorted(tuple(h) for h in airs), "shared": sorted(n for n in links if n < ns),
            "repeats": sorted(n - ns for n in links if n >= ns)} for airs, links in _airing_groups(items)]
    out.sort(key=lambda g: g["airings"][0])
    return out
