"""Scanning long recordings: "which songs play in this recording, and when?" (csrc/shz_scan.hip).

The reference recognises one recorded stretch at a time (recognizer.py:357-392).  A monitor asks the same question of every
overlapping stretch of an hour of broadcast.  Here every recording is fingerprinted ONCE; its device-resident hash list is cut
into overlapping time windows, all windows are matched together (shz_scan_batch), and the per-window answers are folded
into segments (shz_scan_timeline).

A window's hashes are a SUBSET of the whole recording's hashes -- not what fingerprinting the cut audio would give: peaks
near a cut see their neighbours beyond it, and a pair counts for the window its anchor lies in.  A recording must fit one
extraction pass (2^20 frames, about 13.5 hours at the default hop); chaining longer files is the caller's.

Recordings that play at another speed are scanned at a speed ladder (speeds=); recordings whose tempo and
pitch moved by factors of their own at a list of warp pairs (tempos= / pitches= / warps=), every window at
every pair (search="grid") or, far cheaper, every window at the pitch ladder and then at the tempo ladder beside its own best
pitch (search="separable", a heuristic), which rests on the library's per-window variant lists."""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._ffi import HOP, takes_delta_tol, takes_key_cap, takes_song_filter

TOPN = 2                 # recognizer.py:68, as the package has it
DEFAULT_FS = 44100       # recognizer.py:21-38


def _flatten(recordings):
    """Channels of all recordings, and the first channel of every recording (+ the end)."""
    from . import _as_pcm
    chans, first = [], [0]
    for r in recordings:
        cs = [r] if (isinstance(r, np.ndarray) and r.ndim == 1) else list(r)
        chans.extend(_as_pcm(c) for c in cs)
        first.append(len(chans))
    return chans, np.asarray(first, np.uint32)


def seconds_to_frames(seconds: float, Fs: int, hop: int = HOP) -> int:
    """round(seconds * Fs / hop), at least 1: a span of time in spectrogram frames."""
    return max(1, int(round(float(seconds) * int(Fs) / int(hop))))


def _ladder(speeds):
    """speeds=True: the default ladder; else Q16 integers as recognize_speeds takes them."""
    from .speed import _check_speeds, speed_ladder
    return speed_ladder() if speeds is True else _check_speeds(speeds)


# shift_tol of a scan over warps.  Between neighbouring hits of one piece |delta2 - delta1 - W(step)| was at
# most 1 frame on the fixture of tests/test_gpu_scan_warps.py under the default ladders, and 3 frames where a piece's tempo
# (1.08) lies between two rungs of the default tempo ladder (1.042, 1.084) and neighbouring windows choose either: a window
# matched at a tempo that is off by d sees the song position of about its middle, off by d x window / 2 -- one rung (4.2 %)
# over half a 108-frame window is 2.3 frames, plus the rounding.  The largest measured value plus one frame for the rounding
# of the two deltas.
WARP_SHIFT_TOL = 4


def _rung(ladder) -> int:
    """The largest gap between neighbouring distinct values of a Q16 list (0 for a single value)."""
    u = np.unique(np.asarray(ladder, np.int64))
    return int(np.diff(u).max()) if len(u) > 1 else 0


def _warp_dist(t16, f16):
    return np.abs(np.asarray(t16, np.int64) - 65536) + np.abs(np.asarray(f16, np.int64) - 65536)


def _merge_dense(parts, t16, f16):
    """Dense scan_warps results over consecutive chunks of a pair list as one call over the whole list gives them."""
    from .speed import merge_warp_chunks
    work = tuple(int(sum(p["work"][i] for p in parts)) for i in range(2))
    out = merge_warp_chunks([{k: v for k, v in p.items() if k != "work"} for p in parts], t16, f16)
    out["work"] = work
    return out


def _scan_warp_windows(run, tl, pl, t16, f16, row, search):
    """The library calls of a scan over warps.  run(t16, f16, select) -> (res, win_off, ms) is Context.scan_warps on the
    prepared audio.  Returns (res, win_off, ms); res["warps"] = (t16, f16) of the variants res["best"] indexes."""
    from .speed import S_ONE, warp_chunks, warp_grid
    ms = np.zeros(4)

    def dense(a16, b16, r):
        parts, wo = [], None
        for a, b in warp_chunks(len(a16), r):
            res, wo, m = run(a16[a:b], b16[a:b], None)
            parts.append(res)
            ms[:] += m
        return _merge_dense(parts, a16, b16), wo
    if search == "grid":
        res, win_off = dense(t16, f16, row)
        res["tried"], res["warps"] = np.ones(res["profile"].shape, bool), (t16, f16)
        return res, win_off, ms
    # separable: the pitch ladder at tempo 1, then per window the tempo ladder at its own best pitch
    one = np.full(len(pl), S_ONE, np.uint32)
    res, win_off = dense(one, pl, 1)
    n_wins = len(res["best"])
    res["stage1"] = {"best": res["best"].copy(), "profile": res["profile"], "work": res["work"]}
    found = res["profile"][np.arange(n_wins), res["best"]] >= 1 if n_wins else np.zeros(0, bool)
    rungs = np.unique(res["best"][found])                      # the distinct pitch rungs stage 1's windows chose
    others = np.flatnonzero(tl != S_ONE)
    g_t, g_f = warp_grid(tl, pl[rungs]) if len(rungs) else (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    all_t, all_f = np.concatenate([one, g_t]), np.concatenate([pl, g_f])
    profile = np.zeros((n_wins, len(all_t)), np.uint32)
    tried = np.zeros((n_wins, len(all_t)), bool)
    profile[:, :len(pl)], tried[:, :len(pl)] = res["profile"], True
    work2 = (0, 0)
    if len(rungs) and len(others):
        col = np.searchsorted(rungs, res["best"])              # a window's column of the stage-2 grid
        lists = [(others * len(rungs) + col[w]) if found[w] else np.zeros(0, np.int64) for w in range(n_wins)]
        dist = _warp_dist(all_t, all_f)
        top = profile[np.arange(n_wins), res["best"]].astype(np.int64)
        for a, b in warp_chunks(len(g_t), len(rungs)):
            part = [x[(x >= a) & (x < b)] - a for x in lists]
            so = np.concatenate([[0], np.cumsum([len(x) for x in part])]).astype(np.uint64)
            sw = np.concatenate(part).astype(np.uint32) if so[-1] else np.zeros(0, np.uint32)
            r2, _, m = run(g_t[a:b], g_f[a:b], (so, sw))
            ms[:] += m
            work2 = (work2[0] + r2["work"][0], work2[1] + r2["work"][1])
            for w in np.flatnonzero(np.diff(so.astype(np.int64)) > 0).tolist():
                cols = len(pl) + a + sw[int(so[w]):int(so[w + 1])].astype(np.int64)
                profile[w, cols], tried[w, cols] = r2["profile"][int(so[w]):int(so[w + 1])], True
                g = len(pl) + a + int(r2["best"][w])
                cur = int(res["best"][w])
                p = int(profile[w, g])
                if (-p, int(dist[g]), g) < (-int(top[w]), int(dist[cur]), cur):     # the best-variant rule over both stages
                    top[w] = p
                    res["best"][w] = g
                    for k in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs"):
                        res[k][w] = r2[k][w]
    res["stage2"] = {"work": work2}
    res["work"] = (res["work"][0] + work2[0], res["work"][1] + work2[1])
    res["profile"], res["tried"], res["warps"] = profile, tried, (all_t, all_f)
    return res, win_off, ms


@takes_key_cap(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
@takes_song_filter(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
@takes_delta_tol(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
def scan_windows(recordings, db, Fs: int = 44100, window_seconds: float = 5, step_seconds: float = 1, topn: int = TOPN,
                 resample_to: int = None, full_sort: bool = False, speeds=None, tempos=None, pitches=None, warps=None,
                 search: str = "grid", floor: bool = False, _extents: dict = None, _fit: dict = None):
    """Every window of every recording matched in one library call.  recordings: 1-D int16 arrays, or lists of channels as in
    recognize_batch.  Returns a dict: the arrays of Table.match over all windows, recording-major (sid, delta, aligned, dedup
    [n_windows, topn]; nres, nhash, npairs [n_windows]), plus win_off (CSR of the windows over the recordings), frames (F_r
    of every recording), window_frames, step_frames, hop, fs (the rate the frames are counted at) and ms = (extract, window,
    match) device times.  Window w of a recording starts at frame w * step_frames; `delta` is the song frame at the window's
    start.  resample_to: the recordings are at Fs, the table at resample_to; they are resampled on the device and scanned
    there.  speeds (a Q16 ladder, or True for speed_ladder()): every window is matched at every rung (shz_scan_speeds,
    DESIGN.md 3.7d); the arrays are the best rung's, `delta` is in the TABLE's frames, and the dict gains best (rung index
    per window), profile ([n_windows, K]), speed (the chosen factor per window, float), speeds (the ladder) and ms =
    (extract, warp, window, match).  speeds=None: the plain scan, untouched.
    tempos / pitches (two Q16 ladders), warps=(t16, f16) and search="grid" | "separable" mean what they mean in
    recognize_warps and exclude speeds= (ValueError): every window is matched at warp pairs (shz_scan_warps, DESIGN.md
    3.7i).  The dict then carries best (index per window into warps), warps (the two Q16 lists of the variants), profile
    ([n_windows, len(warps[0])]: the rank-0 aligned count of every variant) and tried (which of them the window tried: all
    for the grid), tempo / pitch (the chosen factors per window, float), work = (warped hash entries written, window entries
    handed to the match) summed over the calls, and ms = (extract, warp, window, match).  search="grid": one dense call;
    more than 1,024 pairs go in calls of whole tempo rows, merged by the best-variant rule.  search="separable", a
    HEURISTIC as in recognize_warps: stage 1 scans every window at (65536, p) for every pitch; stage 2 is one call in which
    every window that stage 1 gave a rank-0 count of at least 1 tries (a, its own best pitch) for every tempo a != 65536 and
    the other windows try nothing; the answer is the best over everything a window tried, the variants are stage 1's
    followed by the stage-2 grid (the tempos x the pitch rungs stage 1 chose), and stage1 / stage2 carry the stages' own
    best / profile / work.
    delta_tol= (keyword): the vote tolerance in offset bins while the call runs (Context.tolerance); None: the context's.
    floor (the plain scan only: ValueError with speeds=, tempos=, pitches=, warps= or another search): the dict gains song_hist
    and bin_hist, [n_windows, 32] uint32, recording-major -- the two vote-floor histograms of every window (Context.floor,
    shazam_amd.floor); the other arrays do not change.
    songs= / exclude= (keywords, song ids): every window is matched within / without these songs (Context.songs): the arrays
    of the same scan on a database holding only the allowed songs, npairs counting the kept pairs; any kind of scan.
    max_key_rows= (keyword): the key cap while the call runs (Context.key_cap: keys that hold more table rows vote for
    nobody); None: the context's; any kind of scan.
    _fit (scan(extents="fit")): the plays stage of a warped scan runs behind the scan on the same prepared audio -- with
    resample_to= the same device buffer, before it is freed -- and the dict gains "plays" (_play_stage)."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, resample_to_device
    if not hasattr(db.table, "h"):
        raise NotImplementedError("scanning takes the unsharded table (shards=1)")
    warped = tempos is not None or pitches is not None or warps is not None or search != "grid"
    if warped and speeds is not None:
        raise ValueError("speeds= is one factor for time and frequency: it excludes tempos=, pitches= and warps=")
    if floor and (warped or speeds is not None):
        raise ValueError("floor=True takes the plain scan: not with speeds=, tempos=, pitches=, warps= or another search")
    if floor and _extents is not None:
        raise ValueError("floor=True takes the plain scan: not inside the extent call")
    if warped:
        from .speed import _warp_list
        tl, pl, t16, f16, row = _warp_list(tempos, pitches, warps, search)
    ctx = db.ctx
    topn = int(topn)
    db.finalize()
    hop = int(getattr(ctx, "hop", HOP))
    chans, first = _flatten(recordings)
    fs = int(Fs)
    kw = dict(amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, topn=topn, full_sort=full_sort)
    if warped:
        def run(table, pcm, off, first, wf, sf, **k):
            call = lambda a16, b16, select: ctx.scan_warps(table, pcm, off, first, wf, sf, a16, b16, select, **k)   # noqa: E731
            res, win_off, ms = _scan_warp_windows(call, tl, pl, t16, f16, row, search)
            return res, win_off, tuple(float(m) for m in ms)
    elif _extents is not None:   # scan(extents=True): the timeline and the extent pass inside the same library call
        if speeds is not None:
            raise ValueError("extents=True takes the plain scan: not with speeds=")

        def run(table, pcm, off, first, wf, sf, fs, **k):
            ms_ = _extents["margin_seconds"]
            margin = wf if ms_ is None else max(0, int(round(float(ms_) * fs / hop)))
            res, win_off, seg, zone, ms = ctx.scan_extents(table, pcm, off, first, wf, sf, _extents["min_aligned"], _extents["max_gap"],
                                                           margin, ctx.vote_tolerance, fs=fs, keep=_extents.get("keep"), **k)
            res.update(segments=seg, zones=zone, margin_frames=margin)
            return res, win_off, ms
    elif floor:       # the rows the call records, one per window in the order of the result arrays
        def run(*a, **k):
            with ctx.floor():
                res, win_off, ms = ctx.scan_batch(*a, **k)
                res["song_hist"], res["bin_hist"] = ctx.take_floor()
            if len(res["song_hist"]) != len(res["nres"]):
                raise RuntimeError(f"vote floor: {len(res['song_hist'])} rows recorded for {len(res['nres'])} windows")
            return res, win_off, ms
    elif speeds is None:
        run = ctx.scan_batch
    else:
        sp = _ladder(speeds)
        run = lambda table, pcm, off, first, wf, sf, **k: ctx.scan_speeds(table, pcm, off, first, wf, sf, sp, **k)   # noqa: E731
    if resample_to is not None and int(resample_to) != fs:
        fs = int(resample_to)
        wf, sf = seconds_to_frames(window_seconds, fs, hop), seconds_to_frames(step_seconds, fs, hop)
        buf, off = resample_to_device(chans, int(Fs), fs, ctx)
        try:
            res, win_off, ms = run(db.table, buf, off, first, wf, sf, fs=fs, pcm_device=True, **kw)
            if _fit is not None:
                res["plays"] = _play_stage(ctx, db.table, buf, off, first, wf, sf, fs, hop, res, win_off, _fit, True)
        finally:
            buf.free()
    else:
        wf, sf = seconds_to_frames(window_seconds, fs, hop), seconds_to_frames(step_seconds, fs, hop)
        off = np.zeros(len(chans) + 1, np.uint64)
        if chans:
            off[1:] = np.cumsum([len(c) for c in chans])
        pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
        res, win_off, ms = run(db.table, pcm, off, first, wf, sf, fs=fs, **kw)
        if _fit is not None:
            res["plays"] = _play_stage(ctx, db.table, pcm, off, first, wf, sf, fs, hop, res, win_off, _fit, False)
    frames = np.array([max((ctx.frames_of(int(off[c + 1] - off[c])) for c in range(int(first[r]), int(first[r + 1]))), default=0)
                       for r in range(len(first) - 1)], np.int64)
    res.update(win_off=win_off, frames=frames, window_frames=wf, step_frames=sf, hop=hop, fs=fs, ms=ms)
    if speeds is not None:
        res.update(speeds=sp, speed=sp[res["best"]].astype(np.float64) / 65536.0)
    if warped:
        res.update(tempo=res["warps"][0][res["best"]].astype(np.float64) / 65536.0,
                   pitch=res["warps"][1][res["best"]].astype(np.float64) / 65536.0)
    return res


def default_drift_bins(window_frames: int, margin_frames: int, time_factors, tol: int) -> int:
    """drift_bins=None of scan(extents="fit"): ceil(L h / 65536), L = ceil((window + margin) t_max / 65536) the largest warped
    edge-zone length and h the largest gap between neighbouring distinct time factors of the variants (0 for one factor) -- a
    segment's hits may sit a rung from its majority rung, and a play one rung off drifts by h / 65536 bins per warped frame.
    Clamped so that the candidate of an edge zone, 2 (tol + drift_bins) + 1 bins, stays within the 4,096 of the moments."""
    t_max = int(np.max(np.asarray(time_factors, np.int64)))
    L = -(-(int(window_frames) + int(margin_frames)) * t_max // 65536)
    return max(0, min(-(-L * _rung(time_factors) // 65536), (4096 - 1) // 2 - int(tol)))


def _play_stage(ctx, table, pcm, off, first, wf, sf, fs, hop, res, win_off, fit, pcm_device):
    """The plays stage of scan(extents="fit"): the timeline of the scan just run (fit["timeline"](res, win_off, step) ->
    (segments, t16, f16): the fold and every segment's own Q16 pair), then ONE Context.scan_plays on the same audio."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE
    seg, t16, f16 = fit["timeline"](res, win_off, sf)
    margin = wf if fit["margin_seconds"] is None else max(0, int(round(float(fit["margin_seconds"]) * fs / hop)))
    drift = fit["drift_bins"]
    if drift is None:
        drift = default_drift_bins(wf, margin, fit["time_factors"](res), ctx.vote_tolerance)
    zone, work, ms = ctx.scan_plays(table, pcm, off, first, wf, sf, dict(seg, t16=t16, f16=f16), margin, int(drift), fs=fs,
                                    amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, pcm_device=pcm_device)
    return dict(segments=seg, t16=t16, f16=f16, zones=zone, work=work, ms=ms, margin_frames=margin, drift_bins=int(drift))


def _play_keys(w, i, tempo_key):
    """What extents="fit" adds to segment i.  Zone results are in WARPED recording frames; extent.own_frames
    maps them back with the segment's own time factor, and the result is clipped to the zone."""
    from .extent import dense_span, line_fit, own_frames, tempo_of
    p = w["plays"]
    zone, t16 = p["zones"], int(p["t16"][i])
    hop, fs = w["hop"], w["fs"]
    z = {k: [int(x) for x in zone[k][i]] for k, _ in _ffi.PLAY_ZONE_FIELDS}       # [whole, head, tail] of every field
    wlo = [(lo * t16 + 32768) >> 16 for lo in z["lo"]]
    whi = [(hi * t16 + 32768) >> 16 for hi in z["hi"]]
    secs = lambda frame: round(frame * hop / fs, 5)                              # noqa: E731  (as _segment converts)
    song_secs = lambda frame: round(float(frame) / DEFAULT_FS * hop, 5)          # noqa: E731  (as offset_seconds converts)
    clip = lambda f, k: min(max(f, z["lo"][k]), z["hi"][k])                      # noqa: E731
    d = {"play_first_frame": None, "play_last_frame": None}
    if z["count"][1]:
        span = dense_span(zone["hist"][i, 1], z["shift"][1])
        start = z["q_first"][1] if span is None else wlo[1] + span[0]             # the first warped frame of the play
        d["play_start_seconds"] = secs(clip(own_frames(start, start, t16)[0], 1))
        d["play_first_frame"] = own_frames(z["q_first"][1], z["q_first"][1], t16)[0]
    if z["count"][2]:
        span = dense_span(zone["hist"][i, 2], z["shift"][2])
        last = z["q_last"][2] if span is None else min(wlo[2] + span[1], whi[2]) - 1   # its last warped frame
        d["play_end_seconds"] = secs(clip(own_frames(last, last, t16)[1] + 1, 2))
        d["play_last_frame"] = own_frames(z["q_last"][2], z["q_last"][2], t16)[1]
    some = z["count"][0] > 0
    fit = {k: z[k][0] for k in ("count", "sum_q", "sum_u", "sum_qq", "sum_qu", "d_lo")}
    line = line_fit(**fit)
    d.update(song_start_seconds=song_secs(z["t_first"][0]) if some else None,
             song_end_seconds=song_secs(z["t_last"][0] + 1) if some else None,
             pairs=z["count"][0], extent_hist=zone["hist"][i, 0].copy(), extent_shift=z["shift"][0], extent_lo=z["lo"][0], fit=fit)
    d[tempo_key] = None if line is None else float(tempo_of(t16, line[0]))
    return d


def _segment(db, w, seg, i):
    """What a segment of either timeline says: the song, the span of its windows in the recording (the last window's end
    clipped to the recording's), how many of them named the song and their best aligned count."""
    from . import SONG_ID, SONG_NAME
    r, first, last = int(seg["rec"][i]), int(seg["first"][i]), int(seg["last"][i])
    hop, fs, sf, wf = w["hop"], w["fs"], w["step_frames"], w["window_frames"]
    end_frame = min(last * sf + wf, int(w["frames"][r]))
    return {
        SONG_ID: int(seg["sid"][i]),
        SONG_NAME: db.get_song_by_id(int(seg["sid"][i])).get(SONG_NAME, None).encode("utf8"),
        "start_seconds": round(first * sf * hop / fs, 5),
        "end_seconds": round(end_frame * hop / fs, 5),
        "windows": int(seg["hits"][i]),
        "hashes_aligned": int(seg["best"][i]),
    }


@takes_key_cap(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
@takes_song_filter(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
@takes_delta_tol(lambda *a, **k: (k["db"] if "db" in k else a[1]).ctx)
def scan(recordings, db, Fs: int = 44100, window_seconds: float = 5, step_seconds: float = 1, topn: int = TOPN,
         resample_to: int = None, min_aligned: int = 20, max_gap: int = 1, speeds=None, shift_tol: int = None, rung_tol: int = 1,
         tempos=None, pitches=None, warps=None, search: str = "grid", tempo_tol: int = None, pitch_tol: int = None,
         extents=False, margin_seconds: float = None, drift_bins: int = None, min_score: float = None):
    """The timeline of every recording: a list (per recording) of segments, each a dict with song_id, song_name,
    start_seconds / end_seconds (the span of the segment's windows in the recording, the last window's end clipped to the
    recording's), offset_seconds (the position in the song at the segment's start: align_matches' formula,
    recognizer.py:318, with the context's hop), shift (song frame - recording frame), windows (how many of the segment's
    windows named the song) and hashes_aligned (the best aligned count among them).  A window counts when its best
    candidate has at least min_aligned aligned hashes; windows of one song at one shift, at most max_gap non-hit windows
    apart, form a segment (shz_scan_timeline).
    speeds (a Q16 ladder, or True for speed_ladder()): the recording may play faster or slower than the table's copies.
    Windows are matched at every rung, and a segment is a run of hits of one song whose neighbours are at most max_gap
    windows apart, chose rungs at most rung_tol apart and whose song positions advance by the warped step within shift_tol
    frames (shz_scan_timeline_speeds; there is no constant shift, so no "shift" key).  A segment then carries "speed" (the
    rung its hits chose most often, as a float), "speed_fit" ((pos_last - pos_first) / ((last - first) * step_frames), None
    for a one-hit segment), "offset_seconds" / "offset_end_seconds" (the song position at the start of its first / last hit
    window, in the TABLE's seconds) and "pos_first" / "pos_last" (the same in the table's frames).  shift_tol=None: 2.
    tempos / pitches / warps / search (as in scan_windows; ValueError together with speeds=): tempo and pitch may have moved
    by factors of their own.  A segment is a run of hits of one song whose neighbours are at most max_gap windows apart, chose
    tempo factors at most tempo_tol and pitch factors at most pitch_tol apart (Q16; None: one rung each, the largest gap
    between neighbouring distinct values of the respective list of the variants) and whose song positions advance by the step
    warped with the TEMPO factor within shift_tol frames (shz_scan_timeline_warps; None: WARP_SHIFT_TOL).  It carries what a
    speed scan's segment carries, with "tempo" and "pitch" (the pair its hits chose most often, as floats) and "tempo_fit" in
    place of "speed" and "speed_fit".
    delta_tol= (keyword): the vote tolerance in offset bins while the call runs (Context.tolerance); None: the context's.
    songs= / exclude= (keywords, song ids): the windows are matched within / without these songs (Context.songs,
    scan_windows): exclude=[a station's jingles] leaves their segments out of the timeline.
    max_key_rows= (keyword): the key cap while the call runs (Context.key_cap, scan_windows); None: the context's.
    extents=True (the plain scan only: ValueError with speeds=, tempos=, pitches=, warps= or another search;
    NotImplementedError on a sharded table): start_seconds / end_seconds are only as fine as the windows, so every segment also
    says where its aligned hashes really lie (shz_scan_extents, DESIGN.md 3.7l: the extent pass on three zones of the
    recording -- the whole play, its head and its tail, each widened by margin_seconds; None: one window -- at the call's
    tolerance, inside the same library call).  Every key above keeps its value; a segment gains play_start_seconds /
    play_end_seconds (the first / last bucket of the head / tail zone's histogram that holds extent.DENSE_MIN_COUNT pairs,
    the end clipped to the zone's; without such a bucket the zone's first / last pair; without a pair start_seconds /
    end_seconds), play_first_frame / play_last_frame (the first pair of the head zone, the last of the tail zone, in recording
    frames; None without a pair), song_start_seconds / song_end_seconds (the span of the whole play's pairs in the song,
    converted as offset_seconds; None without a pair), pairs (their number), extent_hist / extent_shift / extent_lo (their
    histogram over the whole-play zone, which starts at recording frame extent_lo).
    extents="fit" (with speeds=, or with tempos= / pitches= / warps= and either search; ValueError without a ladder: use
    extents=True; NotImplementedError on a sharded table): the same refinement for a warped scan, and the tempo the play
    really runs at (shz_scan_plays).  The scan and its timeline run exactly as without it; then ONE library
    call on the same prepared audio warps the frames of every play at the play's own pair, cuts the three zones and runs the
    extent pass with the moments, the candidate of every zone widened by drift_bins offset bins (None:
    default_drift_bins) beside the call's tolerance.  Every key above keeps its value; a segment gains play_start_seconds /
    play_end_seconds (dense_span on the head / tail zone's histogram, which counts WARPED frames; the frame goes through
    extent.own_frames with the segment's time factor and is clipped to the zone; the fallbacks of extents=True),
    play_first_frame / play_last_frame (own recording frames), song_start_seconds / song_end_seconds, pairs (of the whole
    play), extent_hist / extent_shift / extent_lo (bucket b of the whole-play zone holds the warped frames W(extent_lo) + [b <<
    shift, (b + 1) << shift), W with the segment's time factor), fit (count, the four sums and d_lo of the whole play:
    extent.line_fit's arguments) and play_tempo (extent.tempo_of on the fitted slope, as a float; None without a fit) -- under
    speeds= the key is play_speed.
    min_score (the plain scan, with or without extents=True; ValueError with a ladder): a window counts only if its best
    candidate ALSO scores at least min_score -- shazam_amd.floor.score of its aligned count against the window's own song
    histogram (scan_windows(floor=True)), a heuristic measured on synthetic audio only.  A window whose
    score is None (nothing to compare against) counts: min_aligned alone decides there.  The windows below it have their
    nres cleared before the timeline.  With extents=True, whose timeline is folded inside the library call, the windows are
    scanned once with the floor on and the extent call then runs with a keep mask of them (SHZ_SCAN_KEEP_MASK): two scans.
    None, the default: no such test, the call as it always was."""
    from . import OFFSET_SECS
    if min_score is not None:
        if speeds is not None or tempos is not None or pitches is not None or warps is not None or search != "grid":
            raise ValueError("min_score takes the plain scan: not with speeds=, tempos=, pitches=, warps= or another search")
    ladder = speeds is not None or tempos is not None or pitches is not None or warps is not None or search != "grid"
    fit = None
    if isinstance(extents, str):
        if extents != "fit":
            raise ValueError('extents is False, True or "fit"')
        if not ladder:
            raise ValueError('extents="fit" refines a warped scan (speeds=, tempos=, pitches=, warps=): use extents=True')
        fit = dict(margin_seconds=margin_seconds, drift_bins=drift_bins)
    elif extents:
        if ladder:
            raise ValueError('extents=True takes the plain scan: a warped scan takes extents="fit" (DESIGN.md 3.7n)')
        return _scan_extents(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, margin_seconds,
                             min_score)
    if tempos is not None or pitches is not None or warps is not None or search != "grid":
        if speeds is not None:
            raise ValueError("speeds= is one factor for time and frequency: it excludes tempos=, pitches= and warps=")
        return _scan_warps(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap,
                           dict(tempos=tempos, pitches=pitches, warps=warps, search=search), tempo_tol, pitch_tol,
                           WARP_SHIFT_TOL if shift_tol is None else shift_tol, fit)
    shift_tol = 2 if shift_tol is None else shift_tol
    if speeds is not None:
        return _scan_speeds(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, speeds,
                            shift_tol, rung_tol, fit)
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, floor=min_score is not None)
    nres = w["nres"]
    if min_score is not None:      # windows below the score are cleared before the timeline, which stays as it is
        from .floor import keep_windows
        nres = keep_windows(nres, w["aligned"], w["song_hist"], float(min_score))
    seg = _ffi.scan_timeline(w["win_off"], w["sid"], w["delta"], w["aligned"], nres, w["step_frames"], min_aligned, max_gap)
    out = [[] for _ in range(len(w["frames"]))]
    for i in range(len(seg["rec"])):
        first, shift = int(seg["first"][i]), int(seg["shift"][i])
        out[int(seg["rec"][i])].append(dict(
            _segment(db, w, seg, i),
            **{OFFSET_SECS: round(float(shift + first * w["step_frames"]) / DEFAULT_FS * w["hop"], 5), "shift": shift}))
    return out


def _scan_extents(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, margin_seconds,
                  min_score=None):
    from . import OFFSET_SECS
    from .extent import dense_span
    keep = None
    if min_score is not None:      # the windows judged on a scan with the floor on; the extent call keeps the rest
        from .floor import keep_windows
        f = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, floor=True)
        keep = (keep_windows(f["nres"], f["aligned"], f["song_hist"], float(min_score)) > 0) | (f["nres"] == 0)
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to,
                     _extents=dict(min_aligned=int(min_aligned), max_gap=int(max_gap), margin_seconds=margin_seconds, keep=keep))
    seg, zone = w["segments"], w["zones"]
    hop, fs = w["hop"], w["fs"]
    secs = lambda frame: round(frame * hop / fs, 5)                              # noqa: E731  (as _segment converts)
    song_secs = lambda frame: round(float(frame) / DEFAULT_FS * hop, 5)          # noqa: E731  (as offset_seconds converts)
    out = [[] for _ in range(len(w["frames"]))]
    for i in range(len(seg["rec"])):
        first, shift = int(seg["first"][i]), int(seg["shift"][i])
        d = dict(_segment(db, w, seg, i),
                 **{OFFSET_SECS: round(float(shift + first * w["step_frames"]) / DEFAULT_FS * hop, 5), "shift": shift})
        z = {k: [int(x) for x in zone[k][i]] for k in _ffi.ZONE_FIELDS}          # [whole, head, tail] of every field
        d["play_start_seconds"], d["play_end_seconds"] = d["start_seconds"], d["end_seconds"]
        d["play_first_frame"] = d["play_last_frame"] = None
        if z["count"][1]:
            span = dense_span(zone["hist"][i, 1], z["shift"][1])
            d["play_start_seconds"] = secs(z["q_first"][1] if span is None else z["lo"][1] + span[0])
            d["play_first_frame"] = z["q_first"][1]
        if z["count"][2]:
            span = dense_span(zone["hist"][i, 2], z["shift"][2])
            d["play_end_seconds"] = secs(z["q_last"][2] + 1 if span is None else min(z["lo"][2] + span[1], z["hi"][2]))
            d["play_last_frame"] = z["q_last"][2]
        some = z["count"][0] > 0
        d.update(song_start_seconds=song_secs(z["t_first"][0]) if some else None,
                 song_end_seconds=song_secs(z["t_last"][0] + 1) if some else None,
                 pairs=z["count"][0], extent_hist=zone["hist"][i, 0].copy(), extent_shift=z["shift"][0], extent_lo=z["lo"][0])
        out[int(seg["rec"][i])].append(d)
    return out


def _scan_speeds(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, speeds, shift_tol,
                 rung_tol, fit=None):
    from . import OFFSET_SECS
    sp = _ladder(speeds)

    def timeline(res, win_off, sf):
        return _ffi.scan_timeline_speeds(win_off, res["sid"], res["delta"], res["aligned"], res["nres"], res["best"], sf, sp,
                                         min_aligned, max_gap, rung_tol, shift_tol)
    if fit is not None:
        def fold(res, win_off, sf):
            seg = timeline(res, win_off, sf)
            return seg, sp[seg["rung"]], sp[seg["rung"]]
        fit = dict(fit, timeline=fold, time_factors=lambda res: sp)
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, speeds=speeds, _fit=fit)
    seg = w["plays"]["segments"] if fit is not None else timeline(w, w["win_off"], w["step_frames"])
    hop, sf = w["hop"], w["step_frames"]
    out = [[] for _ in range(len(w["frames"]))]
    for i in range(len(seg["rec"])):
        first, last = int(seg["first"][i]), int(seg["last"][i])
        p0, p1 = int(seg["pos_first"][i]), int(seg["pos_last"][i])
        out[int(seg["rec"][i])].append(dict(_segment(db, w, seg, i), **{
            OFFSET_SECS: round(float(p0) / DEFAULT_FS * hop, 5),
            "offset_end_seconds": round(float(p1) / DEFAULT_FS * hop, 5),
            "pos_first": p0,
            "pos_last": p1,
            "first_window": first,
            "last_window": last,
            "speed": float(sp[int(seg["rung"][i])]) / 65536.0,
            "speed_fit": (p1 - p0) / float((last - first) * sf) if last > first else None,
        }))
        if fit is not None:
            d = out[int(seg["rec"][i])][-1]
            d.update(dict(play_start_seconds=d["start_seconds"], play_end_seconds=d["end_seconds"]), **_play_keys(w, i, "play_speed"))
    return out


def _scan_warps(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, variants, tempo_tol,
                pitch_tol, shift_tol, fit=None):
    from . import OFFSET_SECS

    def timeline(res, win_off, sf):
        t16, f16 = res["warps"]
        return _ffi.scan_timeline_warps(win_off, res["sid"], res["delta"], res["aligned"], res["nres"], res["best"], sf, t16, f16,
                                        min_aligned, max_gap, _rung(t16) if tempo_tol is None else int(tempo_tol),
                                        _rung(f16) if pitch_tol is None else int(pitch_tol), shift_tol)
    if fit is not None:
        def fold(res, win_off, sf):
            seg = timeline(res, win_off, sf)
            return seg, res["warps"][0][seg["warp"]], res["warps"][1][seg["warp"]]
        fit = dict(fit, timeline=fold, time_factors=lambda res: res["warps"][0])
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, _fit=fit, **variants)
    t16, f16 = w["warps"]
    seg = w["plays"]["segments"] if fit is not None else timeline(w, w["win_off"], w["step_frames"])
    hop, sf = w["hop"], w["step_frames"]
    out = [[] for _ in range(len(w["frames"]))]
    for i in range(len(seg["rec"])):
        first, last = int(seg["first"][i]), int(seg["last"][i])
        p0, p1 = int(seg["pos_first"][i]), int(seg["pos_last"][i])
        out[int(seg["rec"][i])].append(dict(_segment(db, w, seg, i), **{
            OFFSET_SECS: round(float(p0) / DEFAULT_FS * hop, 5),
            "offset_end_seconds": round(float(p1) / DEFAULT_FS * hop, 5),
            "pos_first": p0,
            "pos_last": p1,
            "first_window": first,
            "last_window": last,
            "tempo": float(t16[int(seg["warp"][i])]) / 65536.0,
            "pitch": float(f16[int(seg["warp"][i])]) / 65536.0,
            "tempo_fit": (p1 - p0) / float((last - first) * sf) if last > first else None,
        }))
        if fit is not None:
            d = out[int(seg["rec"][i])][-1]
            d.update(dict(play_start_seconds=d["start_seconds"], play_end_seconds=d["end_seconds"]), **_play_keys(w, i, "play_tempo"))
    return out
