"""Scanning long recordings: "which songs play in this recording, and when?" (csrc/shz_scan.hip).

The reference recognises one recorded stretch at a time (recognizer.py:357-392).  A monitor asks the same question of every
overlapping stretch of an hour of broadcast.  Here every recording is fingerprinted ONCE; its device-resident hash list is cut
into overlapping time windows, all windows are matched together (shz_scan_batch), and the per-window answers are folded
into segments (shz_scan_timeline).

A window's hashes are a SUBSET of the whole recording's hashes -- not what fingerprinting the cut audio would give: peaks
near a cut see their neighbours beyond it, and a pair counts for the window its anchor lies in.  A recording must fit one
extraction pass (2^20 frames, about 13.5 hours at the default hop); chaining longer files is the caller's."""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._ffi import HOP

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


def scan_windows(recordings, db, Fs: int = 44100, window_seconds: float = 5, step_seconds: float = 1, topn: int = TOPN,
                 resample_to: int = None, full_sort: bool = False, speeds=None):
    """Every window of every recording matched in one library call.  recordings: 1-D int16 arrays, or lists of channels as in
    recognize_batch.  Returns a dict: the arrays of Table.match over all windows, recording-major (sid, delta, aligned, dedup
    [n_windows, topn]; nres, nhash, npairs [n_windows]), plus win_off (CSR of the windows over the recordings), frames (F_r
    of every recording), window_frames, step_frames, hop, fs (the rate the frames are counted at) and ms = (extract, window,
    match) device times.  Window w of a recording starts at frame w * step_frames; `delta` is the song frame at the window's
    start.  resample_to: the recordings are at Fs, the table at resample_to; they are resampled on the device and scanned
    there.  speeds (a Q16 ladder, or True for speed_ladder()): every window is matched at every rung (shz_scan_speeds,
    DESIGN.md 3.7d); the arrays are the best rung's, `delta` is in the TABLE's frames, and the dict gains best (rung index
    per window), profile ([n_windows, K]), speed (the chosen factor per window, float), speeds (the ladder) and ms =
    (extract, warp, window, match).  speeds=None: the plain scan, untouched."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, resample_to_device
    if not hasattr(db.table, "h"):
        raise NotImplementedError("scanning takes the unsharded table (shards=1)")
    ctx = db.ctx
    topn = int(topn)
    db.finalize()
    hop = int(getattr(ctx, "hop", HOP))
    chans, first = _flatten(recordings)
    fs = int(Fs)
    kw = dict(amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, topn=topn, full_sort=full_sort)
    if speeds is None:
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
        finally:
            buf.free()
    else:
        wf, sf = seconds_to_frames(window_seconds, fs, hop), seconds_to_frames(step_seconds, fs, hop)
        off = np.zeros(len(chans) + 1, np.uint64)
        if chans:
            off[1:] = np.cumsum([len(c) for c in chans])
        pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
        res, win_off, ms = run(db.table, pcm, off, first, wf, sf, fs=fs, **kw)
    frames = np.array([max((ctx.frames_of(int(off[c + 1] - off[c])) for c in range(int(first[r]), int(first[r + 1]))), default=0)
                       for r in range(len(first) - 1)], np.int64)
    res.update(win_off=win_off, frames=frames, window_frames=wf, step_frames=sf, hop=hop, fs=fs, ms=ms)
    if speeds is not None:
        res.update(speeds=sp, speed=sp[res["best"]].astype(np.float64) / 65536.0)
    return res


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


def scan(recordings, db, Fs: int = 44100, window_seconds: float = 5, step_seconds: float = 1, topn: int = TOPN,
         resample_to: int = None, min_aligned: int = 20, max_gap: int = 1, speeds=None, shift_tol: int = 2, rung_tol: int = 1):
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
    window, in the TABLE's seconds) and "pos_first" / "pos_last" (the same in the table's frames)."""
    from . import OFFSET_SECS
    if speeds is not None:
        return _scan_speeds(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, speeds,
                            shift_tol, rung_tol)
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to)
    seg = _ffi.scan_timeline(w["win_off"], w["sid"], w["delta"], w["aligned"], w["nres"], w["step_frames"], min_aligned, max_gap)
    out = [[] for _ in range(len(w["frames"]))]
    for i in range(len(seg["rec"])):
        first, shift = int(seg["first"][i]), int(seg["shift"][i])
        out[int(seg["rec"][i])].append(dict(
            _segment(db, w, seg, i),
            **{OFFSET_SECS: round(float(shift + first * w["step_frames"]) / DEFAULT_FS * w["hop"], 5), "shift": shift}))
    return out


def _scan_speeds(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, min_aligned, max_gap, speeds, shift_tol,
                 rung_tol):
    from . import OFFSET_SECS
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to, speeds=speeds)
    sp = w["speeds"]
    seg = _ffi.scan_timeline_speeds(w["win_off"], w["sid"], w["delta"], w["aligned"], w["nres"], w["best"], w["step_frames"], sp,
                                    min_aligned, max_gap, rung_tol, shift_tol)
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
    return out
