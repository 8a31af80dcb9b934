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


def scan_windows(recordings, db, Fs: int = 44100, window_seconds: float = 5, step_seconds: float = 1, topn: int = TOPN,
                 resample_to: int = None, full_sort: bool = False):
    """Every window of every recording matched in one library call.  recordings: 1-D int16 arrays, or lists of channels as in
    recognize_batch.  Returns a dict: the arrays of Table.match over all windows, recording-major (sid, delta, aligned, dedup
    [n_windows, topn]; nres, nhash, npairs [n_windows]), plus win_off (CSR of the windows over the recordings), frames (F_r
    of every recording), window_frames, step_frames, hop, fs (the rate the frames are counted at) and ms = (extract, window,
    match) device times.  Window w of a recording starts at frame w * step_frames; `delta` is the song frame at the window's
    start.  resample_to: the recordings are at Fs, the table at resample_to; they are resampled on the device and scanned
    there."""
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
    if resample_to is not None and int(resample_to) != fs:
        fs = int(resample_to)
        wf, sf = seconds_to_frames(window_seconds, fs, hop), seconds_to_frames(step_seconds, fs, hop)
        buf, off = resample_to_device(chans, int(Fs), fs, ctx)
        try:
            res, win_off, ms = ctx.scan_batch(db.table, buf, off, first, wf, sf, fs=fs, pcm_device=True, **kw)
        finally:
            buf.free()
    else:
        wf, sf = seconds_to_frames(window_seconds, fs, hop), seconds_to_frames(step_seconds, fs, hop)
        off = np.zeros(len(chans) + 1, np.uint64)
        if chans:
            off[1:] = np.cumsum([len(c) for c in chans])
        pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
        res, win_off, ms = ctx.scan_batch(db.table, pcm, off, first, wf, sf, fs=fs, **kw)
    frames = np.array([max((ctx.frames_of(int(off[c + 1] - off[c])) for c in range(int(first[r]), int(first[r + 1]))), default=0)
                       for r in range(len(first) - 1)], np.int64)
    res.update(win_off=win_off, frames=frames, window_frames=wf, step_frames=sf, hop=hop, fs=fs, ms=ms)
    return res


def scan(recordings, db, Fs: int = 44100, window_seconds: float = 5, step_seconds: float = 1, topn: int = TOPN,
         resample_to: int = None, min_aligned: int = 20, max_gap: int = 1):
    """The timeline of every recording: a list (per recording) of segments, each a dict with song_id, song_name,
    start_seconds / end_seconds (the span of the segment's windows in the recording, the last window's end clipped to the
    recording's), offset_seconds (the position in the song at the segment's start: align_matches' formula,
    recognizer.py:318, with the context's hop), shift (song frame - recording frame), windows (how many of the segment's
    windows named the song) and hashes_aligned (the best aligned count among them).  A window counts when its best
    candidate has at least min_aligned aligned hashes; windows of one song at one shift, at most max_gap non-hit windows
    apart, form a segment (shz_scan_timeline)."""
    from . import OFFSET_SECS, SONG_ID, SONG_NAME
    w = scan_windows(recordings, db, Fs, window_seconds, step_seconds, topn, resample_to)
    seg = _ffi.scan_timeline(w["win_off"], w["sid"], w["delta"], w["aligned"], w["nres"], w["step_frames"], min_aligned, max_gap)
    hop, fs, sf, wf = w["hop"], w["fs"], w["step_frames"], w["window_frames"]
    out = [[] for _ in range(len(w["frames"]))]
    for i in range(len(seg["rec"])):
        r, first, last, shift = int(seg["rec"][i]), int(seg["first"][i]), int(seg["last"][i]), int(seg["shift"][i])
        song = db.get_song_by_id(int(seg["sid"][i]))
        end_frame = min(last * sf + wf, int(w["frames"][r]))
        out[r].append({
            SONG_ID: int(seg["sid"][i]),
            SONG_NAME: song.get(SONG_NAME, None).encode("utf8"),
            "start_seconds": round(first * sf * hop / fs, 5),
            "end_seconds": round(end_frame * hop / fs, 5),
            OFFSET_SECS: round(float(shift + first * sf) / DEFAULT_FS * hop, 5),
            "shift": shift,
            "windows": int(seg["hits"][i]),
            "hashes_aligned": int(seg["best"][i]),
        })
    return out
