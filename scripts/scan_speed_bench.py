#!/usr/bin/env python3
"""scan_speed_bench.py -- scanning recordings whose songs are pitched up or down (scan_windows(speeds=ladder): the peaks
once, every rung warped, the windows cut from the warped hash lists on the device) beside the only route the library had
before: every window cut from the audio and handed to recognize_speeds.

    python scripts/scan_speed_bench.py [--songs 2000] [--recordings 4] [--seconds 120] [--window 5] [--step 1]
                                       [--ladders 1,11,71] [--reps 5] [--out TAG]

Table and recordings as scripts/scan_bench.py has them (--songs x 30 s music-like tracks; --recordings x --seconds assembled
from 20 s pieces of table songs, piece j of recording r is song (97 r + 13 j) % songs from a start that is not hop-aligned),
except that piece j plays PITCH[j % 6] times as fast as the table's copy (linear interpolation on the host, as
tests/speed_twin.speed_up does it): +-1, 3 and 5 %.
For every ladder length K (K rungs at the default step around 65536; 71 is speed_ladder()'s +-5 %):
(a) scan_windows(recordings, speeds=ladder);
(b) the BASELINE, never the new code: the same windows cut from the audio on the host -- window w is the samples of frames
    [w step, w step + window) -- through recognize_speeds in batches of 1024 clips: the STFT and the peak pass run
    window / step times over the same audio.
Wall seconds of each (the median, smallest and largest of --reps runs after one warm-up), (b) over (a), the device times of
(a)'s four stages and (b)'s three (of its last batch), how often the window's top song is the one that plays at its middle
and, for those, how often the chosen rung is within one step of the piece's factor.  Prints one JSON line; --out TAG also
writes it to profiles/TAG_scan_speed_bench.json."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scan_bench import FS, HOP, NFFT, PIECE_S, build_table, timed  # noqa: E402

PITCH = (1.01, 0.97, 1.05, 0.99, 1.03, 0.95)


def speed_up(x, s):
    """x played s times as fast, by linear interpolation: y[n] = x(n s), rounded to int16."""
    x = np.asarray(x).astype(np.float64)
    n = int((len(x) - 1) / float(s)) + 1 if len(x) else 0
    pos = np.arange(n, dtype=np.float64) * float(s)
    return np.clip(np.rint(np.interp(pos, np.arange(len(x), dtype=np.float64), x)), -32768, 32767).astype(np.int16)


def build_recordings(ctx, n_songs, n_recs, seconds):
    """Recordings of pitched pieces of table songs; returns (host arrays, [(song id, factor)] per recording)."""
    from shazam_amd import _ffi
    n = seconds * FS
    room = int(PIECE_S * FS * max(PITCH)) + 2
    buf = ctx.alloc(room * 2)
    recs, truth = [], []
    for r in range(n_recs):
        parts, pieces = [], []
        for j, a in enumerate(range(0, n, PIECE_S * FS)):
            ln, s = min(PIECE_S * FS, n - a), PITCH[j % len(PITCH)]
            song, start, src = (97 * r + 13 * j) % n_songs, 2048 * 10 + 555 + 31 * j, int(ln * s) + 2
            ctx.check(_ffi.lib().shz_synth_corpus(ctx.h, 1, 77, song, 1, src, 3000, 100, 1500, start, _ffi.vp(buf.ptr)))
            parts.append(speed_up(buf.download(np.int16, src), s)[:ln])
            pieces.append((song + 1, s))
        recs.append(np.concatenate(parts))
        truth.append(pieces)
    buf.free()
    return recs, truth


def ladder_of(k):
    from shazam_amd.speed import DEFAULT_STEP_Q16
    return (65536 + DEFAULT_STEP_Q16 * (np.arange(k) - k // 2)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--recordings", type=int, default=4)
    ap.add_argument("--seconds", type=int, default=120)
    ap.add_argument("--window", type=float, default=5)
    ap.add_argument("--step", type=float, default=1)
    ap.add_argument("--ladders", default="1,11,71")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_scan_speed_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    from shazam_amd.scan import seconds_to_frames
    from shazam_amd.speed import DEFAULT_STEP_Q16
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    recs, truth = build_recordings(ctx, a.songs, a.recordings, a.seconds)
    wf, sf = seconds_to_frames(a.window, FS), seconds_to_frames(a.step, FS)
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()),
           "recordings": a.recordings, "recording_seconds": a.seconds, "window_frames": wf, "step_frames": sf,
           "replication": -(-wf // sf), "pitch": list(PITCH), "reps": a.reps, "ladders": []}

    def judge(win_off, top, rung, lad):
        """(windows that name the song at their middle, of those: chosen rung within one step of the piece's factor)"""
        right = near = 0
        for r in range(a.recordings):
            for i in range(int(win_off[r]), int(win_off[r + 1])):
                mid = ((i - int(win_off[r])) * sf + wf / 2) * HOP / FS
                song, s = truth[r][min(int(mid // PIECE_S), len(truth[r]) - 1)]
                if top[i] == song:
                    right += 1
                    near += int(abs(int(lad[rung[i]]) - round(s * 65536)) <= DEFAULT_STEP_Q16)
        return right, near

    for k in [int(x) for x in a.ladders.split(",")]:
        lad = ladder_of(k)
        # (a) the scan
        t_scan, w, r_scan = timed(lambda: S.scan_windows(recs, db, window_seconds=a.window, step_seconds=a.step, topn=1, speeds=lad),
                                  a.reps)
        win_off, n_win = w["win_off"], int(w["win_off"][-1])
        top_scan = np.where(w["nres"] > 0, w["sid"][:, 0], 0)
        right, near = judge(win_off, top_scan, w["best"], lad)
        row = {"rungs": k, "windows": n_win,
               "scan_speeds": {"seconds": t_scan, "seconds_min_max": r_scan, "windows_per_second": n_win / t_scan,
                               "ms_extract": w["ms"][0], "ms_warp": w["ms"][1], "ms_window": w["ms"][2], "ms_match": w["ms"][3],
                               "top1_is_the_song_at_the_window_middle": right / max(n_win, 1),
                               "of_those_rung_within_one_step": near / max(right, 1)}}

        # (b) the baseline: the same windows cut from the audio, through recognize_speeds
        def cut_clips():
            tops, rungs, tm = [], [], None
            clips = [x[i * sf * HOP:(i * sf + wf - 1) * HOP + NFFT] for r, x in enumerate(recs)
                     for i in range(int(win_off[r + 1] - win_off[r]))]
            for b0 in range(0, len(clips), 1024):
                results, tm = S.recognize_speeds(clips[b0:b0 + 1024], db, speeds=lad, topn=1)
                tops.extend(rr[0]["song_id"] if rr else 0 for rr in results)
                rungs.extend(tm["speed_best"].tolist())
            return np.asarray(tops, np.uint32), np.asarray(rungs, np.int64), tm
        t_cut, (top_cut, rung_cut, tm), r_cut = timed(cut_clips, a.reps)
        right, near = judge(win_off, top_cut, rung_cut, lad)
        row["cut_clips_recognize_speeds"] = {
            "seconds": t_cut, "seconds_min_max": r_cut, "windows_per_second": n_win / t_cut,
            "ms_extract_last_batch": 1e3 * tm["fingerprint_time"], "ms_warp_last_batch": 1e3 * tm["warp_time"],
            "ms_match_last_batch": 1e3 * tm["query_time"],
            "top1_is_the_song_at_the_window_middle": right / max(n_win, 1), "of_those_rung_within_one_step": near / max(right, 1),
            "top1_same_as_scan": float(np.mean(top_cut == top_scan)) if n_win else None}
        row["cut_clips_over_scan"] = t_cut / t_scan
        res["ladders"].append(row)
    db.close()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_scan_speed_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
