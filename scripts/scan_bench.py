#!/usr/bin/env python3
"""scan_bench.py -- scanning recordings (scan_windows: one extraction, all windows in one match) beside the two ways the
library had to get per-window answers.

    python scripts/scan_bench.py [--songs 2000] [--recordings 4] [--seconds 120] [--window 5] [--step 1] [--out TAG]

Table: --songs x 30 s music-like tracks.  Recordings: --recordings x --seconds, assembled on the device from 20 s pieces of
table songs (piece j of recording r is song (97 r + 13 j) % songs from a start that is not hop-aligned), read back once:
all three paths take the same host PCM.
(a) scan_windows(recordings): every recording fingerprinted once, its windows cut on the device, matched together.
(b) the same windows cut from the audio on the host -- window w is the samples of frames [w step, w step + window) -- and
    handed to recognize_batch(fused=True) in batches of 1024 clips: the STFT, peak picking and hashing run window / step
    times over the same audio.
(c) StreamRecognizer(device=True) with one listener per recording, fed in 8192-sample chunks: an answer per push.
Wall seconds of each (the median, smallest and largest of --reps runs after one warm-up; (c): one warm-up, one run), the ratios against (a), the
device times of (a)'s three stages, and how often (a) and (b) name the same top song (their hashes differ at the cuts, so
this need not be 1).  Prints one JSON line; --out TAG also writes it to profiles/TAG_scan_bench.json."""
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

FS, HOP, NFFT = 44100, 2048, 4096
SONG_S, PIECE_S = 30, 20


def build_table(S, ctx, n_songs):
    db = S.get_database("hip")(ctx=ctx)
    ln = SONG_S * FS
    for b0 in range(0, n_songs, 500):
        nb = min(500, n_songs - b0)
        pcm = ctx.synth_corpus(1, 77, b0, nb, ln)
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, np.arange(nb + 1, dtype=np.uint64) * ln, pcm_device=True)
        pcm.free()
        for c in range(nb):
            db.insert_song(f"song{b0 + c}", f"{b0 + c:040x}", int(ho[c + 1] - ho[c]))
            db.set_song_fingerprinted(b0 + c + 1)
        db.insert_clips(k, t1, ho, b0 + 1)
    db.finalize()
    return db


def build_recordings(ctx, n_songs, n_recs, seconds):
    """Recordings assembled on the device from pieces of table songs; returns (host arrays, [(song id, piece start s)])."""
    from shazam_amd import _ffi
    n = seconds * FS
    buf = ctx.alloc(n * 2)
    recs, truth = [], []
    for r in range(n_recs):
        pieces = []
        for j, a in enumerate(range(0, n, PIECE_S * FS)):
            ln = min(PIECE_S * FS, n - a)
            song, start = (97 * r + 13 * j) % n_songs, 2048 * 10 + 555 + 31 * j
            ctx.check(_ffi.lib().shz_synth_corpus(ctx.h, 1, 77, song, 1, ln, 3000, 100, 1500, start, _ffi.vp(buf.ptr + a * 2)))
            pieces.append((song + 1, a / FS))
        recs.append(buf.download(np.int16, n))
        truth.append(pieces)
    buf.free()
    return recs, truth


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out, [float(min(t)), float(max(t))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--recordings", type=int, default=4)
    ap.add_argument("--seconds", type=int, default=120)
    ap.add_argument("--window", type=float, default=5)
    ap.add_argument("--step", type=float, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_scan_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    from shazam_amd.scan import seconds_to_frames
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    recs, truth = build_recordings(ctx, a.songs, a.recordings, a.seconds)
    wf, sf = seconds_to_frames(a.window, FS), seconds_to_frames(a.step, FS)
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()),
           "recordings": a.recordings, "recording_seconds": a.seconds, "window_frames": wf, "step_frames": sf,
           "replication": -(-wf // sf)}

    # (a) the scan
    t_scan, w, r_scan = timed(lambda: S.scan_windows(recs, db, window_seconds=a.window, step_seconds=a.step, topn=1), a.reps)
    n_win = int(w["win_off"][-1])
    res["windows"] = n_win
    res["scan"] = {"seconds": t_scan, "seconds_min_max": r_scan, "ms_extract": w["ms"][0], "ms_window": w["ms"][1], "ms_match": w["ms"][2],
                   "windows_per_second": n_win / t_scan}
    top_scan = np.where(w["nres"] > 0, w["sid"][:, 0], 0)
    # how many windows name the song that plays at their middle (windows across a piece border may name either)
    right = 0
    for r in range(a.recordings):
        for i in range(int(w["win_off"][r]), int(w["win_off"][r + 1])):
            mid = ((i - int(w["win_off"][r])) * sf + wf / 2) * HOP / FS
            right += int(top_scan[i] == truth[r][min(int(mid // PIECE_S), len(truth[r]) - 1)][0])
    res["scan"]["top1_is_the_song_at_the_window_middle"] = right / max(n_win, 1)

    # (b) the same windows cut from the audio, through the fused recognise call
    def cut_clips():
        tops = []
        clips = [x[i * sf * HOP:(i * sf + wf - 1) * HOP + NFFT] for r, x in enumerate(recs)
                 for i in range(int(w["win_off"][r + 1] - w["win_off"][r]))]
        for b0 in range(0, len(clips), 1024):
            results, _ = S.recognize_batch(clips[b0:b0 + 1024], db, topn=1, fused=True)
            tops.extend(rr[0]["song_id"] if rr else 0 for rr in results)
        return np.asarray(tops, np.uint32)
    t_cut, top_cut, r_cut = timed(cut_clips, a.reps)
    res["cut_clips_fused"] = {"seconds": t_cut, "seconds_min_max": r_cut, "windows_per_second": n_win / t_cut,
                              "top1_same_as_scan": float(np.mean(top_cut == top_scan)) if n_win else None}

    # (c) the stream classes: one listener per recording, 8192-sample chunks, an answer per push
    def stream():
        rec = S.StreamRecognizer(db, a.recordings, channels=1, window_seconds=a.window, topn=1, device=True)
        n = 0
        for p in range(0, a.seconds * FS, 8192):
            rec.push([x[p:p + 8192] for x in recs])
            n += 1
        rec.close()
        return n
    t_stream, pushes, _ = timed(stream, 1)
    res["stream_device"] = {"seconds": t_stream, "pushes": pushes, "answers_per_second": pushes * a.recordings / t_stream}

    res["cut_clips_over_scan"] = t_cut / t_scan
    res["stream_over_scan"] = t_stream / t_scan
    db.close()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_scan_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
