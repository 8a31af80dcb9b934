#!/usr/bin/env python3
"""scan_warp_bench.py -- scanning recordings whose songs were time-stretched and pitch-shifted by factors of their own
(scan_windows(tempos=, pitches=): the peaks once, every pair warped, the windows cut on the device), every window at every
pair (search="grid") against the per-window lists of the separable search (search="separable") against the only route the
library had before: every window cut from the audio and handed to recognize_warps.

    python scripts/scan_warp_bench.py [--songs 2000] [--recordings 2] [--seconds 120] [--window 5] [--step 1] [--reps 5]
                                      [--out TAG]

The table is scripts/scan_bench.py's (--songs x 30 s music-like tracks) plus 8 note songs (tests/warp_twin.notes_clip(7, c,
30)), whose renderer takes a tempo and a pitch: the recordings are --recordings x --seconds assembled from 20 s pieces of the
note songs, piece j of recording r is note song (3 r + j) % 8 from its start at the pair PAIRS[j % 6] -- tempo only, pitch
only and both.  The ladders are the defaults, tempo_ladder() x pitch_ladder() = 3 x 83 = 249 pairs.
(a) scan_windows(..., search="grid");  (b) scan_windows(..., search="separable");
(c) the BASELINE, never the new code: the same windows cut from the audio on the host through recognize_warps (grid) in
    batches of 1024 clips.
Wall seconds of each (the median, smallest and largest of --reps runs after one warm-up), the four device times and the work
counts of (a) and (b) (warped hash entries written, window entries handed to the match), how often the window's top song is
the one that plays at its middle and, for those, how often the chosen pair is within one rung of the piece's on both axes.
Prints one JSON line; --out TAG also writes it to profiles/TAG_scan_warp_bench.json."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scan_bench import FS, HOP, NFFT, PIECE_S, SONG_S, timed  # noqa: E402

PAIRS = ((1.04, 1.0), (1.0, 1.03), (1.03, 0.97), (0.96, 1.0), (1.0, 0.97), (0.97, 1.03))
NOTE_SONGS = 8


def build_table(S, ctx, n_songs):
    """scan_bench's table with the note songs behind it (song ids n_songs + 1 ..)."""
    import warp_twin as W
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
    k, t1, ho = S.fingerprint_batch([W.notes_clip(7, c, SONG_S) for c in range(NOTE_SONGS)], ctx=ctx)
    for c in range(NOTE_SONGS):
        db.insert_song(f"notes{c}", f"{n_songs + c:040x}", int(ho[c + 1] - ho[c]))
        db.set_song_fingerprinted(n_songs + c + 1)
    db.insert_clips(k, t1, ho, n_songs + 1)
    db.finalize()
    return db


def build_recordings(n_songs, n_recs, seconds):
    """Recordings of pieces of the note songs at PAIRS; returns (host arrays, [(song id, tempo, pitch)] per recording)."""
    import warp_twin as W
    recs, truth = [], []
    for r in range(n_recs):
        parts, pieces = [], []
        for j, a in enumerate(range(0, seconds, PIECE_S)):
            c, (tempo, pitch) = (3 * r + j) % NOTE_SONGS, PAIRS[j % len(PAIRS)]
            parts.append(W.notes_clip(7, c, min(PIECE_S, seconds - a), tempo, pitch))
            pieces.append((n_songs + c + 1, tempo, pitch))
        recs.append(np.concatenate(parts))
        truth.append(pieces)
    return recs, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--recordings", type=int, default=2)
    ap.add_argument("--seconds", type=int, default=120)
    ap.add_argument("--window", type=float, default=5)
    ap.add_argument("--step", type=float, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_scan_warp_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    from shazam_amd.scan import seconds_to_frames
    from shazam_amd.speed import DEFAULT_PITCH_STEP_Q16, DEFAULT_TEMPO_STEP_Q16, pitch_ladder, tempo_ladder
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    recs, truth = build_recordings(a.songs, a.recordings, a.seconds)
    wf, sf = seconds_to_frames(a.window, FS), seconds_to_frames(a.step, FS)
    tl, pl = tempo_ladder(), pitch_ladder()
    res = {"device": ctx.device_info()["name"], "songs": a.songs + NOTE_SONGS, "table_rows": int(db.num_fingerprints()),
           "recordings": a.recordings, "recording_seconds": a.seconds, "window_frames": wf, "step_frames": sf,
           "replication": -(-wf // sf), "pairs_of_the_pieces": list(PAIRS), "tempos": len(tl), "pitches": len(pl),
           "grid_pairs": len(tl) * len(pl), "reps": a.reps}

    def judge(win_off, top, t16, f16):
        """(windows that name the song at their middle, of those: chosen pair within one rung of the piece's on both axes)"""
        right = near = 0
        for r in range(a.recordings):
            for i in range(int(win_off[r]), int(win_off[r + 1])):
                mid = ((i - int(win_off[r])) * sf + wf / 2) * HOP / FS
                song, tempo, pitch = truth[r][min(int(mid // PIECE_S), len(truth[r]) - 1)]
                if top[i] == song:
                    right += 1
                    near += int(abs(int(t16[i]) - round(tempo * 65536)) <= DEFAULT_TEMPO_STEP_Q16 and
                                abs(int(f16[i]) - round(pitch * 65536)) <= DEFAULT_PITCH_STEP_Q16)
        return right, near

    tops = {}
    for search in ("grid", "separable"):
        t, w, rng = timed(lambda: S.scan_windows(recs, db, window_seconds=a.window, step_seconds=a.step, topn=1, tempos=tl,
                                                 pitches=pl, search=search), a.reps)
        win_off, n_win = w["win_off"], int(w["win_off"][-1])
        tops[search] = np.where(w["nres"] > 0, w["sid"][:, 0], 0)
        right, near = judge(win_off, tops[search], w["warps"][0][w["best"]], w["warps"][1][w["best"]])
        res[search] = {"windows": n_win, "seconds": t, "seconds_min_max": rng, "windows_per_second": n_win / t,
                       "ms_extract": w["ms"][0], "ms_warp": w["ms"][1], "ms_window": w["ms"][2], "ms_match": w["ms"][3],
                       "work_hash_entries": w["work"][0], "work_window_entries": w["work"][1],
                       "variants_tried_per_window": float(w["tried"].sum(axis=1).mean()) if n_win else None,
                       "top1_is_the_song_at_the_window_middle": right / max(n_win, 1),
                       "of_those_pair_within_one_rung": near / max(right, 1)}
    res["separable"]["top1_same_as_grid"] = float(np.mean(tops["separable"] == tops["grid"])) if n_win else None
    res["grid_over_separable"] = {"seconds": res["grid"]["seconds"] / res["separable"]["seconds"],
                                  "work_hash_entries": res["grid"]["work_hash_entries"] / max(res["separable"]["work_hash_entries"], 1),
                                  "work_window_entries": res["grid"]["work_window_entries"] / max(res["separable"]["work_window_entries"], 1)}

    # (c) the baseline: the same windows cut from the audio, through recognize_warps
    def cut_clips():
        top, t16, f16, tm = [], [], [], None
        clips = [x[i * sf * HOP:(i * sf + wf - 1) * HOP + NFFT] for r, x in enumerate(recs)
                 for i in range(int(win_off[r + 1] - win_off[r]))]
        for b0 in range(0, len(clips), 1024):
            results, tm = S.recognize_warps(clips[b0:b0 + 1024], db, tempos=tl, pitches=pl, topn=1)
            top.extend(rr[0]["song_id"] if rr else 0 for rr in results)
            t16.extend(tm["warps"][0][tm["warp_best"]].tolist())
            f16.extend(tm["warps"][1][tm["warp_best"]].tolist())
        return np.asarray(top, np.uint32), t16, f16, tm
    t_cut, (top_cut, t16, f16, tm), r_cut = timed(cut_clips, a.reps)
    right, near = judge(win_off, top_cut, t16, f16)
    res["cut_clips_recognize_warps"] = {
        "seconds": t_cut, "seconds_min_max": r_cut, "windows_per_second": n_win / t_cut,
        "ms_extract_last_batch": 1e3 * tm["fingerprint_time"], "ms_warp_last_batch": 1e3 * tm["warp_time"],
        "ms_match_last_batch": 1e3 * tm["query_time"],
        "top1_is_the_song_at_the_window_middle": right / max(n_win, 1), "of_those_pair_within_one_rung": near / max(right, 1),
        "top1_same_as_grid": float(np.mean(top_cut == tops["grid"])) if n_win else None}
    res["cut_clips_over_grid"] = t_cut / res["grid"]["seconds"]
    res["cut_clips_over_separable"] = t_cut / res["separable"]["seconds"]
    db.close()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_scan_warp_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
