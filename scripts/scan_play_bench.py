#!/usr/bin/env python3
"""scan_play_bench.py -- what the plays stage of a warped scan (shz_scan_plays, scan(extents="fit")) costs beside the ladder
scan it follows, what the job form saves, and what it buys at the borders and in the speed.

    python scripts/scan_play_bench.py [--songs 2000] [--recordings 4] [--seconds 120] [--window 5] [--step 1] [--out PATH]

Table and recordings as scripts/scan_speed_bench.py has them: --songs x 30 s music-like tracks; --recordings x --seconds
assembled from 20 s pieces of table songs, piece j resampled on the host to play PITCH[j % 6] times as fast (+-1, 3 and 5 %).
The planted borders are the pieces' borders, the planted factors the pieces' speeds.
Cost: scan_windows(speeds=speed_ladder()) and, on its timeline's segments, Context.scan_plays (a margin of one window, the
default drift_bins), alternating, one warm-up each, then --reps runs: the medians of the calls' own hipEvent times.  The stage's
ms_extract is the price of not fusing it into the scan call: the peaks are extracted a second time.
The job form: out_work[0], the peak items the stage warped, beside (distinct pairs the segments chose) x (the recordings' peaks),
what re-warping whole recordings at every pair in use would warp.
Benefit: scan(speeds=, extents="fit"); every planted piece is held against the segments of its song that overlap it:
|earliest start_seconds - piece start| and |latest end_seconds - piece end| beside play_start_seconds / play_end_seconds, and
|speed - planted| beside |play_speed - planted| over the segments with a fit (median, 90th percentile, largest).
Prints one JSON line and writes it to --out (default profiles/scan_play_bench.json)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FS, HOP = 44100, 2048
PIECE_S = 20


def stats(x):
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return None
    return {"median": float(np.median(x)), "p90": float(np.percentile(x, 90)), "max": float(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--recordings", type=int, default=4)
    ap.add_argument("--seconds", type=int, default=120)
    ap.add_argument("--window", type=float, default=5)
    ap.add_argument("--step", type=float, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-aligned", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_play_bench.json"))
    a = ap.parse_args()
    import shazam_amd as S
    from scan_bench import build_table
    from scan_speed_bench import build_recordings
    from shazam_amd import _ffi
    from shazam_amd.scan import default_drift_bins, seconds_to_frames
    from shazam_amd.speed import speed_ladder
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    recs, truth = build_recordings(ctx, a.songs, a.recordings, a.seconds)
    lad = speed_ladder()
    wf, sf = seconds_to_frames(a.window, FS), seconds_to_frames(a.step, FS)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in recs])
    pcm, first = np.concatenate(recs), np.arange(len(recs) + 1, dtype=np.uint32)
    drift = default_drift_bins(wf, wf, lad, ctx.vote_tolerance)
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()),
           "recordings": a.recordings, "recording_seconds": a.seconds, "window_frames": wf, "step_frames": sf, "margin_frames": wf,
           "rungs": len(lad), "drift_bins": drift, "min_aligned": a.min_aligned, "reps": a.reps}

    # ---- cost: the ladder scan and the stage on its segments, alternating
    def scan():
        w, wo, ms = ctx.scan_speeds(db.table, pcm, off, first, wf, sf, lad, topn=2)
        return w, wo, ms
    w, wo, _ = scan()
    seg = _ffi.scan_timeline_speeds(wo, w["sid"], w["delta"], w["aligned"], w["nres"], w["best"], sf, lad, a.min_aligned, 1, 1, 2)
    plays = dict(seg, t16=lad[seg["rung"]], f16=lad[seg["rung"]])
    runs = {"scan_speeds": [], "scan_plays": []}
    work = None
    for rep in range(a.reps + 1):
        m1 = scan()[2]
        _, work, m2 = ctx.scan_plays(db.table, pcm, off, first, wf, sf, plays, wf, drift)
        if rep:   # (the first round warms both up)
            runs["scan_speeds"].append(m1)
            runs["scan_plays"].append(m2)
    m1, m2 = (np.median(np.asarray(runs[k], np.float64), axis=0) for k in ("scan_speeds", "scan_plays"))
    res["windows"], res["segments"] = int(wo[-1]), int(len(seg["rec"]))
    res["scan_speeds"] = dict(zip(("ms_extract", "ms_warp", "ms_window", "ms_match"), (float(x) for x in m1)))
    res["scan_plays"] = dict(zip(("ms_extract", "ms_warp", "ms_extent"), (float(x) for x in m2)))
    res["plays_over_scan"] = float(m2.sum() / m1.sum())
    res["plays_without_extract_over_scan"] = float(m2[1:].sum() / m1.sum())
    peaks = int(ctx.peaks(pcm, off)[2][-1])
    pairs_in_use = len(set(int(x) for x in plays["t16"]))
    res["work"] = {"peak_items_warped": work[0], "hash_entries_written": work[1], "zone_entries": work[2],
                   "recordings_peaks": peaks, "pairs_in_use": pairs_in_use, "whole_recordings_at_every_pair": pairs_in_use * peaks,
                   "saving": pairs_in_use * peaks / max(work[0], 1)}

    # ---- benefit: the borders and the speed
    segs = S.scan(recs, db, window_seconds=a.window, step_seconds=a.step, min_aligned=a.min_aligned, speeds=lad, extents="fit")
    err = {k: [] for k in ("start_seconds", "end_seconds", "play_start_seconds", "play_end_seconds")}
    rung_err, fit_err, used, missed = [], [], set(), 0
    for r, lst in enumerate(segs):
        for j, (sid, s) in enumerate(truth[r]):
            t0, t1 = j * PIECE_S, min((j + 1) * PIECE_S, a.seconds)
            mine = [i for i, x in enumerate(lst) if x["song_id"] == sid and min(x["end_seconds"], t1) > max(x["start_seconds"], t0)]
            if not mine:
                missed += 1
                continue
            used.update((r, i) for i in mine)
            for k in err:
                v = [lst[i][k] for i in mine]
                err[k].append(abs(min(v) - t0) if "start" in k else abs(max(v) - t1))
            for i in mine:
                if lst[i]["play_speed"] is not None:
                    rung_err.append(abs(lst[i]["speed"] - s))
                    fit_err.append(abs(lst[i]["play_speed"] - s))
    res["pieces"] = int(sum(len(t) for t in truth))
    res["pieces_without_a_segment"] = missed
    res["segments_without_a_piece"] = int(sum(len(x) for x in segs)) - len(used)
    res["boundary_error_seconds"] = {k: stats(v) for k, v in err.items()}
    res["speed_error"] = {"segments_with_a_fit": len(fit_err), "rung": stats(rung_err), "play_speed": stats(fit_err)}
    db.close()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
