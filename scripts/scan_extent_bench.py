#!/usr/bin/env python3
"""scan_extent_bench.py -- what the extent stage of shz_scan_extents costs beside the scan it rides on, and what it buys.

    python scripts/scan_extent_bench.py [--songs 2000] [--recordings 4] [--seconds 120] [--window 5] [--step 1] [--out PATH]

Table: --songs x 30 s music-like tracks.  Recordings: --recordings x --seconds, assembled on the device from 20 s pieces of
table songs as scripts/scan_bench.py assembles them (piece j of recording r is song (97 r + 13 j) % songs from a start that is
not hop-aligned), read back once: both calls take the same host PCM.  The planted boundaries are the pieces' borders.
Cost: shz_scan_batch against shz_scan_extents (min_aligned 20, max_gap 1, a margin of one window, histograms on), cases
alternating, one warm-up each, then --reps runs: the median of the calls' own hipEvent times (ms_extract / ms_window /
ms_match / ms_extent) and of the wall time around the call.  extent_over_scan = ms_extent / (ms_extract + ms_window +
ms_match) of the same calls; extent_over_match = ms_extent / ms_match.
Benefit: scan(extents=True) on the same recordings; every planted piece is held against the segments of its song that
overlap it (several, where the piece's alignment falls between two offset bins): |earliest start_seconds - piece start| and
|latest end_seconds - piece end| beside the same for play_start_seconds / play_end_seconds (median, 90th percentile,
largest; pieces without a segment and segments without a piece are counted apart).
Prints one JSON line and writes it to --out (default profiles/scan_extent_bench.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_extent_bench.json"))
    a = ap.parse_args()
    import shazam_amd as S
    from scan_bench import build_recordings, build_table
    from shazam_amd.scan import seconds_to_frames
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    recs, truth = build_recordings(ctx, a.songs, a.recordings, a.seconds)
    wf, sf = seconds_to_frames(a.window, FS), seconds_to_frames(a.step, FS)
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in recs])
    pcm, first = np.concatenate(recs), np.arange(len(recs) + 1, dtype=np.uint32)
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()),
           "recordings": a.recordings, "recording_seconds": a.seconds, "window_frames": wf, "step_frames": sf,
           "margin_frames": wf, "min_aligned": a.min_aligned, "reps": a.reps}

    # ---- cost: the two calls, alternating
    def plain():
        t0 = time.perf_counter()
        _, wo, ms = ctx.scan_batch(db.table, pcm, off, first, wf, sf, topn=2, cap_windows=n_win)
        return time.perf_counter() - t0, ms + (0.0,), 0
    def extents():   # noqa: E306
        t0 = time.perf_counter()
        rc, _, _, zone, _, _, n_segs, ms = ctx.scan_extents_raw(db.table, pcm, off, first, wf, sf, a.min_aligned, 1, wf, 0, topn=2,
                                                                cap_windows=n_win, cap_segs=n_win)
        ctx.check(rc)
        return time.perf_counter() - t0, ms, n_segs
    n_win = int(ctx.scan_batch(db.table, pcm, off, first, wf, sf, topn=2)[1][-1])
    runs = {"scan_batch": [], "scan_extents": []}
    for rep in range(a.reps + 1):
        for name, fn in (("scan_batch", plain), ("scan_extents", extents)):
            r = fn()
            if rep:   # (the first round warms both up)
                runs[name].append(r)
    res["windows"] = n_win
    for name, rr in runs.items():
        ms = np.median(np.asarray([r[1] for r in rr], np.float64), axis=0)
        res[name] = {"wall_seconds": float(np.median([r[0] for r in rr])), "ms_extract": float(ms[0]), "ms_window": float(ms[1]),
                     "ms_match": float(ms[2]), "ms_extent": float(ms[3]), "segments": int(rr[-1][2])}
    e = res["scan_extents"]
    res["extent_over_scan"] = e["ms_extent"] / (e["ms_extract"] + e["ms_window"] + e["ms_match"])
    res["extent_over_match"] = e["ms_extent"] / e["ms_match"]
    res["wall_extents_over_batch"] = e["wall_seconds"] / res["scan_batch"]["wall_seconds"]

    # ---- benefit: the boundaries
    segs = S.scan(recs, db, window_seconds=a.window, step_seconds=a.step, min_aligned=a.min_aligned, extents=True)
    # a piece whose alignment falls between two offset bins comes as several segments (its windows name either shift), so the
    # boundaries of a PIECE are the earliest start and the latest end over the segments of its song that overlap it
    err = {k: [] for k in ("start_seconds", "end_seconds", "play_start_seconds", "play_end_seconds")}
    used, missed, per_piece = set(), 0, []
    for r, lst in enumerate(segs):
        for sid, t0 in truth[r]:
            t1 = min(t0 + PIECE_S, a.seconds)
            mine = [i for i, s in enumerate(lst) if s["song_id"] == sid and min(s["end_seconds"], t1) > max(s["start_seconds"], t0)]
            if not mine:
                missed += 1
                continue
            used.update((r, i) for i in mine)
            per_piece.append(len(mine))
            for k in err:
                v = [lst[i][k] for i in mine]
                err[k].append(abs(min(v) - t0) if "start" in k else abs(max(v) - t1))
    res["segments"] = int(sum(len(x) for x in segs))
    res["pieces"] = int(sum(len(t) for t in truth))
    res["pieces_without_a_segment"] = missed
    res["segments_per_piece"] = stats(per_piece)
    res["segments_without_a_piece"] = res["segments"] - len(used)
    res["boundary_error_seconds"] = {k: stats(v) for k, v in err.items()}
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
