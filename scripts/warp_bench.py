#!/usr/bin/env python3
"""warp_bench.py -- recognition under two warp factors (recognize_warps: the peaks once, every (tempo, pitch) pair warped,
hashed and matched on the device) against the shape of the pair list, beside recognize_speeds on its default ladder.

    python scripts/warp_bench.py [--songs 2000] [--seconds 10] [--queries 1,200] [--reps 3] [--out TAG]

Table and queries: those of scripts/speed_bench.py (--songs x 30 s music-like tracks; queries cut from table songs at the
table's tempo and pitch, so the pair (65536, 65536) finds them and every other pair is work that finds nothing -- what a
monitor pays for a search).  For every query count, wall milliseconds per query (the median, smallest and largest of --reps
runs after one warm-up) and the device times of the three stages of
    tempo_only   11 tempo rungs (1 % steps) at pitch 65536
    pitch_only   the default pitch ladder at tempo 65536
    grid         every pair of the two: search="grid"
    separable    the pitch ladder, then the tempo ladder at the best pitch: search="separable"
and, for scale, recognize_speeds on the default speed ladder.  Every row is printed as it is measured; the last line is the
whole result as one JSON object; --out TAG also writes it to profiles/TAG_warp_bench.json."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from speed_bench import build_queries, build_table, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--queries", default="1,200")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_warp_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    counts = [int(x) for x in a.queries.split(",")]
    qs_all, truth_all = build_queries(ctx, a.songs, max(counts), a.seconds)
    tl, pl, sl = S.tempo_ladder(step=0.01), S.pitch_ladder(), S.speed_ladder()
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()),
           "query_seconds": a.seconds, "tempo_rungs": len(tl), "pitch_rungs": len(pl), "speed_rungs": len(sl), "runs": []}
    configs = [("tempo_only", len(tl), lambda q: S.recognize_warps(q, db, tempos=tl, topn=1)),
               ("pitch_only", len(pl), lambda q: S.recognize_warps(q, db, pitches=pl, topn=1)),
               ("separable", len(tl) + len(pl), lambda q: S.recognize_warps(q, db, tempos=tl, pitches=pl, topn=1, search="separable")),
               ("grid", len(tl) * len(pl), lambda q: S.recognize_warps(q, db, tempos=tl, pitches=pl, topn=1, search="grid")),
               ("recognize_speeds", len(sl), lambda q: S.recognize_speeds(q, db, speeds=sl, topn=1))]
    for nq in counts:
        qs, truth = qs_all[:nq], truth_all[:nq]
        for name, variants, fn in configs:
            t, (r, tm), mm = timed(lambda: fn(qs), a.reps)
            row = {"queries": nq, "search": name, "variants": variants, "ms_per_query": 1e3 * t / nq,
                   "ms_per_query_min_max": [1e3 * x / nq for x in mm], "ms_extract": 1e3 * tm["fingerprint_time"],
                   "ms_warp": 1e3 * tm["warp_time"], "ms_match": 1e3 * tm["query_time"],
                   "top1_right": float(np.mean([bool(x) and x[0]["song_id"] == s for x, s in zip(r, truth)]))}
            if name != "recognize_speeds":
                row["chose_identity"] = float(np.mean([bool(x) and (x[0]["tempo"], x[0]["pitch"]) == (1.0, 1.0) for x in r]))
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
    db.close()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_warp_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
