#!/usr/bin/env python3
"""fit_bench.py -- the extent stage of warped recognition and the tempo fit from its pairs (recognize_warps(extents=True):
csrc/shz_speed.hip, csrc/shz_extent.hip, shazam_amd/extent.py), measured on the note corpus.

    python scripts/fit_bench.py [--songs 8] [--seconds 10] [--tempos 0.97,0.98,0.99,1.01,1.02,1.03] [--reps 5] [--out FILE.json]

Table: --songs x 30 s of the note corpus (tests/warp_twin.py: notes_clip(7, c, 30)).  Queries: for every song and every true
tempo of --tempos, --seconds from the song's second 8 RENDERED at that tempo (pitch 1) -- not made by the code under test.
The true tempos lie off the rungs of the default tempo ladder (0.958, 1.0, 1.042: DEFAULT_TEMPO_STEP_Q16), which is the
search: recognize_warps(tempos=tempo_ladder(), extents=True), drift_bins at its default.
Reported: the device times of the stages (ms_extract, ms_warp, ms_match, ms_extent: the median of --reps calls after one
warm-up, all queries in one call) and the same call without extents; over the queries whose top answer is the right song,
|tempo_fit - true| beside |rung - true| -- the median and the worst of each -- per true tempo and over all, the share of
queries without a fit and the share with the wrong song.  No bar is set: the numbers are what DESIGN.md 3.7m quotes.
Prints one JSON line; --out (default profiles/fit_bench.json) also writes it."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FS, SONG_S, CUT_S = 44100, 30, 8


def render(W, song, tempo, seconds):
    """`seconds` of song `song` from its second 8, heard at `tempo` (tests/test_gpu_warp_recognize.py: _render)"""
    x = W.notes_clip(7, song, CUT_S / tempo + seconds + 0.1, tempo, 1.0)
    s0 = int(round(CUT_S / tempo * FS))
    return x[s0:s0 + int(seconds * FS)]


def stats(x):
    x = np.asarray(x, float)
    return {"n": int(len(x))} if len(x) == 0 else {"n": int(len(x)), "median": float(np.median(x)), "worst": float(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--tempos", default="0.97,0.98,0.99,1.01,1.02,1.03")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.json"))
    a = ap.parse_args()
    import shazam_amd as S
    import warp_twin as W
    ctx = S.get_context(0)
    songs = [W.notes_clip(7, c, SONG_S) for c in range(a.songs)]
    db = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    for c in range(a.songs):
        db.insert_song(f"song{c}", f"{c:040x}", int(ho[c + 1] - ho[c]))
        db.set_song_fingerprinted(c + 1)
    db.table.insert_clips(k, t1, ho, 1)
    db.finalize()
    true = [float(x) for x in a.tempos.split(",")]
    queries, truth = [], []
    for c in range(a.songs):
        for tempo in true:
            queries.append(render(W, c, tempo, a.seconds))
            truth.append((c + 1, tempo))
    tl = S.tempo_ladder()
    with_ext = lambda: S.recognize_warps(queries, db, tempos=tl, topn=1, extents=True)
    without = lambda: S.recognize_warps(queries, db, tempos=tl, topn=1)
    ms = {"extents": {n: [] for n in ("fingerprint_time", "warp_time", "query_time", "extent_time")},
          "plain": {n: [] for n in ("fingerprint_time", "warp_time", "query_time")}}
    with_ext(), without()
    for _ in range(a.reps):   # (the two cases alternate)
        _, tp = without()
        results, tm = with_ext()
        for name, t in (("plain", tp), ("extents", tm)):
            for n in ms[name]:
                ms[name][n].append(1e3 * t[n])
    short = {"fingerprint_time": "ms_extract", "warp_time": "ms_warp", "query_time": "ms_match", "extent_time": "ms_extent"}
    out = {"device": ctx.device_info()["name"], "corpus": "note corpus (tests/warp_twin.py notes_clip, seed 7)", "songs": a.songs,
           "table_rows": int(db.num_fingerprints()), "query_seconds": a.seconds, "queries": len(queries), "true_tempos": true,
           "tempo_rungs": [float(x) / 65536 for x in tl], "drift_bins": int(tm["drift_bins"]), "reps": a.reps,
           "with_extents": {short[n]: float(np.median(v)) for n, v in ms["extents"].items()},
           "without_extents": {short[n]: float(np.median(v)) for n, v in ms["plain"].items()}}
    rows, per = [], {t: [] for t in true}
    wrong = nofit = 0
    for r, (sid, tempo) in zip(results, truth):
        if not r or r[0]["song_id"] != sid:
            wrong += 1
            continue
        if r[0]["tempo_fit"] is None:
            nofit += 1
            continue
        row = (abs(r[0]["tempo_fit"] - tempo), abs(r[0]["tempo"] - tempo), r[0]["fit"]["count"])
        rows.append(row)
        per[tempo].append(row)
    out.update({"wrong_song_share": wrong / len(queries), "no_fit_share": nofit / len(queries),
                "abs_err_tempo_fit": stats([x[0] for x in rows]), "abs_err_rung": stats([x[1] for x in rows]),
                "pairs_per_fit": stats([x[2] for x in rows]),
                "per_true_tempo": [{"true": t, "abs_err_tempo_fit": stats([x[0] for x in v]), "abs_err_rung": stats([x[1] for x in v])}
                                   for t, v in per.items()]})
    db.close()
    try:
        out["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        out["commit"] = None
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
