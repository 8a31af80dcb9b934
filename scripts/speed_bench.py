#!/usr/bin/env python3
"""speed_bench.py -- speed-tolerant recognition (recognize_speeds: the peaks once, every factor of a ladder warped, hashed and
matched on the device) against the length of the ladder, beside the plain fused call on the same queries.

    python scripts/speed_bench.py [--songs 2000] [--seconds 10] [--ladders 1,11,101] [--queries 1,200] [--reps 5] [--out TAG]

Table: --songs x 30 s music-like tracks.  Queries: --seconds cut from table songs on the device (query i is song
(97 i) % songs from a start that is not hop-aligned), read back once; they play at the table's speed, so the rung 65536
finds them and every other rung is work that finds nothing -- what a monitor pays for a ladder.
For every query count and every ladder length K (K rungs at the default step around 65536): wall milliseconds per query of
recognize_speeds (the median, smallest and largest of --reps runs after one warm-up), the device times of its three stages, and how often
the top answer is the right song and the chosen rung is 65536.  For scale: recognize_batch(fused=True) on the same queries, the code path of the
library before it had a ladder.  Prints one JSON line; --out TAG also writes it to profiles/TAG_speed_bench.json."""
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

FS = 44100
SONG_S = 30


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


def build_queries(ctx, n_songs, n_queries, seconds):
    from shazam_amd import _ffi
    n = seconds * FS
    buf = ctx.alloc(n * 2)
    qs, truth = [], []
    for i in range(n_queries):
        song, start = (97 * i) % n_songs, 2048 * 40 + 555 + 31 * i
        ctx.check(_ffi.lib().shz_synth_corpus(ctx.h, 1, 77, song, 1, n, 3000, 100, 1500, start, _ffi.vp(buf.ptr)))
        qs.append(buf.download(np.int16, n))
        truth.append(song + 1)
    buf.free()
    return qs, truth


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out, [float(min(t)), float(max(t))]


def ladder_of(k):
    from shazam_amd.speed import DEFAULT_STEP_Q16
    return (65536 + DEFAULT_STEP_Q16 * (np.arange(k) - k // 2)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--ladders", default="1,11,101")
    ap.add_argument("--queries", default="1,200")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_speed_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    counts = [int(x) for x in a.queries.split(",")]
    ladders = [int(x) for x in a.ladders.split(",")]
    qs_all, truth_all = build_queries(ctx, a.songs, max(counts), a.seconds)
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()),
           "query_seconds": a.seconds, "step_q16": int(ladder_of(3)[2] - ladder_of(3)[1]), "runs": []}
    for nq in counts:
        qs, truth = qs_all[:nq], truth_all[:nq]
        t_plain, (r_plain, tm_plain), mm = timed(lambda: S.recognize_batch(qs, db, topn=1, fused=True), a.reps)
        row = {"queries": nq,
               "fused_plain": {"ms_per_query": 1e3 * t_plain / nq, "ms_per_query_min_max": [1e3 * x / nq for x in mm],
                               "ms_extract": 1e3 * tm_plain["fingerprint_time"], "ms_match": 1e3 * tm_plain["query_time"],
                               "top1_right": float(np.mean([bool(r) and r[0]["song_id"] == s for r, s in zip(r_plain, truth)]))},
               "ladders": []}
        for k in ladders:
            lad = ladder_of(k)
            t, (r, tm), mm = timed(lambda: S.recognize_speeds(qs, db, speeds=lad, topn=1), a.reps)
            row["ladders"].append({
                "rungs": k, "ms_per_query": 1e3 * t / nq, "ms_per_query_min_max": [1e3 * x / nq for x in mm],
                "ms_extract": 1e3 * tm["fingerprint_time"], "ms_warp": 1e3 * tm["warp_time"], "ms_match": 1e3 * tm["query_time"],
                "over_fused_plain": t / t_plain,
                "top1_right": float(np.mean([bool(x) and x[0]["song_id"] == s for x, s in zip(r, truth)])),
                "chose_unity": float(np.mean(lad[tm["speed_best"]] == 65536))})
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
        path = os.path.join(ROOT, "profiles", f"{a.out}_speed_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
