#!/usr/bin/env python3
"""listen_speed_bench.py -- live listeners at a speed ladder (peak windows on the device: shz_listeners_push_speeds) per push
of 8192-sample chunks, beside the two things a caller could do before on the same input.

    python scripts/listen_speed_bench.py [--songs 500] [--listeners 1,64] [--ladders 1,7,21] [--window 5] [--warm 40]
                                         [--pushes 30] [--out TAG]

Table: --songs x 30 s music-like tracks.  Listener i (mono) hears song (97 i) % songs from a start that is not hop-aligned, at
the table's speed: the rung 65536 finds it and every other rung is work that finds nothing -- what a monitor pays for a
ladder.  Every path is fed --warm pushes first (the window fills), then --pushes pushes are timed; figures are the median
over those pushes, in milliseconds per push of ALL listeners.
  ladder   Listeners(peaks=True).push_speeds at K rungs: wall time, and the hipEvent times of its stages -- the streams'
           push, the window kernels with their read-back, the warp (sp_count / sp_write), the match
  plain    Listeners.push on the same chunks: the hash windows, no ladder -- the difference is the price of the ladder
  today    recognize_speeds at K rungs on the last --window seconds of every listener, buffered on the host, at every
           chunk: the audio goes up again and the whole window's STFT and peaks are redone per chunk
Prints one JSON line; --out TAG also writes it to profiles/TAG_listen_speed_bench.json."""
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
CHUNK = 8192


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


def build_signals(ctx, n_songs, n_listeners, n):
    from shazam_amd import _ffi
    buf = ctx.alloc(n * 2)
    sig, truth = [], []
    for i in range(n_listeners):
        song, start = (97 * i) % n_songs, 2048 * 40 + 555 + 31 * i
        ctx.check(_ffi.lib().shz_synth_corpus(ctx.h, 1, 77, song, 1, n, 3000, 100, 1500, start, _ffi.vp(buf.ptr)))
        sig.append(buf.download(np.int16, n))
        truth.append(song + 1)
    buf.free()
    return sig, truth


def ladder_of(k):
    from shazam_amd.speed import DEFAULT_STEP_Q16
    return (65536 + DEFAULT_STEP_Q16 * (np.arange(k) - k // 2)).astype(np.uint32)


def med(xs):
    return float(np.median(xs))


def run_listeners(ctx, db, sig, window_frames, warm, pushes, lad):
    """lad None: the hash windows; else the peak windows at that ladder.  Returns (wall ms per push, stage ms, last res)."""
    from shazam_amd import _ffi
    n = len(sig)
    st = _ffi.Streams(ctx, n)
    L = _ffi.Listeners(st, db.table, n, window_frames, peaks=lad is not None)
    wall, stages, res = [], [], None
    for p in range(warm + pushes):
        chunks = [s[p * CHUNK:(p + 1) * CHUNK] for s in sig]
        if lad is not None and p == warm:
            L.timing(True)
        t0 = time.perf_counter()
        res, _ = L.push(chunks, None, 1) if lad is None else L.push_speeds(chunks, lad, None, 1)
        dt = time.perf_counter() - t0
        if p >= warm:
            wall.append(1e3 * dt)
            if lad is not None:
                stages.append(L.timing(True))
    L.close()
    st.close()
    return wall, (np.median(np.asarray(stages), axis=0).tolist() if stages else None), res


def run_today(S, db, sig, window_samples, warm, pushes, lad):
    """the host-buffered window of every listener through recognize_speeds at every chunk"""
    wall, out = [], None
    for p in range(warm - 1, warm + pushes):           # (one untimed call first)
        hi = (p + 1) * CHUNK
        wins = [s[max(0, hi - window_samples):hi] for s in sig]
        t0 = time.perf_counter()
        out = S.recognize_speeds(wins, db, speeds=lad, topn=1)
        if p >= warm:
            wall.append(1e3 * (time.perf_counter() - t0))
    return wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=500)
    ap.add_argument("--listeners", default="1,64")
    ap.add_argument("--ladders", default="1,7,21")
    ap.add_argument("--window", type=float, default=5.0, help="window_seconds")
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_listen_speed_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    db = build_table(S, ctx, a.songs)
    counts = [int(x) for x in a.listeners.split(",")]
    ladders = [int(x) for x in a.ladders.split(",")]
    window_frames, window_samples = int(a.window * FS / 2048), int(a.window * FS)
    sig_all, truth_all = build_signals(ctx, a.songs, max(counts), (a.warm + a.pushes) * CHUNK)
    res = {"device": ctx.device_info()["name"], "songs": a.songs, "table_rows": int(db.num_fingerprints()), "chunk": CHUNK,
           "window_seconds": a.window, "window_frames": window_frames, "warm": a.warm, "pushes": a.pushes, "runs": []}
    for n in counts:
        sig, truth = sig_all[:n], np.asarray(truth_all[:n])
        wall, _, r = run_listeners(ctx, db, sig, window_frames, a.warm, a.pushes, None)
        row = {"listeners": n, "plain": {"ms_per_push": med(wall), "ms_per_push_min_max": [min(wall), max(wall)],
                                         "top1_right": float(np.mean((r["nres"] > 0) & (r["sid"][:, 0] == truth)))},
               "ladders": []}
        for k in ladders:
            lad = ladder_of(k)
            wall, stages, r = run_listeners(ctx, db, sig, window_frames, a.warm, a.pushes, lad)
            t_wall, (rt, tm) = run_today(S, db, sig, window_samples, a.warm, a.pushes, lad)
            row["ladders"].append({
                "rungs": k,
                "ladder": {"ms_per_push": med(wall), "ms_per_push_min_max": [min(wall), max(wall)],
                           "ms_streams": stages[0], "ms_window": stages[1], "ms_warp": stages[2], "ms_match": stages[3],
                           "window_hashes_per_listener": float(np.mean(r["nhash"])),
                           "top1_right": float(np.mean((r["nres"] > 0) & (r["sid"][:, 0] == truth))),
                           "chose_unity": float(np.mean(lad[r["best"]] == 65536))},
                "today": {"ms_per_push": med(t_wall), "ms_per_push_min_max": [min(t_wall), max(t_wall)],
                          "ms_extract": 1e3 * tm["fingerprint_time"], "ms_warp": 1e3 * tm["warp_time"], "ms_match": 1e3 * tm["query_time"],
                          "top1_right": float(np.mean([bool(x) and x[0]["song_id"] == s for x, s in zip(rt, truth)]))},
                "ladder_over_plain": med(wall) / row["plain"]["ms_per_push"], "today_over_ladder": med(t_wall) / med(wall)})
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
        path = os.path.join(ROOT, "profiles", f"{a.out}_listen_speed_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
