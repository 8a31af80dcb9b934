#!/usr/bin/env python3
"""recognize_bench.py -- the fused recognise call and the device-resident listeners beside the paths they join.

    python scripts/recognize_bench.py [--songs 2000] [--stream-songs 10000] [--listeners 1,64,1024] [--out FILE.json]

(a) the table, query and loop of scripts/single_query_latency.py (--songs x 30 s tonal songs, one 5 s crop, host PCM in,
    result dicts out, 3 warm-up + 50 timed calls): recognize() and recognize(fused=True), total / fingerprint / match ms
    p50 / p99 of each.  fingerprint / match of the fused call are device times (hipEvents), of the two-call path host times.
(b) N mono listeners (and one stereo listener, the case of scripts/stream_bench.py) in 8192-sample chunks against the
    --stream-songs x 10 s music table of stream_bench.py, StreamRecognizer(device=False) and (device=True): push +
    recognise ms p50 / p99 over the pushes of 8 s of audio, the first pass of each recogniser being the warm-up.
Prints one JSON line; --out also writes it to a file (profiles/<tag>_recognize_bench.json)."""
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


def pct(v, q):
    return float(np.percentile(np.asarray(v, np.float64), q))


def single_query(S, ctx, songs):
    db = S.get_database("hip")(ctx=ctx)
    n = 30 * 44100
    for c0 in range(0, songs, 500):
        nc = min(500, songs - c0)
        pcm = ctx.synth_pcm(4321, c0, nc, n, 4000, 1500)
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, np.arange(nc + 1, dtype=np.uint64) * n, pcm_device=True)
        pcm.free()
        for i in range(nc):
            db.songs[c0 + i + 1] = {"song_name": str(c0 + i), "file_sha1": "00", "total_hashes": int(ho[i + 1] - ho[i]),
                                    "fingerprinted": 1, "date_created": None}
        db.insert_clips(k, t1, ho, c0 + 1)
    db.finalize()
    trk = ctx.synth_pcm(4321, 7, 1, n, 4000, 1500)
    q = trk.download(np.int16, n)[13 * 2048 + 77:13 * 2048 + 77 + 5 * 44100].copy()
    trk.free()
    out = {"songs": songs, "table_rows": int(db.num_fingerprints())}
    results = {}
    for name, fused in (("two_call", False), ("fused", True)):
        for _ in range(3):
            S.recognize(q, db=db, fused=fused)
        lat = {"fingerprint": [], "match": [], "total": []}
        s0 = ctx.spec_stats()
        for _ in range(50):
            t0 = time.perf_counter()
            res, tf, tq, ta = S.recognize(q, db=db, fused=fused)
            lat["total"].append(time.perf_counter() - t0)
            lat["fingerprint"].append(tf)
            lat["match"].append(tq)
        s1 = ctx.spec_stats()
        results[name] = res
        out[name] = {f"{k}_ms_p{p}": pct(np.array(v) * 1e3, p) for k, v in lat.items() for p in (50, 99)}
        out[name]["fold_queued"], out[name]["fold_used"] = s1[0] - s0[0], s1[1] - s0[1]
        out[name]["top1"] = [res[0]["song_id"], res[0]["offset"]] if res else None
    out["same_results"] = results["two_call"] == results["fused"]
    db.close()
    return out


def stream_table(S, ctx, n_songs, song_s=10, fs=44100):
    db = S.get_database("hip")(ctx=ctx)
    ln = song_s * fs
    for b0 in range(0, n_songs, 1000):
        nb = min(1000, n_songs - b0)
        pcm = ctx.synth_corpus(1, 77, b0, nb, ln)
        ok, ot = ctx.alloc(nb * 8000 * 4), ctx.alloc(nb * 8000 * 4)
        _, _, ho, cnt = ctx.fingerprint_batch(pcm.ptr, np.arange(nb + 1, dtype=np.uint64) * ln, pcm_device=True,
                                              out_key=ok, out_t1=ot)
        for c in range(nb):
            db.insert_song(f"song{b0 + c}", f"{b0 + c:040x}", int(ho[c + 1] - ho[c]))
        db.insert_clips(ok.ptr, ot.ptr, ho, b0 + 1, device=True)
        for x in (pcm, ok, ot):
            x.free()
    db.finalize()
    return db


def listeners(S, ctx, db, n_songs, n, channels, fs=44100, seconds=8):
    """n listeners of `channels` channels: listener l hears song (1234 + 7 l) % n_songs from a start that is not
    hop-aligned, under traffic noise at 10 dB (the listener of stream_bench.py is l = 0)."""
    from oracle import synth
    from shazam_amd import harness
    length = seconds * fs
    distinct = min(n, 16)                     # (the PCM of 16 listeners, heard by all: synthesis is not what is measured)
    base = []
    for l in range(distinct):
        start = 2048 * 37 + 555 + 97 * l
        clean = synth.music_clip(77, (1234 + 7 * l) % n_songs, start + length)[start:]
        base.append([harness.mix(clean, synth.traffic_noise(5, 2 * l + c, length), 10) for c in range(channels)])
    out = {"listeners": n, "channels": channels, "chunk_samples": 8192, "pushes": len(range(0, length, 8192))}
    last = {}
    for name, device in (("host_window", False), ("device_window", True)):
        lat = []
        for rep in range(2):   # the first pass warms up
            rec = S.StreamRecognizer(db, n, channels=channels, window_seconds=5, device=device)
            lat = []
            for a in range(0, length, 8192):
                chunks = [[c[a:a + 8192] for c in base[l % distinct]] for l in range(n)]
                t0 = time.perf_counter()
                res = rec.push(chunks)
                lat.append((time.perf_counter() - t0) * 1e3)
            rec.close()
        last[name] = res
        out[name] = {"push_recognise_ms_p50": pct(lat, 50), "push_recognise_ms_p99": pct(lat, 99),
                     "push_recognise_ms_max": float(max(lat))}
    out["same_results"] = last["host_window"] == last["device_window"]
    out["top1_correct_last"] = bool(last["device_window"][0][0]) and last["device_window"][0][0][0]["song_id"] == 1234 % n_songs + 1
    out["host_over_device_p50"] = out["host_window"]["push_recognise_ms_p50"] / out["device_window"]["push_recognise_ms_p50"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--stream-songs", type=int, default=10000)
    ap.add_argument("--listeners", default="1,64,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    res = {"device": ctx.device_info()["name"], "single_query": single_query(S, ctx, a.songs)}
    db = stream_table(S, ctx, a.stream_songs)
    res["stream_table"] = {"songs": a.stream_songs, "song_seconds": 10, "table_rows": int(db.num_fingerprints())}
    res["stereo_listener"] = listeners(S, ctx, db, a.stream_songs, 1, 2)
    res["mono_listeners"] = [listeners(S, ctx, db, a.stream_songs, int(n), 1) for n in a.listeners.split(",") if n]
    db.close()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
