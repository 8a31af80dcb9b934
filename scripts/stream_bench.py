#!/usr/bin/env python3
"""stream_bench.py -- live streams (shz_streams_*) on one MI355X.

    python scripts/stream_bench.py [--streams 1024] [--seconds 30] [--songs 10000] [--out FILE.json]

(a) --streams streams of on-device synthetic PCM (shz_synth_pcm: tonal + noise), --seconds long, pushed in 1 s chunks
    (device PCM in, device hashes out): audio-s/s, push ms p50 / p99, frames computed per new frame (the halo the window
    plan recomputes, from shz_stream_plan).
(b) one stereo listener in the reference's 8192-sample chunks (recognizer.py:21-25) against a table of --songs 10 s
    music-like songs: latency of push + recognise (StreamRecognizer: one push, one batched match) p50 / p99.
Prints one JSON line; --out also writes it to a file."""
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


def many_streams(S, ctx, n, seconds, fs=44100):
    F = S._ffi
    st = F.Streams(ctx, n, fs, 10.0, 5)
    chunk = fs
    pcm = ctx.alloc(n * chunk * 2)
    ok, ot = ctx.alloc(n * 200 * 5 * 4 + (1 << 20)), ctx.alloc(n * 200 * 5 * 4 + (1 << 20))
    co = (np.arange(n + 1, dtype=np.uint64) * chunk)
    ms, hashes = [], 0
    computed = new = 0
    samples = [0] * n
    settled = [0] * n
    for p in range(seconds):
        ctx.synth_pcm(2024, 0, n, chunk, 4000, 1500, start=p * chunk, out=pcm)   # second p of every stream, chunk-major
        ctx.sync()
        ending = p == seconds - 1
        t0 = time.perf_counter()
        rc, _, _, ho, cnt = st.push_raw(pcm.ptr, co, end=True if ending else None, pcm_device=True, out_key=ok, out_t1=ot)
        ms.append((time.perf_counter() - t0) * 1e3)
        ctx.check(rc)
        hashes += cnt
        for i in range(1):   # every stream has the same schedule: the plan of one is the plan of all
            wf0, ws0, ws1, h = F.stream_plan(samples[i], samples[i] + chunk, settled[i], st.hop, ending)
            if h > settled[i]:
                computed += ctx.frames_of(ws1 - ws0)
                new += h - settled[i]
            samples[i] += chunk
            settled[i] = h
    st.close()
    for b in (pcm, ok, ot):
        b.free()
    steady = ms[1:-1] or ms
    return {"streams": n, "seconds": seconds, "chunk_samples": chunk, "hashes": int(hashes),
            "audio_s_per_s": n * seconds / (sum(ms) / 1e3),
            "audio_s_per_s_steady": n * len(steady) / (sum(steady) / 1e3),
            "push_ms_p50": pct(steady, 50), "push_ms_p99": pct(steady, 99), "push_ms_first": ms[0], "push_ms_last": ms[-1],
            "frames_computed_per_new_frame": computed / max(new, 1)}


def listener(S, ctx, n_songs, song_s=10, fs=44100):
    from oracle import synth
    from shazam_amd import harness
    db = S.get_database("hip")(ctx=ctx)
    ln = song_s * fs
    batch = 1000
    t0 = time.perf_counter()
    for b0 in range(0, n_songs, batch):
        nb = min(batch, n_songs - b0)
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
    build_s = time.perf_counter() - t0
    song = 1234 % n_songs
    start = 2048 * 37 + 555
    length = 8 * fs
    clean = synth.music_clip(77, song, start + length)[start:]
    chans = [harness.mix(clean, synth.traffic_noise(5, c, length), 10) for c in range(2)]
    lat, top = [], []
    for rep in range(2):   # the first pass warms up
        rec = S.StreamRecognizer(db, 1, channels=2, window_seconds=5)
        lat_r = []
        for a in range(0, length, 8192):
            t0 = time.perf_counter()
            out = rec.push([[c[a:a + 8192] for c in chans]])
            lat_r.append((time.perf_counter() - t0) * 1e3)
            top.append(out[0][0][0]["song_id"] if out[0][0] else None)
        rec.close()
        lat = lat_r
    n_rows = db.num_fingerprints()
    db.close()
    return {"songs": n_songs, "song_seconds": song_s, "table_rows": int(n_rows), "build_s": build_s, "chunk_samples": 8192,
            "pushes": len(lat), "push_recognise_ms_p50": pct(lat, 50), "push_recognise_ms_p99": pct(lat, 99),
            "top1_correct_last": top[-1] == song + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=30)
    ap.add_argument("--songs", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    many_streams(S, ctx, a.streams, 4)   # warm-up: code objects, every buffer at its full size
    res = {"device": ctx.device_info()["name"], "many_streams": many_streams(S, ctx, a.streams, a.seconds),
           "listener": listener(S, ctx, a.songs)}
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
