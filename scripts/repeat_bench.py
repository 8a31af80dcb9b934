#!/usr/bin/env python3
"""repeat_bench.py -- repeated content inside one synthetic hour of broadcast (find_repeats: one extraction, the lag histogram
of the recording against itself on the device) beside the same join in numpy on the host.

    python scripts/repeat_bench.py [--minutes 60] [--reps 5] [--out TAG]

The hour: slots of 30 s, slot i playing music-like track i -- except the advert slots: advert A (track 5000) airs in the slots
7, 31, 55, 79 and 103, advert B (track 5001) in 15, 63 and 111, each from the same start.  A slot is 645.996 frames, so the lags
between two airings are not whole frames.  Assembled on the device, read back once: both paths start from the same host PCM.
(a) Context.repeats_batch on the host PCM: the three device stage times (extraction | compose .. expand | cells) and the wall
    time of the call; then find_repeats (the call, the fold, the dicts).  One warm-up, then --reps runs: the min, the median
    and the max of each.
(b) the CPU baseline, timed outside the GPU region on the hashes of one fingerprint_batch: the dictionary join of
    tests/repeat_twin.py in numpy -- unique (key, t), the runs of every key, all pairs of every run of at most max_run
    entries by run length, the cells by one more unique.  It must give the device's pairs and cells.
Prints one JSON line; --out TAG also writes it to profiles/TAG_repeat_bench.json."""
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

FS, HOP = 44100, 2048
SLOT_S = 30
ADVERTS = {5000: (7, 31, 55, 79, 103), 5001: (15, 63, 111)}
MIN_LAG_S, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS = 5.0, 64, 5, 8


def build_hour(ctx, minutes):
    from shazam_amd import _ffi
    n_slots, ln = minutes * 60 // SLOT_S, SLOT_S * FS
    advert = {s: a for a, slots in ADVERTS.items() for s in slots}
    buf = ctx.alloc(n_slots * ln * 2)
    for s in range(n_slots):
        track, start = (advert[s], 2048 * 10 + 555) if s in advert else (s, 2048 * 10 + 555 + 31 * s)
        ctx.check(_ffi.lib().shz_synth_corpus(ctx.h, 1, 77, track, 1, ln, 3000, 100, 1500, start, _ffi.vp(buf.ptr + s * ln * 2)))
    pcm = buf.download(np.int16, n_slots * ln)
    buf.free()
    aired = [len([s for s in slots if s < n_slots]) for slots in ADVERTS.values()]
    return pcm, sum(n * (n - 1) // 2 for n in aired)


def numpy_join(key32, t1, min_lag, max_lag, max_run, cell_shift, min_cell_pairs):
    """The twin's join for one recording, in numpy: the pairs, and the kept cells' columns lag, block, pairs, first, last"""
    u = np.unique((key32.astype(np.uint64) << np.uint64(20)) | t1.astype(np.uint64))
    _, start, count = np.unique(u >> np.uint64(20), return_index=True, return_counts=True)
    t = (u & np.uint64(0xFFFFF)).astype(np.int64)
    lags, firsts = [], []
    for m in np.unique(count):
        if m < 2 or m > max_run:
            continue
        T = t[start[count == m][:, None] + np.arange(m)[None, :]]           # [runs of m entries, m]
        i, j = np.triu_indices(m, 1)
        lag = T[:, j] - T[:, i]
        ok = (lag >= min_lag) & (lag <= max_lag)
        lags.append(lag[ok])
        firsts.append(T[:, i][ok])
    lag = np.concatenate(lags) if lags else np.zeros(0, np.int64)
    ti = np.concatenate(firsts) if firsts else np.zeros(0, np.int64)
    cell = (lag << 20) | (ti >> cell_shift)
    order = np.argsort(cell, kind="stable")
    cell, ti = cell[order], ti[order]
    ck, c0, cn = np.unique(cell, return_index=True, return_counts=True)
    first = np.minimum.reduceat(ti, c0) if len(c0) else ti
    last = np.maximum.reduceat(ti, c0) if len(c0) else ti
    keep = cn >= min_cell_pairs
    return len(lag), {"lag": (ck >> 20)[keep], "block": (ck & 0xFFFFF)[keep], "pairs": cn[keep], "first": first[keep], "last": last[keep]}


def stats(x):
    return {"min": float(np.min(x)), "median": float(np.median(x)), "max": float(np.max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_repeat_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    pcm, planted = build_hour(ctx, a.minutes)
    off, rc0 = np.asarray([0, len(pcm)], np.uint64), [0, 1]
    lo, hi = max(1, int(round(MIN_LAG_S * FS / HOP))), (1 << 20) - 1
    res = {"device": ctx.device_info()["name"], "minutes": a.minutes, "samples": int(len(pcm)), "frames": ctx.frames_of(len(pcm)),
           "min_lag": lo, "max_lag": hi, "max_run": MAX_RUN, "cell_shift": CELL_SHIFT, "min_cell_pairs": MIN_CELL_PAIRS,
           "reps": a.reps, "planted_pairs_of_airings": planted}

    # (a) the device path
    def call():
        return ctx.repeats_batch(pcm, off, rc0, lo, hi, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS, cap_cells=1 << 20)
    call()
    ms, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        cells, m = call()
        wall.append(time.perf_counter() - t0)
        ms.append(m)
    ms = np.asarray(ms)
    res["repeats_batch"] = {"ms_extract": stats(ms[:, 0]), "ms_pairs": stats(ms[:, 1]), "ms_cells": stats(ms[:, 2]),
                            "wall_seconds": stats(wall), "hashes": int(cells["rec_hashes"][0]), "pairs": int(cells["rec_pairs"][0]),
                            "skipped_keys": int(cells["rec_skipped_keys"][0]), "skipped_rows": int(cells["rec_skipped_rows"][0]),
                            "cells": int(len(cells["lag"]))}
    S.find_repeats([pcm], Fs=FS, min_lag_seconds=MIN_LAG_S, ctx=ctx)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        reps = S.find_repeats([pcm], Fs=FS, min_lag_seconds=MIN_LAG_S, ctx=ctx)
        wall.append(time.perf_counter() - t0)
    groups = S.occurrences(reps)
    res["find_repeats"] = {"wall_seconds": stats(wall), "repeats": len(reps), "groups": [len(g["intervals"]) for g in groups],
                           "longest_seconds": max((p["first_end_seconds"] - p["first_start_seconds"] for p in reps), default=0.0)}

    # (b) the host join, outside the GPU region
    key32, t1, _, _ = ctx.fingerprint_batch(pcm, off)
    numpy_join(key32[:1000], t1[:1000], lo, hi, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        n_pairs, host = numpy_join(key32, t1, lo, hi, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS)
        wall.append(time.perf_counter() - t0)
    same = n_pairs == int(cells["rec_pairs"][0]) and all(np.array_equal(np.asarray(host[k], np.int64), cells[k].astype(np.int64))
                                                         for k in ("lag", "block", "pairs", "first", "last"))
    res["numpy_join"] = {"wall_seconds": stats(wall), "pairs": int(n_pairs), "cells": int(len(host["lag"])), "same_as_device": bool(same)}
    dev = res["repeats_batch"]["ms_pairs"]["min"] + res["repeats_batch"]["ms_cells"]["min"]
    res["numpy_over_device_join"] = res["numpy_join"]["wall_seconds"]["min"] * 1e3 / dev if dev else None
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_repeat_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
