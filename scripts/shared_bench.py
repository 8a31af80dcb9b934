#!/usr/bin/env python3
"""shared_bench.py -- content shared between two synthetic broadcast logs (find_shared: one extraction of both recordings, the
signed lag histogram of one against the other on the device) beside the same join in numpy on the host.

    python scripts/shared_bench.py [--minutes 60] [--reps 5] [--out TAG]

Two recordings ("Monday", "Tuesday") of --minutes each, in slots of 30 s.  Monday's slot i plays music-like track i, Tuesday's
track 10000 + i -- except the advert slots: advert A (track 5000) airs on Monday in the slots 7, 31 and 79 and on Tuesday in 11,
40 and 103, advert B (track 5001) on Monday in 15 and on Tuesday in 20 and 63, each from the same start.  A slot is 645.996
frames, so the lags between two airings are not whole frames; they are negative for A's 31 -> 11 and 79 -> 11 / 40.  Assembled
on the device, read back once: both paths start from the same host PCM.
(a) Context.shared_batch on the host PCM, one job (Monday, Tuesday), the whole lag range: the three device stage times
    (extraction | compose .. expand | cells) and the wall time of the call; then find_shared (the call, the fold, the dicts).
    One warm-up, then --reps runs: the min, the median and the max of each.
(b) the CPU baseline, timed outside the GPU region on the hashes of one fingerprint_batch: the dictionary join of
    tests/shared_twin.py in numpy -- unique (key, t) of either recording, the keys of both, all (t_a, t_b) of every key of at
    most max_run times on either side by the two run lengths, the cells by one more unique.  It must give the device's pairs,
    skip counters and cells.
Prints one JSON line; --out TAG also writes it to profiles/TAG_shared_bench.json."""
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
ADVERTS = ({5000: (7, 31, 79), 5001: (15,)}, {5000: (11, 40, 103), 5001: (20, 63)})   # Monday, Tuesday
MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS = 64, 5, 8
T_MAX, BIAS = (1 << 20) - 1, 1 << 20


def build_day(ctx, minutes, day):
    from shazam_amd import _ffi
    n_slots, ln = minutes * 60 // SLOT_S, SLOT_S * FS
    advert = {s: a for a, slots in ADVERTS[day].items() for s in slots}
    buf = ctx.alloc(n_slots * ln * 2)
    for s in range(n_slots):
        track, start = (advert[s], 2048 * 10 + 555) if s in advert else (10000 * day + s, 2048 * 10 + 555 + 31 * s)
        ctx.check(_ffi.lib().shz_synth_corpus(ctx.h, 1, 77, track, 1, ln, 3000, 100, 1500, start, _ffi.vp(buf.ptr + s * ln * 2)))
    pcm = buf.download(np.int16, n_slots * ln)
    buf.free()
    return pcm, {a: len([s for s in slots if s < n_slots]) for a, slots in ADVERTS[day].items()}


def _runs(key32, t1):
    u = np.unique((key32.astype(np.uint64) << np.uint64(20)) | t1.astype(np.uint64))
    keys, start, count = np.unique(u >> np.uint64(20), return_index=True, return_counts=True)
    return (u & np.uint64(0xFFFFF)).astype(np.int64), keys, start, count


def numpy_join(ka, ta, kb, tb, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs):
    """The twin's join of one job, in numpy: pairs, skipped keys, skipped rows, and the kept cells' columns lag (biased), block,
    pairs, first, last"""
    t_a, keys_a, sa, ca = _runs(ka, ta)
    t_b, keys_b, sb, cb = _runs(kb, tb)
    _, ia, ib = np.intersect1d(keys_a, keys_b, assume_unique=True, return_indices=True)
    sa, ca, sb, cb = sa[ia], ca[ia], sb[ib], cb[ib]
    stop = (ca > max_run) | (cb > max_run)
    lags, firsts = [], []
    for ma, mb in sorted(set(zip(ca[~stop].tolist(), cb[~stop].tolist()))):
        sel = ~stop & (ca == ma) & (cb == mb)
        A = t_a[sa[sel][:, None] + np.arange(ma)[None, :]]                      # [keys, ma]
        B = t_b[sb[sel][:, None] + np.arange(mb)[None, :]]                      # [keys, mb]
        lag = B[:, None, :] - A[:, :, None]
        ok = (lag >= lag_lo) & (lag <= lag_hi)
        lags.append(lag[ok])
        firsts.append(np.broadcast_to(A[:, :, None], lag.shape)[ok])
    lag = np.concatenate(lags) if lags else np.zeros(0, np.int64)
    t = np.concatenate(firsts) if firsts else np.zeros(0, np.int64)
    cell = ((lag + BIAS) << 20) | (t >> cell_shift)
    order = np.argsort(cell, kind="stable")
    cell, t = cell[order], t[order]
    ck, c0, cn = np.unique(cell, return_index=True, return_counts=True)
    first = np.minimum.reduceat(t, c0) if len(c0) else t
    last = np.maximum.reduceat(t, c0) if len(c0) else t
    keep = cn >= min_cell_pairs
    return len(lag), int(stop.sum()), int((ca + cb)[stop].sum()), {"lag": (ck >> 20)[keep], "block": (ck & 0xFFFFF)[keep],
                                                                      "pairs": cn[keep], "first": first[keep], "last": last[keep]}


def stats(x):
    return {"min": float(np.min(x)), "median": float(np.median(x)), "max": float(np.max(x))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_shared_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    days = [build_day(ctx, a.minutes, d) for d in (0, 1)]
    pcm = np.concatenate([d[0] for d in days])
    n = len(days[0][0])
    off, rc0, jobs = np.asarray([0, n, 2 * n], np.uint64), [0, 1, 2], [(0, 1)]
    planted = sum(days[0][1][adv] * days[1][1][adv] for adv in days[0][1])
    res = {"device": ctx.device_info()["name"], "minutes_each": a.minutes, "recordings": 2, "samples": int(len(pcm)),
           "frames_each": ctx.frames_of(n), "lag_lo": -T_MAX, "lag_hi": T_MAX, "max_run": MAX_RUN, "cell_shift": CELL_SHIFT,
           "min_cell_pairs": MIN_CELL_PAIRS, "reps": a.reps, "planted_pairs_of_airings": planted}

    # (a) the device path
    def call():
        return ctx.shared_batch(pcm, off, rc0, jobs, -T_MAX, T_MAX, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS, cap_cells=1 << 21)
    call()
    ms, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        cells, m = call()
        wall.append(time.perf_counter() - t0)
        ms.append(m)
    ms = np.asarray(ms)
    res["shared_batch"] = {"ms_extract": stats(ms[:, 0]), "ms_pairs": stats(ms[:, 1]), "ms_cells": stats(ms[:, 2]),
                           "wall_seconds": stats(wall), "hashes": [int(x) for x in cells["rec_hashes"]],
                           "pairs": int(cells["job_pairs"][0]), "skipped_keys": int(cells["job_skipped_keys"][0]),
                           "skipped_rows": int(cells["job_skipped_rows"][0]), "cells": int(len(cells["lag"]))}
    recs = [pcm[:n], pcm[n:]]
    S.find_shared(recs, Fs=FS, ctx=ctx)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        found = S.find_shared(recs, Fs=FS, ctx=ctx)
        wall.append(time.perf_counter() - t0)
    groups = S.shared_occurrences(found)
    res["find_shared"] = {"wall_seconds": stats(wall), "stretches": len(found), "groups": [len(g["airings"]) for g in groups],
                          "lags": sorted(p["lag"] for p in found),
                          "longest_seconds": max((p["a_end_seconds"] - p["a_start_seconds"] for p in found), default=0.0)}

    # (b) the host join, outside the GPU region
    key32, t1, ho, _ = ctx.fingerprint_batch(pcm, off)
    ho = [int(x) for x in ho]
    cols = (key32[:ho[1]], t1[:ho[1]], key32[ho[1]:], t1[ho[1]:])
    numpy_join(*(c[:1000] for c in cols), -T_MAX, T_MAX, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        n_pairs, skip_keys, skip_rows, host = numpy_join(*cols, -T_MAX, T_MAX, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS)
        wall.append(time.perf_counter() - t0)
    same = (n_pairs, skip_keys, skip_rows) == (int(cells["job_pairs"][0]), int(cells["job_skipped_keys"][0]),
                                               int(cells["job_skipped_rows"][0])) \
        and all(np.array_equal(np.asarray(host[k], np.int64), cells[k].astype(np.int64)) for k in ("lag", "block", "pairs", "first", "last"))
    res["numpy_join"] = {"wall_seconds": stats(wall), "pairs": int(n_pairs), "skipped_keys": skip_keys, "skipped_rows": skip_rows,
                         "cells": int(len(host["lag"])), "same_as_device": bool(same)}
    dev = res["shared_batch"]["ms_pairs"]["min"] + res["shared_batch"]["ms_cells"]["min"]
    res["numpy_over_device_join"] = res["numpy_join"]["wall_seconds"]["min"] * 1e3 / dev if dev else None
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_shared_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
