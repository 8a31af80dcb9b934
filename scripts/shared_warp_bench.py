#!/usr/bin/env python3
"""shared_warp_bench.py -- ALTERED content shared between two synthetic broadcast logs (find_shared at a speed ladder: the
peaks of both recordings once, one warp pass, the join of shz_shared_* at every rung) beside plain find_shared on the same two
hours in the same run, and beside the same join in numpy on the host.

    python scripts/shared_warp_bench.py [--minutes 60] [--reps 5] [--out TAG]

The two recordings of scripts/shared_bench.py ("Monday", "Tuesday"; adverts A and B in their slots), but station B plays its
adverts sped up 1.03 (linear interpolation on the host; the 0.87 s left of the 30 s slot are silent), so the plain join finds
none of them.  One pair (Tuesday, Monday), the whole lag range, three speed ladders:
     1 rung    1.03
     9 rungs   1.000 .. 1.040 in steps of 0.5 %
    73 rungs   0.955 .. 1.045 in steps of 0.125 %
(a) Context.shared_warps_batch, one job per rung: the four device stage times (extraction | warp | compose .. expand | cells)
    and the wall time; min, median and max of --reps runs after a warm-up.  The hash, item (= the hashes of Tuesday at every
    rung) and pair counts.  Then find_shared(speeds=ladder): wall time and what was found.
(b) Context.shared_batch and plain find_shared on the same PCM: the comparison.
(c) the CPU baseline for the 1- and the 9-rung ladder, outside the timed region: shared_bench's numpy join on the hashes
    Context.warp_pair_hash_tf gives for Tuesday's peaks at every rung.  It must give the device's pairs, skip counters and cells.
Prints one JSON line; --out TAG also writes it to profiles/TAG_shared_warp_bench.json."""
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

from shared_bench import ADVERTS, CELL_SHIFT, FS, MAX_RUN, MIN_CELL_PAIRS, SLOT_S, T_MAX, build_day, numpy_join, stats  # noqa: E402

SPEED = 1.03
q16 = lambda x: int(round(x * 65536))                                            # noqa: E731
LADDERS = {1: [q16(SPEED)], 9: [q16(1.0 + 0.005 * k) for k in range(9)], 73: [q16(0.955 + 0.00125 * k) for k in range(73)]}


def speed_up(x, s):
    """x played s times as fast, by linear interpolation (tests/speed_twin.py)"""
    x = x.astype(np.float64)
    pos = np.arange(int((len(x) - 1) / s) + 1, dtype=np.float64) * s
    return np.clip(np.rint(np.interp(pos, np.arange(len(x), dtype=np.float64), x)), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="tag: the line also goes to profiles/<tag>_shared_warp_bench.json")
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    monday, _ = build_day(ctx, a.minutes, 0)
    tuesday, _ = build_day(ctx, a.minutes, 1)
    ln, n_slots = SLOT_S * FS, a.minutes * 60 // SLOT_S
    planted = 0
    for adv, slots in ADVERTS[1].items():
        for s in (s for s in slots if s < n_slots):
            fast = speed_up(tuesday[s * ln:(s + 1) * ln], SPEED)
            tuesday[s * ln:(s + 1) * ln] = 0
            tuesday[s * ln:s * ln + len(fast)] = fast
            planted += len([m for m in ADVERTS[0][adv] if m < n_slots])
    pcm = np.concatenate([monday, tuesday])
    n = len(monday)
    off, rc0 = np.asarray([0, n, 2 * n], np.uint64), [0, 1, 2]
    recs = [pcm[:n], pcm[n:]]
    res = {"device": ctx.device_info()["name"], "minutes_each": a.minutes, "recordings": 2, "samples": int(len(pcm)),
           "frames_each": ctx.frames_of(n), "speed_of_b": SPEED, "max_run": MAX_RUN, "cell_shift": CELL_SHIFT,
           "min_cell_pairs": MIN_CELL_PAIRS, "reps": a.reps, "planted_pairs_of_airings": planted, "ladders": {}}

    def timed(call):
        call()
        ms, wall, out = [], [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out, m = call()
            wall.append(time.perf_counter() - t0)
            ms.append(m)
        return out, np.asarray(ms), wall

    def wall_of(call):
        call()
        wall, out = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = call()
            wall.append(time.perf_counter() - t0)
        return out, wall

    # (b) the plain join, the comparison
    cells, ms, wall = timed(lambda: ctx.shared_batch(pcm, off, rc0, [(1, 0)], -T_MAX, T_MAX, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS,
                                                     cap_cells=1 << 21))
    found, fwall = wall_of(lambda: S.find_shared(recs, pairs=[(1, 0)], Fs=FS, ctx=ctx))
    res["plain"] = {"ms_extract": stats(ms[:, 0]), "ms_pairs": stats(ms[:, 1]), "ms_cells": stats(ms[:, 2]), "wall_seconds": stats(wall),
                    "hashes": [int(x) for x in cells["rec_hashes"]], "items": int(cells["rec_hashes"][1]),
                    "pairs": int(cells["job_pairs"][0]), "cells": int(len(cells["lag"])),
                    "find_shared": {"wall_seconds": stats(fwall), "stretches": len(found)}}
    # (a) the ladders
    kept = {}
    for rungs, ladder in LADDERS.items():
        jobs = [(1, 0, v, -T_MAX, T_MAX) for v in range(rungs)]
        cells, ms, wall = timed(lambda: ctx.shared_warps_batch(pcm, off, rc0, ladder, ladder, jobs, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS,
                                                               cap_cells=1 << 22))
        kept[rungs] = cells
        sp = np.asarray(ladder, np.uint32)
        found, fwall = wall_of(lambda: S.find_shared(recs, pairs=[(1, 0)], speeds=sp, Fs=FS, ctx=ctx))
        res["ladders"][str(rungs)] = {
            "ms_extract": stats(ms[:, 0]), "ms_warp": stats(ms[:, 1]), "ms_pairs": stats(ms[:, 2]), "ms_cells": stats(ms[:, 3]),
            "wall_seconds": stats(wall), "hashes": [int(x) for x in cells["rec_hashes"]],
            "items": int(np.sum(cells["job_hashes"], dtype=np.int64)), "pairs": int(np.sum(cells["job_pairs"], dtype=np.int64)),
            "pairs_at_the_true_rung": int(cells["job_pairs"][ladder.index(q16(SPEED))]), "cells": int(len(cells["lag"])),
            "find_shared": {"wall_seconds": stats(fwall), "stretches": len(found),
                            "speeds": sorted({round(p["speed"], 5) for p in found if "speed" in p}),
                            "at_the_true_rung": len([p for p in found if p["t16"] == q16(SPEED)]),
                            "tempo_fit": stats([p["tempo_fit"] for p in found if p["t16"] == q16(SPEED) and p["tempo_fit"]] or [0.0])}}
    # (c) the host join of the 1- and the 9-rung ladder, outside the GPU region
    pf, pt, po = ctx.peaks(pcm, off)
    po = [int(x) for x in po]
    km, tm, _ = ctx.warp_pair_hash_tf(pf[:po[1]], pt[:po[1]], [0, po[1]], [65536], [65536])
    for rungs in (1, 9):
        ladder, cells = LADDERS[rungs], kept[rungs]
        k, t1, ho = ctx.warp_pair_hash_tf(pf[po[1]:], pt[po[1]:], [0, po[2] - po[1]], ladder, ladder)
        ho = [int(x) for x in ho]
        t0 = time.perf_counter()
        same, n_pairs, n_cells = True, 0, 0
        for v in range(rungs):
            got = numpy_join(k[ho[v]:ho[v + 1]], t1[ho[v]:ho[v + 1]], km, tm, -T_MAX, T_MAX, MAX_RUN, CELL_SHIFT, MIN_CELL_PAIRS)
            c0, c1 = int(cells["cell_off"][v]), int(cells["cell_off"][v + 1])
            same = same and (got[0], got[1], got[2]) == (int(cells["job_pairs"][v]), int(cells["job_skipped_keys"][v]),
                                                         int(cells["job_skipped_rows"][v])) \
                and all(np.array_equal(np.asarray(got[3][f], np.int64), cells[f][c0:c1].astype(np.int64))
                        for f in ("lag", "block", "pairs", "first", "last"))
            n_pairs, n_cells = n_pairs + got[0], n_cells + len(got[3]["lag"])
        host = time.perf_counter() - t0
        r = res["ladders"][str(rungs)]
        r["numpy_join"] = {"wall_seconds": host, "pairs": int(n_pairs), "cells": int(n_cells), "same_as_device": bool(same)}
        dev = r["ms_pairs"]["min"] + r["ms_cells"]["min"]
        r["numpy_over_device_join"] = host * 1e3 / dev if dev else None
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    line = json.dumps(res)
    print(line)
    if a.out:
        path = os.path.join(ROOT, "profiles", f"{a.out}_shared_warp_bench.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
