#!/usr/bin/env python3
"""catalog_fit_bench.py -- find_duplicates(..., extents="fit") measured: the extent stage on the found pairs (csrc/shz_catalog.hip:
the job form of the row warp, shz_match_songs_warps_extents; shazam_amd/catalog.py: pair_extents_warps).

    python scripts/catalog_fit_bench.py [--songs 4000] [--song-seconds 10] [--planted 0.02] [--lo 0.95] [--hi 1.05] [--step STEP]
                                        [--topn 5] [--batch-rows ROWS] [--out FILE.json]

The corpus, the planted copies and the ladder are catalog_speed_bench.py's (build_catalogue): N music-like synthetic songs, a
--planted fraction resampled to speeds within +-5 %, alternately ON a rung of the ladder and HALF A STEP beside it.
It reports, for every --songs N, from ONE find_duplicates(speeds=ladder, extents="fit", timings=True) call:
  * "ms": the device times of the search's stages (gather, warp, match) and of the extent stage (its own gather, warp and
    extent passes together), hipEvent times summed over the batches, and the extent stage's share of their sum -- a ratio of
    two numbers of the same run of the same build, written down and not asserted -- beside the wall-clock seconds of the call
    with and without extents="fit";
  * over the planted copies that were found, the distribution (median, 90th percentile, largest) of |tempo_fit - true factor|
    beside |rung - true factor|, on-rung and half-step plants apart; the true factor of a pair is the plant's speed where the
    plant's rows were warped and its inverse where the source's were.  Pairs whose fit is NaN are counted.
No threshold of the library depends on these figures.  Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from catalog_speed_bench import build_catalogue  # noqa: E402


def _dist(x):
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return {"n": 0}
    return {"n": int(len(x)), "median": float(np.median(x)), "p90": float(np.percentile(x, 90)), "max": float(x.max())}


def fit_bench(S, ctx, n_songs, song_s, planted, topn, ladder, step_q16, batch_rows):
    from shazam_amd import catalog
    db, plants = build_catalogue(S, ctx, n_songs, song_s, planted, step_q16)
    kw = dict(topn=topn, min_aligned=catalog.MIN_ALIGNED_WARPED, min_coverage=catalog.MIN_COVERAGE_WARPED, speeds=ladder,
              batch_rows=batch_rows)
    warm = np.arange(1, min(n_songs + len(plants), 100) + 1)
    S.find_duplicates(db, sids=warm, extents="fit", **kw)
    t0 = time.perf_counter()
    S.find_duplicates(db, timings=True, **kw)
    plain_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = S.find_duplicates(db, timings=True, extents="fit", **kw)
    fit_s = time.perf_counter() - t0
    ms = res["ms"]
    out = {"songs": n_songs, "planted": len(plants), "song_seconds": song_s, "table_rows": int(db.num_fingerprints()), "topn": topn,
           "batch_rows": batch_rows, "rungs": len(ladder), "step_q16": step_q16, "pairs": int(len(res["pairs"])),
           "find_duplicates_s": plain_s, "find_duplicates_fit_s": fit_s,
           "ms": {"gather": ms[0], "warp": ms[1], "match": ms[2], "extent_stage": ms[3], "extent_share": ms[3] / max(sum(ms), 1e-9)}}
    p = res["pairs"]
    out["drift_bins"] = int(p["drift_bins"][0]) if len(p) else 0
    want = {(min(a, b), max(a, b)): (a, s, on) for a, b, s, on in plants}
    for name, flag in (("planted_on_rung", True), ("planted_half_step", False)):
        fit_err, rung_err, nan = [], [], 0
        for x in p:
            k = (int(x["a"]), int(x["b"]))
            if k not in want or want[k][2] != flag:
                continue
            plant, s, _ = want[k]
            true = s if int(x[str(x["warped"])]) == plant else 1.0 / s
            if np.isnan(x["tempo_fit"]):
                nan += 1
                continue
            fit_err.append(abs(float(x["tempo_fit"]) - true))
            rung_err.append(abs(int(x["tempo_q16"]) / 65536.0 - true))
        out[name] = {"planted": sum(1 for v in want.values() if v[2] == flag), "no_fit": nan, "abs_fit_minus_true": _dist(fit_err),
                     "abs_rung_minus_true": _dist(rung_err)}
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", default="4000")
    ap.add_argument("--song-seconds", type=int, default=10)
    ap.add_argument("--planted", type=float, default=0.02)
    ap.add_argument("--lo", type=float, default=0.95)
    ap.add_argument("--hi", type=float, default=1.05)
    ap.add_argument("--step", type=float, default=None)
    ap.add_argument("--topn", type=int, default=5)
    ap.add_argument("--batch-rows", type=int, default=None, help="rows x warps of one library call (default: catalog.BATCH_ROWS)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shazam_amd as S
    from shazam_amd.catalog import BATCH_ROWS
    from shazam_amd.speed import DEFAULT_STEP_Q16, speed_ladder
    ctx = S.get_context(0)
    ladder = speed_ladder(a.lo, a.hi, a.step)
    step_q16 = DEFAULT_STEP_Q16 if a.step is None else int(round(a.step * 65536))
    res = {"device": ctx.device_info()["name"]}
    res["catalogues"] = [fit_bench(S, ctx, int(n), a.song_seconds, a.planted, a.topn, ladder, step_q16,
                                   BATCH_ROWS if a.batch_rows is None else a.batch_rows)
                         for n in a.songs.split(",") if n]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
