#!/usr/bin/env python3
"""catalog_speed_bench.py -- find_duplicates at a speed ladder (csrc/shz_catalog.hip: the row warp; shazam_amd/catalog.py) measured.

    python scripts/catalog_speed_bench.py [--songs 4000] [--song-seconds 10] [--planted 0.02] [--lo 0.95] [--hi 1.05]
                                          [--step STEP] [--topn 5] [--warp-songs 500] [--batch-rows ROWS] [--out FILE.json]

The corpus is catalog_bench.py's: N music-like synthetic songs (shz_synth_corpus) of --song-seconds.  A --planted fraction of N
is planted under new ids as ALTERED copies: the source clip resampled on the device (resample_batch) from fs_in to 44,100 Hz and
inserted as 44.1 kHz audio, which plays fs_in / 44,100 times as fast -- a clip resampled by L / M plays M / L as fast.  The planted
speeds lie within +-5 %: for rungs k in (-35, -21, -7, 7, 21, 35) of the default ladder (step 92 / 65536 = 0.14 %), alternately
ON the rung and HALF A STEP beside it (fs_in is rounded to a whole Hz: 0.001 % off at most).
It reports, for every --songs N:
  * seconds and songs per second of find_duplicates(speeds=speed_ladder(lo, hi, step)) beside the plain find_duplicates of the
    same run, and the three stage times (gather, warp, match: hipEvent times summed over the batches);
  * the warp stage alone (shz_warp_rows on device columns of the first --warp-songs songs at the whole ladder, 2 warm-up + 5
    timed calls, the median; BOTH calls of the two-call idiom are in the time only once -- the call is made with enough room):
    bytes per second counted as 8 B read per row and 8 B written per kept item, beside shz_membw's copy rate of the same run;
  * the separation table: the largest aligned count / coverage (of the smaller song) among unrelated pairs at ANY rung -- the
    fold keeps every pair's best over all rungs and both sides -- and the smallest among the planted pairs, on-rung and
    half-step plants apart; then recall and false pairs at the defaults of shazam_amd/catalog.py.
Prints one JSON line; --out also writes it to a file."""
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

from catalog_bench import SEED, median_ms  # noqa: E402

RUNGS = (-35, -21, -7, 7, 21, 35)
FS = 44100


def build_catalogue(S, ctx, n_songs, song_s, planted, step_q16):
    """songs 1 .. n_songs, then the planted ones: (db, plants) with plants = [(new id, source id, speed, on_rung)]"""
    from shazam_amd.resample import resample_batch
    db = S.get_database("hip")(ctx=ctx)
    ln = song_s * FS
    cap = max(8000, 800 * song_s)
    for b0 in range(0, n_songs, 1000):
        nb = min(1000, n_songs - b0)
        pcm = ctx.synth_corpus(1, SEED, b0, nb, ln)
        ok, ot = ctx.alloc(nb * cap * 4), ctx.alloc(nb * cap * 4)
        _, _, ho, _ = ctx.fingerprint_batch(pcm.ptr, np.arange(nb + 1, dtype=np.uint64) * ln, pcm_device=True, out_key=ok, out_t1=ot)
        for c in range(nb):
            db.insert_song(f"song{b0 + c}", f"{b0 + c:040x}", int(ho[c + 1] - ho[c]))
        db.insert_clips(ok.ptr, ot.ptr, ho, b0 + 1, device=True)
        for x in (pcm, ok, ot):
            x.free()
    n_plant = int(round(planted * n_songs))
    rng = np.random.default_rng(3)
    sources = rng.choice(n_songs, n_plant, replace=False).tolist()
    by_rate = {}
    for i, c in enumerate(sources):
        k, on = RUNGS[i % len(RUNGS)], (i // len(RUNGS)) % 2 == 0
        s = (65536 + step_q16 * (k if on else k + 0.5)) / 65536.0
        by_rate.setdefault((int(round(FS * s)), on), []).append(c)
    plants = []
    for (fs_in, on), srcs in sorted(by_rate.items()):
        clips = []
        for c in srcs:
            d = ctx.synth_corpus(1, SEED, c, 1, ln)
            clips.append(d.download(np.int16, ln))
            d.free()
        for c, y in zip(srcs, resample_batch(clips, fs_in, FS, ctx=ctx)):
            kk, tt, _ = S.fingerprint_batch([y], ctx=ctx)
            sid = db.insert_song(f"plant{len(plants)}", f"{n_songs + len(plants):040x}", len(kk))
            db.insert_keys(sid, kk, tt)
            plants.append((sid, c + 1, fs_in / FS, on))
    db.finalize()
    return db, plants


def warp_stage(ctx, db, ladder, n_songs):
    """shz_warp_rows alone, device columns in and out"""
    from shazam_amd import _ffi
    ro, k, o = db.table.song_hashes(np.arange(1, n_songs + 1, dtype=np.uint32))
    rows = int(ro[-1])
    kept = ctx.warp_rows_raw(k, o, ro, ladder, ladder, cap=0)[4]        # (SHZ_E_CAPACITY: the count)
    dk, do = ctx.alloc(max(rows, 1) * 4), ctx.alloc(max(rows, 1) * 4)
    ok, oo = ctx.alloc(max(kept, 1) * 4), ctx.alloc(max(kept, 1) * 4)
    dk.upload(k)
    do.upload(o)

    def call():
        rc = ctx.warp_rows_raw(dk, do, ro, ladder, ladder, cap=kept, device_in=True, out_key=ok, out_off=oo)[0]
        assert rc == _ffi.OK

    ms, lo, hi = median_ms(call, warm=2, reps=5)
    for b in (dk, do, ok, oo):
        b.free()
    nbytes = 8.0 * rows + 8.0 * kept
    return {"songs": n_songs, "rows": rows, "warps": len(ladder), "items": rows * len(ladder), "kept_items": kept, "ms": ms,
            "ms_min": lo, "ms_max": hi, "bytes_counted": nbytes, "gbs_counted": nbytes / ms / 1e6,
            "items_per_s": rows * len(ladder) / ms * 1e3}


def catalogue_bench(S, ctx, n_songs, song_s, planted, topn, ladder, step_q16, warp_songs, batch_rows):
    from shazam_amd import catalog
    db, plants = build_catalogue(S, ctx, n_songs, song_s, planted, step_q16)
    total = n_songs + len(plants)
    out = {"songs": n_songs, "planted": len(plants), "song_seconds": song_s, "table_rows": int(db.num_fingerprints()), "topn": topn,
           "batch_rows": batch_rows, "rungs": len(ladder), "ladder_lo_q16": int(ladder[0]), "ladder_hi_q16": int(ladder[-1]), "step_q16": step_q16}
    warm = np.arange(1, min(total, 100) + 1)
    S.find_duplicates(db, sids=warm, topn=topn, min_aligned=1, min_coverage=0.5)
    S.find_duplicates(db, sids=warm, topn=topn, min_aligned=1, min_coverage=0.5, speeds=ladder)
    t0 = time.perf_counter()
    S.find_duplicates(db, topn=topn, min_aligned=1, min_coverage=0.5, batch_rows=batch_rows)
    dt = time.perf_counter() - t0
    out["plain"] = {"find_duplicates_s": dt, "songs_per_s": total / dt}
    t0 = time.perf_counter()
    res = S.find_duplicates(db, topn=topn, min_aligned=1, min_coverage=catalog.MIN_COVERAGE_WARPED, speeds=ladder, timings=True,
                            batch_rows=batch_rows)
    dt = time.perf_counter() - t0
    out["ladder"] = {"find_duplicates_s": dt, "songs_per_s": total / dt, "song_rungs_per_s": total * len(ladder) / dt,
                     "ms_gather": res["ms"][0], "ms_warp": res["ms"][1], "ms_match": res["ms"][2]}
    out["ladder_over_plain"] = out["ladder"]["find_duplicates_s"] / out["plain"]["find_duplicates_s"]
    out["membw_copy_gbs"] = ctx.membw(0, 4 << 30, 5)
    out["warp_stage"] = warp_stage(ctx, db, ladder, min(warp_songs, n_songs))
    out["warp_stage"]["over_membw_copy"] = out["warp_stage"]["gbs_counted"] / out["membw_copy_gbs"]
    p = res["pairs"]
    want = {(min(a, b), max(a, b)): (s, on) for a, b, s, on in plants}
    key = [(int(a), int(b)) for a, b in zip(p["a"], p["b"])]
    is_plant = np.array([k in want for k in key], bool)
    cov_small = np.maximum(p["coverage_a"], p["coverage_b"])
    un = ~is_plant
    out["pairs_seen"] = int(len(p))
    out["unrelated"] = {"pairs": int(un.sum()), "aligned_max": int(p["aligned"][un].max(initial=0)),
                        "aligned_p999": float(np.percentile(p["aligned"][un], 99.9)) if un.any() else 0.0,
                        "coverage_small_max": float(cov_small[un].max(initial=0.0))}
    for name, flag in (("planted_on_rung", True), ("planted_half_step", False)):
        m = np.array([f and want[k][1] == flag for k, f in zip(key, is_plant)], bool)
        n_want = sum(1 for v in want.values() if v[1] == flag)
        out[name] = {"planted": n_want, "seen": int(m.sum()), "aligned_min": int(p["aligned"][m].min(initial=1 << 30)),
                     "aligned_median": float(np.median(p["aligned"][m])) if m.any() else 0.0,
                     "coverage_small_min": float(cov_small[m].min(initial=9.0)),
                     "coverage_large_min": float(np.minimum(p["coverage_a"], p["coverage_b"])[m].min(initial=9.0)),
                     "aligned_plain_max": int(p["aligned_plain"][m].max(initial=0)),
                     "rung_error_max_q16": int(max([abs(int(t) - int(round((want[k][0] if w == "b" else 1.0 / want[k][0]) * 65536)))
                                                    for k, t, w, f in zip(key, p["tempo_q16"], p["warped"], m) if f], default=0))}
    keep = p["aligned"] >= catalog.MIN_ALIGNED_WARPED
    found = {k for k, f, kp in zip(key, is_plant, keep) if f and kp}
    same = keep & (p["relation"] == "same")
    out["at_defaults"] = {"min_aligned": catalog.MIN_ALIGNED_WARPED, "min_coverage": catalog.MIN_COVERAGE_WARPED,
                          "recall": len(found) / max(1, len(want)), "false_pairs": int((keep & un).sum()),
                          "planted_labelled_same": int((same & is_plant).sum()), "unrelated_labelled_same": int((same & un).sum())}
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
    ap.add_argument("--warp-songs", type=int, default=500)
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
    res["catalogues"] = [catalogue_bench(S, ctx, int(n), a.song_seconds, a.planted, a.topn, ladder, step_q16, a.warp_songs,
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
