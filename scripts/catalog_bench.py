#!/usr/bin/env python3
"""catalog_bench.py -- the catalogue calls (csrc/shz_catalog.hip, shazam_amd/catalog.py) measured.

    python scripts/catalog_bench.py [--songs 5000,20000] [--song-seconds 10] [--planted 0.02] [--gather-rows 268435456]
                                    [--topn 5] [--out FILE.json]

(a) the gather alone, on a row-level table of --gather-rows random rows over 100,000 song ids in one segment: one in a
    hundred songs listed (and one song, and every song counts-only), shz_table_song_hashes into device columns, 2 warm-up +
    7 timed calls, the median.  GB/s counts 8 bytes per table row (the two passes over the song-id column; counts-only: 4)
    over the time of the WHOLE call -- upload of the list, both passes, the scan, the sort of the hits, the read-back of the
    counts -- beside shz_membw's read rate measured in the same run.  The ratio is the number to write down.
(b) for every --songs N: a table of N music-like synthetic songs (shz_synth_corpus) of --song-seconds, plus a --planted
    fraction of N as planted songs under new ids -- half exact copies, half hop-aligned excerpts (from frame 20, 40, 60 or
    100 to the end).  find_duplicates() over the whole catalogue with min_aligned = 1: seconds, songs per second, and from its
    pairs the two distributions the defaults of min_aligned / min_coverage sit between -- the largest aligned count and
    coverage (of the smaller song) among unrelated pairs, the smallest among planted pairs -- then recall and false pairs at
    the defaults of shazam_amd/catalog.py.
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

SEED = 77
CUTS = (20, 40, 60, 100)


def median_ms(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def gather_bench(S, ctx, rows, n_ids=100_000):
    from shazam_amd import _ffi
    L = _ffi.lib()
    rng = np.random.default_rng(1)
    t = S.Table(ctx)
    chunk = 1 << 25
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        # (key, offset) never repeats across chunks: the chunk index sits in the key's top bits
        key = (rng.integers(0, 1 << 24, n, dtype=np.uint32) | np.uint32((r0 // chunk) << 24)).astype(np.uint32)
        t.insert(key, rng.integers(1, n_ids + 1, n, dtype=np.uint32), rng.integers(0, 4000, n, dtype=np.uint32))
    t.finalize()
    table_rows = int(t.rows()[0])
    out = {"table_rows": table_rows, "segments": t.segments(), "song_ids": n_ids}
    out["membw_read_gbs"] = ctx.membw(1, 4 << 30, 5)
    out["membw_copy_gbs"] = ctx.membw(0, 4 << 30, 5)
    every = np.arange(1, n_ids + 1, dtype=np.uint32)
    lists = {"one_in_a_hundred": rng.choice(every, n_ids // 100, replace=False).astype(np.uint32), "one_song": every[4321:4322],
             "one_in_ten": rng.choice(every, n_ids // 10, replace=False).astype(np.uint32)}
    for name, sids in lists.items():
        ro = np.zeros(len(sids) + 1, np.uint64)
        ctx.check(L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), None, None, 0, 0))
        hits = int(ro[-1])
        dk, do = ctx.alloc(max(hits, 1) * 4), ctx.alloc(max(hits, 1) * 4)

        def full():
            ctx.check(L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), _ffi.ptr(dk),
                                              _ffi.ptr(do), hits, _ffi.SONGS_DEVICE_OUT))

        def counts():
            ctx.check(L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), None, None, 0, 0))

        ms, lo, hi = median_ms(full)
        cms, clo, chi = median_ms(counts)
        out[name] = {"listed": len(sids), "hits": hits, "gather_ms": ms, "gather_ms_min": lo, "gather_ms_max": hi,
                     "gather_gbs": 8.0 * table_rows / ms / 1e6, "counts_ms": cms, "counts_ms_min": clo, "counts_ms_max": chi,
                     "counts_gbs": 4.0 * table_rows / cms / 1e6}
        out[name]["gather_over_membw_read"] = out[name]["gather_gbs"] / out["membw_read_gbs"]
        out[name]["counts_over_membw_read"] = out[name]["counts_gbs"] / out["membw_read_gbs"]
        dk.free()
        do.free()
    ro = np.zeros(n_ids + 1, np.uint64)

    def all_counts():
        ctx.check(L.shz_table_song_hashes(t.h, _ffi.ptr(every), n_ids, ro.ctypes.data_as(_ffi.u64p), None, None, 0, 0))

    ms, lo, hi = median_ms(all_counts)
    assert int(ro[-1]) == table_rows
    out["every_song_counts_only"] = {"listed": n_ids, "hits": table_rows, "counts_ms": ms, "counts_ms_min": lo, "counts_ms_max": hi,
                                     "counts_gbs": 4.0 * table_rows / ms / 1e6}
    t.close()
    return out


def build_catalogue(S, ctx, n_songs, song_s, planted, fs=44100):
    """songs 1 .. n_songs, then the planted ones: (db, plants) with plants = [(new id, source id, cut frames or 0 for a copy)]"""
    db = S.get_database("hip")(ctx=ctx)
    ln = song_s * fs
    cap = max(8000, 800 * song_s)             # hashes a song has room for (about 310 a second on this corpus)
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
    sources = rng.choice(n_songs, n_plant, replace=False)
    plants = []
    for i, c in enumerate(sources.tolist()):
        cut = 0 if i % 2 == 0 else CUTS[(i // 2) % len(CUTS)]
        n = ln - cut * 2048
        pcm = ctx.synth_corpus(1, SEED, c, 1, n, start=cut * 2048)
        ok, ot = ctx.alloc(cap * 4), ctx.alloc(cap * 4)
        _, _, ho, _ = ctx.fingerprint_batch(pcm.ptr, np.array([0, n], np.uint64), pcm_device=True, out_key=ok, out_t1=ot)
        sid = db.insert_song(f"plant{i}", f"{n_songs + i:040x}", int(ho[1]))
        db.insert_clips(ok.ptr, ot.ptr, ho, sid, device=True)
        plants.append((sid, c + 1, cut))
        for x in (pcm, ok, ot):
            x.free()
    db.finalize()
    return db, plants


def catalogue_bench(S, ctx, n_songs, song_s, planted, topn):
    from shazam_amd import catalog
    db, plants = build_catalogue(S, ctx, n_songs, song_s, planted)
    total = n_songs + len(plants)
    out = {"songs": n_songs, "planted": len(plants), "song_seconds": song_s, "table_rows": int(db.num_fingerprints()), "topn": topn}
    S.find_duplicates(db, sids=np.arange(1, min(total, 200) + 1), topn=topn, min_aligned=1, min_coverage=0.5)   # warm-up
    t0 = time.perf_counter()
    res = S.find_duplicates(db, topn=topn, min_aligned=1, min_coverage=0.5)
    dt = time.perf_counter() - t0
    out["find_duplicates_s"] = dt
    out["songs_per_s"] = total / dt
    k = min(total, 2000)                      # the library call alone, on the first songs
    t0 = time.perf_counter()
    db.table.match_songs(np.arange(1, k + 1, dtype=np.uint32), topn=topn)
    out["match_songs_alone"] = {"songs": k, "songs_per_s": k / (time.perf_counter() - t0)}
    p = res["pairs"]
    want = {(min(a, b), max(a, b)): cut for a, b, cut in plants}
    key = [(int(a), int(b)) for a, b in zip(p["a"], p["b"])]
    is_plant = np.array([k in want for k in key], bool)
    cov_small = np.maximum(p["coverage_a"], p["coverage_b"])        # coverage of the smaller song
    cov_large = np.minimum(p["coverage_a"], p["coverage_b"])
    un, pl = ~is_plant, is_plant
    # pairs of two plants of one source, or a plant and another plant's source, are related too: none by construction
    # (every source is drawn once)
    out["pairs_seen"] = int(len(p))
    out["planted_found_at_any_count"] = int(pl.sum())
    out["unrelated"] = {"pairs": int(un.sum()), "aligned_max": int(p["aligned"][un].max(initial=0)),
                        "aligned_p999": float(np.percentile(p["aligned"][un], 99.9)) if un.any() else 0.0,
                        "coverage_small_max": float(cov_small[un].max(initial=0.0))}
    cp = np.array([want[k] == 0 for k, f in zip(key, is_plant) if f], bool)
    al_pl, cs_pl, cl_pl = p["aligned"][pl], cov_small[pl], cov_large[pl]
    out["planted_copies"] = {"pairs": int(cp.sum()), "aligned_min": int(al_pl[cp].min(initial=1 << 30)),
                             "coverage_small_min": float(cs_pl[cp].min(initial=9.0)), "coverage_large_min": float(cl_pl[cp].min(initial=9.0))}
    out["planted_excerpts"] = {"pairs": int((~cp).sum()), "aligned_min": int(al_pl[~cp].min(initial=1 << 30)),
                               "coverage_small_min": float(cs_pl[~cp].min(initial=9.0)),
                               "coverage_large_min": float(cl_pl[~cp].min(initial=9.0)),
                               "coverage_large_max": float(cl_pl[~cp].max(initial=0.0))}
    # at the defaults
    keep = p["aligned"] >= catalog.MIN_ALIGNED
    found = {k for k, f, kp in zip(key, is_plant, keep) if f and kp}
    ca, cb = p["coverage_a"] >= catalog.MIN_COVERAGE, p["coverage_b"] >= catalog.MIN_COVERAGE
    rel = np.where(ca & cb, "same", np.where(ca | cb, "contained", "overlap"))
    out["at_defaults"] = {
        "min_aligned": catalog.MIN_ALIGNED, "min_coverage": catalog.MIN_COVERAGE,
        "recall": len(found) / max(1, len(want)),
        "false_pairs": int((keep & un).sum()),
        "copies_labelled_same": int(sum(1 for k, r, kp, f in zip(key, rel, keep, is_plant) if f and kp and want[k] == 0 and r == "same")),
        "excerpts_labelled_contained": int(sum(1 for k, r, kp, f in zip(key, rel, keep, is_plant) if f and kp and want[k] != 0 and r == "contained")),
        "excerpts_labelled_same": int(sum(1 for k, r, kp, f in zip(key, rel, keep, is_plant) if f and kp and want[k] != 0 and r == "same")),
        "unrelated_labelled_same_or_contained": int(sum(1 for r, kp, f in zip(rel, keep, is_plant) if not f and kp and r != "overlap")),
    }
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", default="5000,20000")
    ap.add_argument("--song-seconds", type=int, default=10)
    ap.add_argument("--planted", type=float, default=0.02)
    ap.add_argument("--gather-rows", type=int, default=1 << 28)
    ap.add_argument("--topn", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shazam_amd as S
    ctx = S.get_context(0)
    res = {"device": ctx.device_info()["name"]}
    if a.gather_rows:
        res["gather"] = gather_bench(S, ctx, a.gather_rows)
    res["catalogues"] = [catalogue_bench(S, ctx, int(n), a.song_seconds, a.planted, a.topn) for n in a.songs.split(",") if n]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
