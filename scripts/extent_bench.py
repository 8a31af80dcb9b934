#!/usr/bin/env python3
"""extent_bench.py -- the match extents (csrc/shz_extent.hip, shazam_amd/extent.py) measured against the match.

    python scripts/extent_bench.py [--songs 20000] [--queries 200] [--reps 10] [--catalogue-songs 500] [--out FILE.json]

A table of --songs music-like synthetic songs of 10 s (shz_synth_corpus).  --queries queries of 10 s (215 hops): 64 hops of
traffic-like noise, 86 hops cut from song q at frame 70 (hop-aligned), 65 hops of noise -- so the true stretch is known: the
query frames 64 .. 149.  Timed with the context's hipEvent timers (shz_timer_start / _stop), 3 warm-up calls and the median
of --reps, the cases alternating: Table.match (topn 5) alone, and Table.match followed by extent.extents_of on its results,
for the whole batch and for one query; then Table.match_songs and Table.match_songs + Table.match_songs_extents on
--catalogue-songs songs (each song's candidates: its five strongest partners).  The ratio (match + extents) / match is the
number to write down.
From the same run, the distributions DENSE_MIN_COUNT (shazam_amd/extent.py) is set by, over all queries: pairs per bucket of
the TRUE song in the buckets that lie wholly inside the stretch; pairs per occupied bucket of the true song OUTSIDE it (the
chance pairs dense_span has to ignore); of unrelated songs at the true song's delta; and of the unrelated runners-up of the
match at their own best delta (the most favourable bin chance offers them).  Prints one JSON line; --out also writes it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, FS, HOP = 77, 44100, 2048
PRE, CUT0, CUTN, POST = 64, 70, 86, 65


def build_table(S, ctx, n_songs, ln):
    t = S.Table(ctx)
    cap = 8000
    for b0 in range(0, n_songs, 1000):
        nb = min(1000, n_songs - b0)
        pcm = ctx.synth_corpus(1, SEED, b0, nb, ln)
        ok, ot = ctx.alloc(nb * cap * 4), ctx.alloc(nb * cap * 4)
        _, _, ho, _ = ctx.fingerprint_batch(pcm.ptr, np.arange(nb + 1, dtype=np.uint64) * ln, pcm_device=True, out_key=ok, out_t1=ot)
        t.insert_clips(ok.ptr, ot.ptr, ho, b0 + 1, device=True)
        for x in (pcm, ok, ot):
            x.free()
    t.finalize()
    return t


def make_queries(S, ctx, nq, ln):
    src = ctx.synth_corpus(1, SEED, 0, nq, ln)
    songs = src.download(np.int16, nq * ln).reshape(nq, ln)
    src.free()
    nz = ctx.synth_corpus(2, SEED + 1, 0, 2 * nq, PRE * HOP + POST * HOP)
    noise = nz.download(np.int16, 2 * nq * (PRE + POST) * HOP).reshape(2 * nq, -1)
    nz.free()
    clips = [np.concatenate([noise[2 * q, :PRE * HOP], songs[q, CUT0 * HOP:(CUT0 + CUTN) * HOP], noise[2 * q + 1, :POST * HOP]])
             for q in range(nq)]
    return S.fingerprint_batch(clips, ctx=ctx)


def timed(ctx, cases, warm=3, reps=10):
    """median / min / max hipEvent ms of every case, the cases alternating inside every repetition"""
    for fn in cases.values():
        for _ in range(warm):
            fn()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            ctx.timer_start(0)
            fn()
            ms[k].append(ctx.timer_stop(0))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ms.items()}


def dist(x):
    x = np.asarray(x)
    if len(x) == 0:
        return {"n": 0}
    return {"n": int(len(x)), "min": int(x.min()), "p01": float(np.percentile(x, 1)), "p10": float(np.percentile(x, 10)),
            "median": float(np.median(x)), "p90": float(np.percentile(x, 90)), "p99": float(np.percentile(x, 99)), "max": int(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--catalogue-songs", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import shazam_amd as S
    from shazam_amd import _ffi
    from shazam_amd.extent import DENSE_MIN_COUNT, dense_span, extents_of
    ctx = S.get_context(0)
    ln = 10 * FS
    t = build_table(S, ctx, a.songs, ln)
    nq = min(a.queries, a.songs)
    qk, qt, qho = make_queries(S, ctx, nq, ln)
    one = (qk[:int(qho[1])], qt[:int(qho[1])], qho[:2])
    out = {"device": ctx.device_info()["name"], "lib": os.path.basename(_ffi.LIB_PATH), "songs": a.songs,
           "table_rows": int(t.rows()[0]), "segments": t.segments(), "reps": a.reps}
    for label, q in (("batch", (qk, qt, qho)), ("one_query", one)):
        res = t.match(*q, 5)
        ext = extents_of(t, *q, res)
        assert np.array_equal(ext["count"], res["aligned"])
        r = timed(ctx, {"match": lambda: t.match(*q, 5),
                        "match_then_extents": lambda: extents_of(t, *q, t.match(*q, 5)),
                        "extents": lambda: extents_of(t, *q, res),
                        "extents_no_hist": lambda: extents_of(t, *q, res, hist=False)}, reps=a.reps)
        r.update({"queries": len(q[2]) - 1, "hashes": int(q[2][-1]), "pairs": int(res["npairs"].sum()),
                  "candidates": int(res["nres"].sum()), "hits": int(ext["count"].sum()),
                  "ratio_match_then_extents_over_match": r["match_then_extents"]["median_ms"] / r["match"]["median_ms"],
                  "ratio_extents_over_match": r["extents"]["median_ms"] / r["match"]["median_ms"]})
        out[label] = r
    # the two distributions of dense_span's min_count, and what it buys over q_first / q_last
    res = t.match(qk, qt, qho, 5)
    ext = extents_of(t, qk, qt, qho, res)
    true_b, noise_b, stray_b, raw_out, dense_out, right = [], [], [], 0, 0, 0
    for q in range(nq):
        sh = int(ext["shift"][q])
        inside = [b for b in range(64) if (b << sh) >= PRE and ((b + 1) << sh) - 1 <= PRE + CUTN - 1]
        for c in range(int(res["nres"][q])):
            h = ext["hist"][q, c]
            if int(res["sid"][q, c]) == q + 1:
                if c == 0:
                    right += 1
                true_b.extend(h[inside].tolist())
                outside = [b for b in range(64) if ((b + 1) << sh) - 1 < PRE or (b << sh) > PRE + CUTN - 1]
                stray_b.extend(h[outside][h[outside] > 0].tolist())
                w = 1 << sh
                raw_out += int(ext["q_first"][q, c] < PRE or ext["q_last"][q, c] > PRE + CUTN - 1)
                span = dense_span(h, sh)
                dense_out += int(span is None or span[0] <= PRE - w or span[1] > PRE + CUTN - 1 + w)
            else:
                noise_b.extend(h[h > 0].tolist())
    # unrelated songs at the TRUE song's delta: five a query, taken at fixed strides through the table
    top_is_true = res["sid"][:, 0] == np.arange(1, nq + 1)
    other = ((np.arange(nq)[:, None] + 1 + 37 * (1 + np.arange(5))[None, :]) % a.songs + 1).astype(np.uint32)
    d0 = np.repeat(res["delta"][:, :1].astype(np.int32), 5, axis=1)
    at_true = t.match_extents(qk, qt, qho, other, d0, d0)
    foreign_b = at_true["hist"][top_is_true]
    foreign_b = foreign_b[foreign_b > 0].tolist()
    out["dense_span"] = {"min_count": DENSE_MIN_COUNT, "top1_right": right, "queries": nq,
                         "true_pairs_per_bucket_inside_the_stretch": dist(true_b),
                         "true_song_pairs_per_occupied_bucket_outside_the_stretch": dist(stray_b),
                         "unrelated_song_at_the_true_delta_pairs_per_occupied_bucket": dist(foreign_b),
                         "unrelated_song_at_the_true_delta_candidates": int(top_is_true.sum()) * 5,
                         "unrelated_runner_up_at_its_own_best_delta_pairs_per_occupied_bucket": dist(noise_b),
                         "true_songs_whose_first_or_last_pair_lies_outside_the_stretch": raw_out,
                         "true_songs_whose_dense_span_leaves_the_stretch_by_a_bucket_or_more": dense_out}
    # the catalogue form
    n_cat = min(a.catalogue_songs, a.songs)
    sids = np.arange(1, n_cat + 1, dtype=np.uint32)
    ms = t.match_songs(sids, topn=5)
    cs, d = ms["sid"], ms["delta"].astype(np.int32)

    def cat_ext():
        return t.match_songs_extents(sids, cs, d, d, cand_n=ms["nres"], hist=False)

    e = cat_ext()
    assert np.array_equal(e["count"], ms["aligned"])
    r = timed(ctx, {"match_songs": lambda: t.match_songs(sids, topn=5),
                    "match_songs_then_extents": lambda: (t.match_songs(sids, topn=5), cat_ext()),
                    "songs_extents": cat_ext}, reps=a.reps)
    r.update({"songs": n_cat, "rows": int(ms["rows"].sum()), "pairs": int(ms["npairs"].sum()),
              "ratio_then_extents_over_match_songs": r["match_songs_then_extents"]["median_ms"] / r["match_songs"]["median_ms"]})
    out["catalogue"] = r
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()
