"""bench_db's query benchmark under the key cap (shz_set_key_cap): the table is built once (bench_db.build_table), then
bench_db.run_queries -- its own queries, its own loop and its own timing: host wall time of the match call per batch --
runs once per cap inside `with ctx.key_cap(cap)`, cap 0 (off) first and last.  The caps are those that
shazam_amd.keycap.cap_for gives the table's key histogram for keep = 1, 0.99, 0.95, 0.9, 0.8, 0.5.  One JSON line per run:
ms per query (the median batch), top-1 accuracy, the votes expanded and their share of the cap-off run's.
scripts/key_cap_curves.py holds the per-query figures (aligned counts, ratios) and the A/B of the cap-off path.
python scripts/key_cap_bench.py [--corpus tonal|music] [--songs 10000] [--queries 1000] [--match-batch 200] [--snr 10] [--out FILE]"""
import argparse
import json
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, ".")
import bench_db  # noqa: E402
import shazam_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--corpus", choices=("tonal", "music"), default="tonal")
ap.add_argument("--songs", type=int, default=10000)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--query-seconds", type=float, default=10.0)
ap.add_argument("--match-batch", type=int, default=200)
ap.add_argument("--snr", type=float, default=10.0)
ap.add_argument("--out", default="")
a = ap.parse_args()

ctx = S.get_context(0)
n_samples, qn = int(a.seconds * bench_db.FS), int(a.query_seconds * bench_db.FS)
tbl, _, bufs = bench_db.build_table(ctx, a.songs, a.seconds, corpus=a.corpus)
for b in bufs[:2]:
    if b is not None:
        b.free()
h = tbl.key_hist()
caps = sorted({S.keycap.cap_for(h, k) for k in (Fraction(1), Fraction(99, 100), Fraction(95, 100), Fraction(9, 10), Fraction(8, 10),
                                                Fraction(1, 2))} - {0}, reverse=True)
bench_db.run_queries(ctx, tbl, a.songs, n_samples, a.match_batch, qn, a.snr, a.match_batch, corpus=a.corpus)   # warm
lines, off_pairs = [], None
for cap in [0] + caps + [0]:
    with ctx.key_cap(cap):
        r = bench_db.run_queries(ctx, tbl, a.songs, n_samples, a.queries, qn, a.snr, a.match_batch, corpus=a.corpus)
    per = r["batch_ms"] / r["sizes"]
    off_pairs = r["pairs"] if off_pairs is None else off_pairs
    lines.append({"cap": cap, "rows_kept": S.keycap.rows_kept(h, cap), "table_rows": int(h["rows"].sum()), "corpus": a.corpus,
                  "songs": a.songs, "queries": a.queries, "match_batch": a.match_batch, "query_seconds": a.query_seconds, "snr": a.snr,
                  "ms_per_query": round(float(np.median(per)), 5), "ms_min": round(float(per.min()), 5),
                  "ms_max": round(float(per.max()), 5), "top1": r["correct"] / a.queries, "votes": int(r["pairs"]),
                  "votes_kept": round(r["pairs"] / max(off_pairs, 1), 5), "device": ctx.device_info()["name"]})
    print(json.dumps(lines[-1]), flush=True)
if a.out:
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
