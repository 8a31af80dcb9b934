"""What the key cap (shz_set_key_cap) does to a bench_db table: the table's key-size histogram, and for the caps that
shazam_amd.keycap.cap_for gives for keep = 1, 0.99, 0.95, 0.9, 0.8, 0.5 -- at every --snr -- the share of votes kept, top-1
accuracy, the true song's median aligned count and its median ratio to the runner-up, and ms per query by bench_db's own
timing (host wall time of the match call, whole batch / queries; the median over --rounds rounds, the caps interleaved
round by round).  The corpus, the tracks and the queries are bench_db's (build_table / make_queries); the queries are
fingerprinted once per SNR and only the match runs per cap.  Prints one JSON line per fact and appends them to --out.
--off-only: the cap-off timing alone, through calls every earlier build has -- for an A/B of the untouched path against
another build on the same box, run alternately.
python scripts/key_cap_curves.py [--corpus tonal|music] [--songs 10000] [--queries 200] [--snr 10 0] [--rounds 7] [--out FILE]"""
import argparse
import json
import sys
import time
from fractions import Fraction

import numpy as np

sys.path.insert(0, ".")
import bench_db  # noqa: E402
import shazam_amd as S  # noqa: E402

KEEPS = (Fraction(1), Fraction(99, 100), Fraction(95, 100), Fraction(9, 10), Fraction(8, 10), Fraction(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=("tonal", "music"), default="tonal")
    ap.add_argument("--songs", type=int, default=10000)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--query-seconds", type=float, default=10.0)
    ap.add_argument("--snr", type=float, nargs="+", default=[10.0, 0.0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = S.get_context(0)
    n_samples, qn, nq = int(a.seconds * bench_db.FS), int(a.query_seconds * bench_db.FS), a.queries
    tbl, _, bufs = bench_db.build_table(ctx, a.songs, a.seconds, corpus=a.corpus)
    for b in bufs[:2]:
        if b is not None:
            b.free()
    base = {"label": a.label, "corpus": a.corpus, "songs": a.songs, "queries": nq, "query_seconds": a.query_seconds,
            "device": ctx.device_info()["name"]}
    lines = []

    def emit(d):
        lines.append({**base, **d})
        print(json.dumps(lines[-1]), flush=True)

    caps = [0]
    if not a.off_only:
        h = tbl.key_hist()
        emit({"fact": "key_hist", "keys": h["keys"].tolist(), "rows": h["rows"].tolist(), "max_rows": h["max_rows"],
              "n_keys": h["n_keys"], "table_rows": int(tbl.rows()[0])})
        caps = [(float(k), S.keycap.cap_for(h, k)) for k in KEEPS]
        emit({"fact": "caps", "caps": [{"keep": k, "cap": c, "rows_kept": S.keycap.rows_kept(h, c)} for k, c in caps]})
        caps = [0] + sorted({c for _, c in caps if c}, reverse=True)
    rng = np.random.default_rng(99)
    tids, starts = rng.integers(0, a.songs, nq), rng.integers(0, n_samples - qn, nq)
    for snr in a.snr:
        q, qb = bench_db.make_queries(ctx, tids, starts, qn, snr, corpus=a.corpus)
        k, t1, ho, _ = ctx.fingerprint_batch(q, np.arange(nq + 1, dtype=np.uint64) * qn, fs=bench_db.FS, pcm_device=True)
        for b in {id(b): b for b in qb}.values():
            b.free()

        def run(cap):
            if cap == 0:                       # (the plain call: what the parent build runs too)
                ctx.sync()
                t0 = time.perf_counter()
                res = tbl.match(k, t1, ho, 2)
                return res, (time.perf_counter() - t0) * 1e3 / nq
            with ctx.key_cap(cap):
                ctx.sync()
                t0 = time.perf_counter()
                res = tbl.match(k, t1, ho, 2)
                return res, (time.perf_counter() - t0) * 1e3 / nq

        ms, res, pairs = {c: [] for c in caps}, {}, {}
        for c in caps:                          # warm: workspace grown, code objects loaded
            run(c)
            res[c], _ = run(c)
            pairs[c] = tbl.match_stats()["pairs"]
        for _ in range(a.rounds):
            for c in caps:
                ms[c].append(run(c)[1])
        for c in caps:
            r, v = res[c], np.asarray(ms[c])
            hit = (r["nres"] > 0) & (r["sid"][:, 0] == 1 + tids)
            true = np.where(hit, r["aligned"][:, 0], np.where((r["nres"] > 1) & (r["sid"][:, 1] == 1 + tids), r["aligned"][:, 1], 0))
            other = np.where(hit, np.where(r["nres"] > 1, r["aligned"][:, 1], 0), np.where(r["nres"] > 0, r["aligned"][:, 0], 0))
            ratio = true[other > 0] / other[other > 0]
            emit({"fact": "cap", "snr": snr, "cap": c, "votes": int(pairs[c]), "votes_kept": round(pairs[c] / max(pairs[0], 1), 5),
                  "ms_per_query": round(float(np.median(v)), 5), "ms_min": round(float(v.min()), 5), "ms_max": round(float(v.max()), 5),
                  "top1": float(hit.mean()), "true_aligned_median": float(np.median(true)),
                  "true_over_runner_up_median": round(float(np.median(ratio)), 3) if len(ratio) else None})
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
