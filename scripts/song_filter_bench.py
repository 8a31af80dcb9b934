"""Cost of the song filter (shz_set_song_filter) on a bench_db-style synthetic table: Table.match of batches of queries, four
ways on the same inputs, in one process --
  no filter        the default routes (vote tiles);
  allow all        a filter that lists every song: the price of the route (8-byte votes, one pass, the full sort, the fold
                   over runs) and of the stage (two kernels, a scan, one read-back) with nothing dropped;
  allow 50 %       the songs of the lower half of the ids (the queries' true songs among them);
  allow 1 %        the queries' true songs and nothing else (query i is cut from song 1 + i mod songs / 100).
The hashes are extracted once; only the match is timed, warm, between two events on the context's stream
(Context.timer_start / timer_stop), reps calls per case, the cases interleaved round by round so that drift hits all of them
alike; the median round is reported with the spread, as ms per query, beside top-1 (the share of queries whose first result is
their true song) and the kept votes.  Prints one JSON line per case, and writes them to --out.
--plain-only: the no-filter case alone, through calls every earlier version of the library has (for an A/B of the untouched
path against another build, run alternately).
python scripts/song_filter_bench.py [--songs 10000] [--queries 200] [--batch 200] [--reps 5] [--rounds 5] [--out FILE]"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import shazam_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--songs", type=int, default=10000)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--queries", type=int, default=200)
ap.add_argument("--query-seconds", type=float, default=10.0)
ap.add_argument("--batch", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()

ctx = S.get_context(0)
t = S.Table(ctx)
n = int(a.seconds * 44100)
for c0 in range(0, a.songs, 500):
    nc = min(500, a.songs - c0)
    pcm = ctx.synth_pcm(4321, c0, nc, n, 4000, 1500)
    k, t1, ho, _ = ctx.fingerprint_batch(pcm, np.arange(nc + 1, dtype=np.uint64) * n, pcm_device=True)
    pcm.free()
    t.insert_clips(k, t1, ho, c0 + 1)
t.finalize()
n_true = max(1, a.songs // 100)
nq, qn = a.queries, int(a.query_seconds * 44100)
src = ctx.synth_pcm(4321, 0, min(n_true, nq), n, 4000, 1500).download(np.int16, min(n_true, nq) * n).reshape(-1, n)
truth = np.asarray([1 + i % n_true for i in range(nq)], np.uint32)
room = n - qn - 131 * nq
assert room > 0, "songs too short for these queries"
cuts = [src[i % n_true, room // 2 + 131 * i: room // 2 + 131 * i + qn] for i in range(nq)]
qk, qt, qho = S.fingerprint_batch(cuts, ctx=ctx)
batches = []
for q0 in range(0, nq, a.batch):
    q1 = min(nq, q0 + a.batch)
    lo, hi = int(qho[q0]), int(qho[q1])
    batches.append((qk[lo:hi], qt[lo:hi], (qho[q0:q1 + 1] - qho[q0]).astype(np.uint64)))

CASES = [("no filter", None)]
if not a.plain_only:
    CASES += [("allow all", np.arange(1, a.songs + 1, dtype=np.uint32)),
              ("allow 50 %", np.arange(1, a.songs // 2 + 1, dtype=np.uint32)),
              ("allow 1 %", np.arange(1, n_true + 1, dtype=np.uint32))]


def run(ids):
    """all batches once; the filter is set once around them, as a caller with a fixed set would"""
    if ids is None:
        return [t.match(*b, 2) for b in batches]
    with ctx.songs(only=ids):
        return [t.match(*b, 2) for b in batches]


ms = {name: [] for name, _ in CASES}
res = {}
for name, ids in CASES:               # warm: workspace grown, code objects loaded
    for _ in range(2):
        res[name] = run(ids)
for _ in range(a.rounds):
    for name, ids in CASES:
        ctx.sync()
        ctx.timer_start(0)
        for _ in range(a.reps):
            run(ids)
        ms[name].append(ctx.timer_stop(0) / a.reps / nq)
if not a.plain_only:
    for x, y in zip(res["allow all"], res["no filter"]):
        for name in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs"):
            assert np.array_equal(x[name], y[name]), name
lines = []
for name, _ in CASES:
    v = np.asarray(ms[name])
    sid = np.concatenate([r["sid"][:, 0] for r in res[name]])
    nres = np.concatenate([r["nres"] for r in res[name]])
    lines.append({"case": name, "label": a.label, "songs": a.songs, "queries": nq, "batch": a.batch, "query_seconds": a.query_seconds,
                  "ms_per_query": round(float(np.median(v)), 5), "ms_min": round(float(v.min()), 5), "ms_max": round(float(v.max()), 5),
                  "rounds": v.round(5).tolist(), "top1": float(((sid == truth) & (nres > 0)).mean()),
                  "kept_votes": int(sum(int(r["npairs"].sum()) for r in res[name])), "device": ctx.device_info()["name"]})
    print(json.dumps(lines[-1]))
if a.out:
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
