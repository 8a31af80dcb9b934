"""Cost of the vote floor (shz_set_vote_floor) on the table and queries of scripts/vote_tol_bench.py: Table.match of 1 and of
200 queries of 10 s, three ways on the same inputs -- floor off (the default routes), full_sort=True (8-byte votes sorted once:
what the floor's route does before its two histogram kernels) and floor on.  The hashes are extracted once; only the match is
timed, warm, between two events on the context's stream (Context.timer_start / timer_stop), reps calls per case, the cases
interleaved round by round so that drift hits all of them alike; the median round is reported, with the spread.  Prints one
JSON line per case; `ratio_to_full_sort` is the honest price of the two kernels and the wider read-back.
python scripts/vote_floor_bench.py [songs] [reps] [rounds]"""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import shazam_amd as S  # noqa: E402

songs = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ctx = S.get_context(0)
t = S.Table(ctx)
n = 30 * 44100
for c0 in range(0, songs, 500):
    nc = min(500, songs - c0)
    pcm = ctx.synth_pcm(4321, c0, nc, n, 4000, 1500)
    k, t1, ho, _ = ctx.fingerprint_batch(pcm, np.arange(nc + 1, dtype=np.uint64) * n, pcm_device=True)
    pcm.free()
    t.insert_clips(k, t1, ho, c0 + 1)
t.finalize()
nq, qn = 200, 10 * 44100
src = ctx.synth_pcm(4321, 0, nq, n, 4000, 1500).download(np.int16, nq * n).reshape(nq, n)
cuts = [src[i, 5 * 44100 + 131 * i: 5 * 44100 + 131 * i + qn] for i in range(nq)]
qk, qt, qho = S.fingerprint_batch(cuts, ctx=ctx)
one = (qk[:int(qho[1])], qt[:int(qho[1])], qho[:2])

CASES = [("floor off", dict()), ("full sort", dict(full_sort=True)), ("floor on", dict(floor=True))]
for label, queries in (("1 query", one), ("200 queries", (qk, qt, qho))):
    n_queries = len(queries[2]) - 1
    ms = {name: [] for name, _ in CASES}
    res = {}
    for name, kw in CASES:               # warm: workspace grown, code objects loaded
        for _ in range(3):
            res[name] = t.match(*queries, 2, **kw)
    for _ in range(rounds):
        for name, kw in CASES:
            ctx.sync()
            ctx.timer_start(0)
            for _ in range(reps):
                t.match(*queries, 2, **kw)
            ms[name].append(ctx.timer_stop(0) / reps)
    for name in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs"):
        assert np.array_equal(res["floor on"][name], res["floor off"][name]), name
    base = float(np.median(ms["full sort"]))
    for name, _ in CASES:
        v = np.asarray(ms[name])
        print(json.dumps({"case": name, "queries": label, "songs": songs, "ms_per_call": round(float(np.median(v)), 4),
                          "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                          "ratio_to_full_sort": round(float(np.median(v)) / base, 3), "votes": int(res[name]["npairs"].sum()),
                          "songs_with_a_vote_mean": float(res["floor on"]["song_hist"].sum(axis=1).mean())}))
