"""Cost of the tolerant vote (shz_set_vote_tolerance) on the synthetic table: ms per query of Table.match for 1 and 200
queries of 10 s, through the default routes, the parent's full sort (SHZ_MATCH_FULL_SORT: 8-byte votes sorted once, like the
tolerant route), the tolerant route forced at tolerance 0, and tolerances 1, 3 and 15.  The hashes are extracted once; only
the match is timed (host arrays in, result arrays out).  Prints one JSON line per case.
python scripts/vote_tol_bench.py [songs] [reps]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import shazam_amd as S  # noqa: E402
from shazam_amd import _ffi  # noqa: E402

songs = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
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
# 200 queries of 10 s, cut from 200 songs at places that are no multiple of the hop
nq, qn = 200, 10 * 44100
src = ctx.synth_pcm(4321, 0, nq, n, 4000, 1500).download(np.int16, nq * n).reshape(nq, n)
cuts = [src[i, 5 * 44100 + 131 * i: 5 * 44100 + 131 * i + qn] for i in range(nq)]
qk, qt, qho = S.fingerprint_batch(cuts, ctx=ctx)
one = (qk[:int(qho[1])], qt[:int(qho[1])], qho[:2])

CASES = [("default routes", 0, None, False), ("full sort", 0, None, True), ("tolerant route, tol 0", _ffi.DEBUG_VOTE_TOLERANT_ROUTE, None, False),
         ("tol 1", 0, 1, False), ("tol 3", 0, 3, False), ("tol 15", 0, 15, False)]
for label, queries in (("1 query", one), ("200 queries", (qk, qt, qho))):
    n_queries = len(queries[2]) - 1
    for name, debug, tol, full_sort in CASES:
        ctx.set_debug(debug)
        try:
            for _ in range(3):
                res = t.match(*queries, 2, full_sort=full_sort, delta_tol=tol)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                res = t.match(*queries, 2, full_sort=full_sort, delta_tol=tol)
            dt = (time.perf_counter() - t0) / reps
        finally:
            ctx.set_debug(0)
        right = int((res["sid"][:, 0] == np.arange(1, n_queries + 1)).sum())
        print(json.dumps({"case": name, "queries": label, "songs": songs, "ms_per_query": round(dt * 1e3 / n_queries, 4),
                          "votes": int(res["npairs"].sum()), "top1_right": right, "top1_aligned_mean": float(res["aligned"][:, 0].mean())}))
