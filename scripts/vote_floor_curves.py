"""What the vote floor's score says, on the music-like synthetic corpus of `bench_db.py --corpus music`: the distribution of
shazam_amd.floor.score for queries whose song IS in the table and for queries whose song was DELETED from it, over catalogue
sizes, query SNRs and vote tolerances 0 and 2.  Per case one JSON line: the quantiles of both groups' scores (of the rank-0
result against the query's own song histogram; "songs" and "bins"), how many of each group have no score (nothing to fit, or
no result at all), and the min_score that separates the groups if one does: the midpoint between the lowest score of a
present query that was answered RIGHT and the highest score of an absent one, when the former is the larger.
Queries: 10 s crops at arbitrary offsets under traffic-like noise.  The absent group: the same crops after delete_songs of
their tracks -- the same audio, the same table but for those tracks.
python scripts/vote_floor_curves.py [queries] [sizes ...]      (default: 200 queries; 1000 and 10000 songs)"""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import shazam_amd as S  # noqa: E402
from bench_db import FS, build_table, make_queries  # noqa: E402
from shazam_amd import floor  # noqa: E402

nq = int(sys.argv[1]) if len(sys.argv) > 1 else 200
sizes = [int(x) for x in sys.argv[2:]] or [1000, 10000]
SECONDS, QSECONDS = 30.0, 10.0
ctx = S.get_context(0)


def scores(res, which):
    hist = res["song_hist"] if which == "songs" else res["bin_hist"]
    return [floor.score(int(res["aligned"][q, 0]), hist[q]) if res["nres"][q] else None for q in range(len(res["nres"]))]


def quant(v):
    v = np.asarray([x for x in v if x is not None and np.isfinite(x)], np.float64)
    if not len(v):
        return None
    return [round(float(x), 2) for x in np.quantile(v, [0.0, 0.05, 0.5, 0.95, 1.0])]


for songs in sizes:
    rng = np.random.default_rng(4242 + songs)
    n_samples, qn = int(SECONDS * FS), int(QSECONDS * FS)
    tids = rng.choice(songs, nq, replace=False)
    starts = rng.integers(0, n_samples - qn, nq)
    hashes = {}
    for snr in (0.0, -6.0):
        q, bufs = make_queries(ctx, tids, starts, qn, snr, corpus="music")
        k, t1, ho, _ = ctx.fingerprint_batch(q, np.arange(nq + 1, dtype=np.uint64) * qn, fs=FS, pcm_device=True)
        hashes[snr] = (k, t1, ho)
        for b in {id(b): b for b in bufs}.values():
            b.free()
    tbl, _, (kbuf, tbuf, _) = build_table(ctx, songs, SECONDS, corpus="music")
    kbuf.free()
    tbuf.free()
    present = {(snr, tol): tbl.match(*hashes[snr], 2, delta_tol=tol, floor=True) for snr in hashes for tol in (0, 2)}
    tbl.delete_songs((tids + 1).astype(np.uint32))
    absent = {(snr, tol): tbl.match(*hashes[snr], 2, delta_tol=tol, floor=True) for snr in hashes for tol in (0, 2)}
    tbl.close()
    for (snr, tol), pres in present.items():
        abst = absent[snr, tol]
        right = (pres["nres"] > 0) & (pres["sid"][:, 0] == tids + 1)
        out = {"songs": songs, "snr_db": snr, "delta_tol": tol, "queries": nq, "present_top1_right": int(right.sum()),
               "present_aligned_median": float(np.median(pres["aligned"][:, 0])), "absent_aligned_max": int(abst["aligned"][:, 0].max()),
               "songs_with_a_vote_median": float(np.median(pres["song_hist"].sum(axis=1)))}
        for which in ("songs", "bins"):
            sp, sa = scores(pres, which), scores(abst, which)
            lo = [s for s, r in zip(sp, right) if r and s is not None]
            hi = [s for s in sa if s is not None]
            sep = None
            if lo and hi and min(lo) > max(hi):
                sep = round((min(lo) + max(hi)) / 2, 2)
            out[which] = {"present_q0_5_50_95_100": quant(sp), "absent_q0_5_50_95_100": quant(sa),
                          "present_right_without_score": int(sum(1 for s, r in zip(sp, right) if r and s is None)),
                          "absent_without_score": int(sum(1 for s in sa if s is None)),
                          "present_right_min": None if not lo else round(min(lo), 2), "absent_max": None if not hi else round(max(hi), 2),
                          "min_score_that_separates": sep}
        print(json.dumps(out), flush=True)
