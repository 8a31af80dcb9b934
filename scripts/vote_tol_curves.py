#!/usr/bin/env python3
"""The measurements of DESIGN.md 3.7j, on the CPU: oracle + twins (tests/warp_twin.py, tests/rows_warp_twin.py,
tests/vote_tol_twin.py), no GPU.

  curves   3.7e's tempo curve (same table, queries and misses as scripts/warp_curves.py) with the vote summed over tol + 1
           neighbouring offset bins: the right song's count relative to its ONE-bin count at the true pair, mean / worst over
           the 24 curves, where the mean falls to half of its own value at the true pair, and the best wrong song's count.
  long     3.7h's long-track case: a track of --minutes as song 1 among three 30 s songs, and its copy played half a step of
           the default speed ladder (46 / 65536 = 0.07 %) fast; the copy's rows warped by the nearest rung (65536: it misses by
           the half-step) and by the true factor, matched against the table.

    python scripts/vote_tol_curves.py curves [--seconds 10] [--tols 0 1 2 4]
    python scripts/vote_tol_curves.py long [--minutes 3] [--tols 0 2 4]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rows_warp_twin as RW  # noqa: E402
import speed_twin as T  # noqa: E402
import warp_twin as W  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402
from oracle import synth  # noqa: E402
from vote_tol_twin import vote_tol  # noqa: E402
from warp_curves import TEMPO_MISS, TRUE, half_crossing  # noqa: E402

R = 44100


def matches_of(k, t1, table):
    pairs = sorted(set(zip(np.asarray(k).tolist(), np.asarray(t1).tolist())))
    return [(sid, off - q) for kk, q in pairs for sid, off in table.get(kk, ())]


def right_and_wrong(matches, sid, tol):
    ranked = vote_tol(matches, tol, 8)
    right = [a for s, _, a in ranked if s == sid]
    wrong = [a for s, _, a in ranked if s != sid]
    return (right[0] if right else 0), (wrong[0] if wrong else 0)


def curves(a):
    songs = [W.notes_clip(7, c, 30) for c in range(4)]
    table = W.table_of([O.fingerprint_keys(s)[:2] for s in songs])
    rows = {tol: [] for tol in a.tols}
    own = {tol: [] for tol in a.tols}
    wrong = {tol: 0 for tol in a.tols}
    for c in range(4):
        for tempo, pitch in TRUE:
            x = W.notes_clip(7, c, 8 / tempo + a.seconds + 0.1, tempo, pitch)
            s0 = int(round(8 / tempo * R))
            _, _, f, t = O.fingerprint_keys(x[s0:s0 + int(a.seconds * R)])
            t16, f16 = W.q16(tempo), W.q16(pitch)
            per_miss = [matches_of(*W.warp_pair_tf(f, t, int(round(t16 * (1 + m / 100))), f16), table) for m in TEMPO_MISS]
            true0 = right_and_wrong(per_miss[TEMPO_MISS.index(0)], c + 1, 0)[0]
            for tol in a.tols:
                got = [right_and_wrong(m, c + 1, tol) for m in per_miss]
                rows[tol].append([r / max(true0, 1) for r, _ in got])
                own[tol].append([r / max(got[TEMPO_MISS.index(0)][0], 1) for r, _ in got])
                wrong[tol] = max(wrong[tol], max(w for _, w in got))
            print(f"song {c} true ({tempo}, {pitch}): one bin {true0}", flush=True)
    print(f"\n## tempo axis, queries of {a.seconds} s, {len(rows[a.tols[0]])} curves; counts relative to the one-bin count at the true pair")
    print("| tol | | " + " | ".join(f"{m:+g}" for m in TEMPO_MISS) + " | half of its own count at | best wrong song |")
    for tol in a.tols:
        arr, rel = np.asarray(rows[tol]), np.asarray(own[tol]).mean(0).tolist()
        hw = f"-{half_crossing(TEMPO_MISS, rel, -1):.2f} % / +{half_crossing(TEMPO_MISS, rel, 1):.2f} %"
        print(f"| {tol} | mean | " + " | ".join(f"{v:.2f}" for v in arr.mean(0)) + f" | {hw} | {wrong[tol]} |")
        print(f"| {tol} | worst | " + " | ".join(f"{v:.2f}" for v in arr.min(0)) + " | | |")


def long_track(a):
    n = int(a.minutes * 60 * R)
    track = synth.music_clip(7, 9, n)
    others = [synth.music_clip(7, c, 30 * R) for c in range(3)]
    half = 46                                                    # half of speed.DEFAULT_STEP_Q16 = 92
    s = (65536 + half) / 65536
    copy = T.speed_up(track, s)
    fp = [O.fingerprint_keys(x)[:2] for x in [track] + others + [copy]]
    rk = np.concatenate([k for k, _ in fp]).astype(np.int64)
    ro = np.concatenate([t for _, t in fp]).astype(np.int64)
    rs = np.concatenate([np.full(len(k), i + 1, np.int64) for i, (k, _) in enumerate(fp)])
    table = RW.table_of_rows(rk, rs, ro)
    ck, co = fp[-1]
    print(f"# track of {a.minutes} min: {len(fp[0][0])} rows, {int(fp[0][1].max()) + 1} frames; its copy at {s:.5f}: {len(ck)} rows (song 5)")
    print("| tol | rung 65536 (misses by 0.07 %): track | best other song | true factor: track | best other song |")
    for tol in a.tols:
        cells = []
        for t16 in (65536, 65536 + half):
            wk, wo, _ = RW.warp_rows(ck, co, t16, t16)
            ranked = [r for r in vote_tol(matches_of(wk, wo, table), tol, 8) if r[0] != 5]
            right = [x[2] for x in ranked if x[0] == 1]
            wrong = [x[2] for x in ranked if x[0] != 1]
            cells += [str(right[0] if right else 0), str(wrong[0] if wrong else 0)]
        print(f"| {tol} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["curves", "long"])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--tols", type=int, nargs="+", default=None)
    a = ap.parse_args()
    if a.what == "curves":
        a.tols = a.tols or [0, 1, 2, 4]
        curves(a)
    else:
        a.tols = a.tols or [0, 2, 4]
        long_track(a)
