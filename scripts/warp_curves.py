#!/usr/bin/env python3
"""The tolerance curves of DESIGN.md 3.7e, on the CPU: oracle + tests/warp_twin.py, no GPU.

4 songs x 30 s notes_clip(7, c) in the table; queries of --seconds cut at second 8 of every song at every true (tempo,
pitch); the peaks of a query are taken once and warped by a pair that misses the truth on ONE axis by m.  Printed: the
aligned count of the right song (its best offset) relative to the count at the true pair, mean / worst over the curves, the
crossings of one half, and the separable search's first stage (pitch ladder at tempo 1) for every query.

    python scripts/warp_curves.py [--seconds 10] [--hist]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import warp_twin as W  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

R = 44100
TRUE = [(0.95, 1.0), (1.05, 1.0), (1.0, 0.95), (1.0, 1.05), (1.03, 0.97), (0.97, 1.03)]
PITCH_MISS = [-0.20, -0.15, -0.10, -0.075, -0.05, -0.025, 0, 0.025, 0.05, 0.075, 0.10, 0.15, 0.20]      # % of the factor
TEMPO_MISS = [-8, -6, -5, -4, -3, -2, -1.5, -1, -0.5, -0.25, 0, 0.25, 0.5, 1, 1.5, 2, 3, 4, 5, 6, 8]


def right_count(k, t1, table, sid):
    """(aligned count of song sid at its best offset, that offset, rank-0 (sid, delta, count))"""
    ranked, _, _ = W.aligned_votes(k, t1, table, 8)
    mine = [(a, d) for s, d, a in ranked if s == sid]
    return (mine[0] if mine else (0, 0)) + (ranked[0] if ranked else (0, 0, 0),)


def half_crossing(miss, mean, side):
    """|m| at which the mean curve first falls to 0.5 going away from 0 on one side, by linear interpolation"""
    i0 = miss.index(0)
    idx = range(i0, len(miss) - 1) if side > 0 else range(i0, 0, -1)
    for i in idx:
        j = i + side
        if mean[i] >= 0.5 > mean[j]:
            return abs(miss[i] + (miss[j] - miss[i]) * (mean[i] - 0.5) / (mean[i] - mean[j]))
    return float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--hist", action="store_true", help="print the right song's votes per offset around the cut (tempo axis)")
    a = ap.parse_args()
    songs = [W.notes_clip(7, c, 30) for c in range(4)]
    table = W.table_of([O.fingerprint_keys(s)[:2] for s in songs])
    curves = {"pitch": [], "tempo": []}
    print(f"# queries of {a.seconds} s, cut at second 8; counts at the true pair / unwarped")
    for c in range(4):
        for tempo, pitch in TRUE:
            x = W.notes_clip(7, c, 8 / tempo + a.seconds + 0.1, tempo, pitch)
            s0 = int(round(8 / tempo * R))
            k0, t0, f, t = O.fingerprint_keys(x[s0:s0 + int(a.seconds * R)])
            t16, f16 = W.q16(tempo), W.q16(pitch)
            true_n = right_count(*W.warp_pair_tf(f, t, t16, f16), table, c + 1)[0]
            plain = right_count(k0, t0, table, c + 1)
            print(f"song {c} true ({tempo}, {pitch}): {true_n} / {plain[0]} (rank 0 unwarped: {plain[2]})")
            for axis, misses in (("pitch", PITCH_MISS), ("tempo", TEMPO_MISS)):
                row = []
                for m in misses:
                    tt = t16 if axis == "pitch" else int(round(t16 * (1 + m / 100)))
                    ff = f16 if axis == "tempo" else int(round(f16 * (1 + m / 100)))
                    k, t1 = W.warp_pair_tf(f, t, tt, ff)
                    n, d, _ = right_count(k, t1, table, c + 1)
                    row.append(n / max(true_n, 1))
                    if a.hist and axis == "tempo" and abs(m) <= 0.5:
                        h = {}
                        for kk, q in zip(k.tolist(), t1.tolist()):
                            for sid, off in table.get(kk, ()):
                                if sid == c + 1 and abs(off - q - 172) <= 4:
                                    h[off - q] = h.get(off - q, 0) + 1
                        print(f"    tempo miss {m:+.2f} %: best {n} at {d}; votes per offset {sorted(h.items())}")
                curves[axis].append(row)
            # the separable search's first stage: the pitch ladder at tempo 1
            best = (0, None, None)
            for f16s in range(65536 - 36 * 92, 65536 + 36 * 92 + 1, 92):
                ranked, _, _ = W.aligned_votes(*W.warp_pair_tf(f, t, 65536, f16s), table, 1)
                if ranked and ranked[0][2] > best[0]:
                    best = (ranked[0][2], ranked[0][0], f16s)
            print(f"    stage 1 (tempo 1, 73 pitch rungs): top answer song {best[1]} with {best[0]} votes at pitch rung {best[2]}"
                  f" (true {f16}, right song {c + 1})")
    for axis, misses in (("pitch", PITCH_MISS), ("tempo", TEMPO_MISS)):
        arr = np.asarray(curves[axis])
        mean, worst, top = arr.mean(0), arr.min(0), arr.max(0)
        print(f"\n## {axis} axis, {len(arr)} curves, miss in % of the factor")
        print("| m | " + " | ".join(f"{m:+g}" for m in misses) + " |")
        print("| mean | " + " | ".join(f"{v:.2f}" for v in mean) + " |")
        print("| worst | " + " | ".join(f"{v:.2f}" for v in worst) + " |")
        print("| best | " + " | ".join(f"{v:.2f}" for v in top) + " |")
        print(f"mean falls to one half at -{half_crossing(misses, mean.tolist(), -1):.3f} % and +{half_crossing(misses, mean.tolist(), 1):.3f} %")


if __name__ == "__main__":
    main()
