#!/usr/bin/env python3
"""shared_warp_curves.py -- how far a rung of find_shared's ladder may miss, on the CPU: no GPU is needed.

    python scripts/shared_warp_curves.py [--write]

The fixture of tests/shared_warp_cases.py (recording 1 holds X sped up 1.03 and Z at tempo 1.04, pitch 0.97; recording 0 holds
both plain), the reference's peaks, the definition of tests/shared_warp_twin.py and the fold of tests/repeat_twin.py at
find_shared's defaults.  Two curves, the miss from 0 to 2 % of the rung in steps of 0.25 %, on either side:
  speed   the job (s, s) for s = 1.03 (1 + miss): the pairs that fall into X's stretch and whether the fold returns it
  tempo   the job (t, 0.97) for t = 1.04 (1 + miss), the pitch hit: the same for Z, the width of its lag range and tempo_fit
Prints the table; --write puts it into DESIGN.md between the two marker lines of 3.7r."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BEGIN, END = "<!-- shared_warp_curves: begin -->", "<!-- shared_warp_curves: end -->"
MISSES = [k * 0.0025 for k in range(-8, 9)]
FINE = [k * 0.0005 for k in range(-5, 6)]     # the speed curve once more where it falls: 0.25 % is already past its foot
X_OWN, Z_OWN = (42, 208), (446, 610)          # the two pieces in recording 1's own frames (the stretches at the true rungs)


def curve(K, shared, extent, peaks, true_t, true_f, own, both_axes, misses=MISSES):
    rows = []
    for miss in misses:
        t16 = K.q16(true_t * (1 + miss))
        f16 = K.q16(true_f * (1 + miss)) if both_axes else K.q16(true_f)
        cells = K.twin_cells(*peaks, [(1, 0, 0, -K.T_MAX, K.T_MAX)], [t16], [f16])
        best = None
        for r in K.twin_fold(cells):
            a0, a1 = extent.own_frames(r["first"], r["last"], t16)
            if min(a1, own[1]) - max(a0, own[0]) + 1 >= (own[1] - own[0] + 1) // 2 and (best is None or r["pairs"] > best["pairs"]):
                best = r
        # the pairs of the job whose t lies in the piece, at the lags within 16 of the piece's strongest cell (every cell counts
        # here, also those below min_cell_pairs)
        every = K.twin_cells(*peaks, [(1, 0, 0, -K.T_MAX, K.T_MAX)], [t16], [f16], min_cell_pairs=1)
        inside = [i for i in range(len(every["lag"])) if own[0] <= extent.own_frames(every["first"][i], every["last"][i], t16)[0] <= own[1]]
        top = max(inside, key=lambda i: every["pairs"][i], default=None)
        near = sum(every["pairs"][i] for i in inside if abs(every["lag"][i] - every["lag"][top]) <= 16) if inside else 0
        fit = None
        if best is not None:
            line = shared.cells_fit(K.stretch_cells(cells, best))
            fit = None if line is None else float(extent.tempo_of(t16, line[0]))
        rows.append((miss, near, best, fit))
    return rows


def table(rows, what):
    out = [f"| {what} rung off by | pairs of the piece near its lag | fold returns it | pairs of the stretch | lag_lo..lag_hi | tempo_fit |",
           "|---|---|---|---|---|---|"]
    for miss, near, best, fit in rows:
        if best is None:
            out.append(f"| {miss * 100:+.2f} % | {near} | no | | | |")
        else:
            out.append(f"| {miss * 100:+.2f} % | {near} | yes | {best['pairs']} | {best['lag_lo']}..{best['lag_hi']} | "
                       f"{'' if fit is None else format(fit, '.4f')} |")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="put the tables into DESIGN.md 3.7r")
    a = ap.parse_args()
    import shared_warp_cases as K
    from shazam_amd import extent, shared
    peaks = K.oracle_peaks(K.recordings())
    lines = ["Speed rungs around 1.03, the piece X (8 s, sped up 1.03 by linear interpolation):", ""]
    lines += table(curve(K, shared, extent, peaks, 1.03, 1.03, X_OWN, True), "speed")
    lines += ["", "The same from -0.25 % to +0.25 % in steps of 0.05 %:", ""]
    lines += table(curve(K, shared, extent, peaks, 1.03, 1.03, X_OWN, True, FINE), "speed")
    lines += ["", "Tempo rungs around 1.04 with the pitch rung at 0.97, the piece Z (8 s, rendered at tempo 1.04 and pitch 0.97):", ""]
    lines += table(curve(K, shared, extent, peaks, 1.04, 0.97, Z_OWN, False), "tempo")
    text = "\n".join(lines)
    print(text)
    if a.write:
        path = os.path.join(ROOT, "DESIGN.md")
        src = open(path).read()
        i, j = src.index(BEGIN) + len(BEGIN), src.index(END)
        with open(path, "w") as f:
            f.write(src[:i] + "\n" + text + "\n" + src[j:])


if __name__ == "__main__":
    main()
