"""Test helpers for altered content shared between recordings (not a conftest, not collected): the two-recording fixture of
DESIGN.md 3.7r -- a piece sped up 1.03, a piece unchanged, a piece rendered at tempo 1.04 and pitch 0.97, between stretches of
noise --, the warps it is asked at, and the whole answer in plain Python (shared_warp_twin.cells, repeat_twin.fold), which the
host tests assert and the GPU tests compare with."""
import numpy as np

import repeat_twin
import shared_warp_twin as twin
from oracle import cpu_ref as O
from oracle import synth
from speed_twin import speed_up
from warp_twin import notes_clip

SR, HOP = 44100, 2048
q16 = lambda x: int(round(x * 65536))                                            # noqa: E731
# the jobs of the table in DESIGN.md 3.7r, plain first
WARPS = [(1.0, 1.0), (1.03, 1.03), (1.04, 0.97), (1.02, 1.02), (1.04, 1.04), (0.97, 0.97), (1.03, 0.97), (1.04, 1.0)]
T16 = [q16(t) for t, _ in WARPS]
F16 = [q16(f) for _, f in WARPS]
DEFAULTS = dict(max_run=64, cell_shift=5, min_cell_pairs=8)
FOLD = dict(lag_tol=1, max_gap=1, min_pairs=100)
T_MAX = (1 << 20) - 1
X_START, X_SECONDS = 2.0, 8.0 / 1.03                                             # where X lies in recording 1, sped up


def recordings():
    """[rec0, rec1]: rec0 the plain side (b of the jobs), rec1 the altered one (a)"""
    N = lambda s, c, sec: synth.traffic_noise(s, c, int(sec * SR))              # noqa: E731
    X, Y, Z = notes_clip(21, 0, 8.0), notes_clip(21, 1, 6.0), notes_clip(21, 2, 8.0)
    Zw = notes_clip(21, 2, 8.0 / 1.04, tempo=1.04, pitch=0.97)
    rec0 = np.concatenate([N(5, 0, 3), X, N(5, 1, 2), Y, N(5, 2, 1), Z, N(5, 3, 1)])
    rec1 = np.concatenate([N(6, 0, 2), speed_up(X, 1.03), N(6, 1, 3), Y, N(6, 2, 2), Zw, N(6, 3, 1)])
    return [rec0.astype(np.int16), rec1.astype(np.int16)]


def self_recording():
    """one recording that holds X and, later, X sped up 1.03"""
    N = lambda c, sec: synth.traffic_noise(7, c, int(sec * SR))                 # noqa: E731
    X = notes_clip(21, 0, 8.0)
    return np.concatenate([N(0, 2), X, N(1, 3), speed_up(X, 1.03), N(2, 1)]).astype(np.int16)


def oracle_peaks(recs):
    """(peak_f, peak_t, peak_off) of mono recordings, by the reference"""
    fs, ts, po = [], [], [0]
    for x in recs:
        _, _, f, t = O.fingerprint_keys(x)
        fs.append(np.asarray(f, np.int64))
        ts.append(np.asarray(t, np.int64))
        po.append(po[-1] + len(f))
    return np.concatenate(fs), np.concatenate(ts), po


def twin_cells(peak_f, peak_t, peak_off, jobs, t16=T16, f16=F16, rec_clip0=None, **kw):
    rec_clip0 = list(range(len(peak_off))) if rec_clip0 is None else rec_clip0
    return twin.cells(peak_f, peak_t, peak_off, rec_clip0, t16, f16, jobs, **dict(DEFAULTS, **kw))


def twin_fold(cells, **kw):
    """repeat_twin.fold on the twin's cells (signed lags: the fold only compares them), the jobs standing in for recordings"""
    return repeat_twin.fold(cells["cell_off"], cells["lag"], cells["block"], cells["pairs"], cells["first"], cells["last"],
                            **dict(FOLD, **kw))


def stretch_cells(cells, rep):
    """(lag, first, last, pairs) of the job's cells inside the stretch's rectangle"""
    j = rep["rec"]
    return [(cells["lag"][i], cells["first"][i], cells["last"][i], cells["pairs"][i])
            for i in range(cells["cell_off"][j], cells["cell_off"][j + 1])
            if rep["lag_lo"] <= cells["lag"][i] <= rep["lag_hi"] and cells["first"][i] >= rep["first"] and cells["last"][i] <= rep["last"]]


def table_jobs(a=1, b=0, n=len(WARPS)):
    """job v = (a, b, warp v) with the widest window"""
    return [(a, b, v, -T_MAX, T_MAX) for v in range(n)]
