"""Speed-tolerant recognition: audio played slightly fast or slow (csrc/shz_speed.hip).

The reference's hash is an exact (f1, f2, dt) triple (recognizer.py:100-114): a query that plays 1 % faster than the table's
copy has already lost the match.  Here the query's constellation peaks are extracted ONCE; for every factor of a ladder their
integer coordinates are mapped back to the table's domain (f' = round(f / s), t' = round(t s)), paired, hashed and matched
on the device, and the factor with the most aligned hashes wins.  A variant costs no FFT.

Limits: the hop is fixed, so a warped time is a rounded frame; a peak near the edge of its 21x21 neighbourhood may move when
the audio is stretched; pitch-preserving time-stretch is NOT covered (it needs independent factors for f and t)."""
from __future__ import annotations

from time import time

import numpy as np

from ._ffi import HOP, NFFT

S_ONE = 65536              # the factor 1.0 in Q16
S_MIN, S_MAX = 32768, 131072
# Twice the factor mismatch at which the right song's aligned count has fallen to half of its value at the true factor:
# 0.07 % measured on the CPU (oracle + tests/speed_twin.py, music-like corpus, true speeds 0.95 .. 1.05), so
# a true speed is never further than that half-width from a rung.  In Q16: round(0.0014 * 65536).
DEFAULT_STEP_Q16 = 92


def speed_ladder(lo: float = 0.95, hi: float = 1.05, step: float = None) -> np.ndarray:
    """The factors tried for a query of unknown speed, as Q16 (uint32, sorted, no duplicates): 65536 + k * step for every k
    that keeps the rung inside [lo, hi], and always 65536 itself.  step=None: the measured default, 92 / 65536 = 0.14 % --
    twice the half-width (0.07 %) of the tolerance curve in DESIGN.md 3.7c, at which the aligned count of the right song
    is half of what the true factor gives."""
    st = DEFAULT_STEP_Q16 if step is None else int(round(float(step) * S_ONE))
    if st < 1:
        raise ValueError("step must be at least 1 / 65536")
    lo16, hi16 = int(np.ceil(float(lo) * S_ONE)), int(np.floor(float(hi) * S_ONE))
    if lo16 < S_MIN or hi16 > S_MAX or lo16 > hi16:
        raise ValueError("speed_ladder: 0.5 <= lo <= hi <= 2.0")
    k_lo, k_hi = -((S_ONE - lo16) // st), (hi16 - S_ONE) // st      # ceil((lo16 - S_ONE) / st), floor((hi16 - S_ONE) / st)
    rungs = S_ONE + st * np.arange(k_lo, k_hi + 1, dtype=np.int64)
    return np.unique(np.concatenate([rungs, [S_ONE]])).astype(np.uint32)


def _check_speeds(speeds) -> np.ndarray:
    sp = np.ascontiguousarray(speeds)
    if sp.dtype.kind not in "iu":
        raise TypeError("speeds are Q16 integers (round(s * 65536)); see speed_ladder")
    return sp.astype(np.uint32)


def warp_hashes(peaks_f, peaks_t, peak_off, speeds, fan_value: int = 5, ctx=None, query_clip0=None):
    """The hashes of every clip at every factor (shz_warp_pair_hash): peaks in (time asc, freq asc) order per clip, peak_off
    their CSR, speeds in Q16.  Returns (key32, t1, hash_off): for query q, for speed v, for every clip c of q the hashes of
    (c, v); hash_off has n_clips * n_speeds + 1 entries in that order.  query_clip0=None: every clip is its own query, so
    segment c * n_speeds + v is clip c at speed v.  t1 is in the table's frames."""
    from . import get_context
    return (ctx or get_context()).warp_pair_hash(peaks_f, peaks_t, peak_off, _check_speeds(speeds), query_clip0, int(fan_value))


def recognize_speeds(queries, db, speeds=None, Fs: int = 44100, topn: int = 2, resample_to: int = None):
    """recognize_batch for queries of unknown speed.  Returns (results_per_query, timings) like recognize_batch; every
    result dict carries "speed" (the chosen factor as a float), OFFSET / OFFSET_SECS are in the TABLE's time, and timings
    carries "speeds" (the ladder, Q16), "speed_best" (index per query) and "speed_profile" ([n_queries, K]: the aligned count
    of the top answer of every factor).  speeds=None: speed_ladder().  The chosen factor is the one with the greatest
    aligned count; ties go to the factor nearest 1.0, then to the lower index."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, _as_pcm, _result_dicts, resample_to_device
    if not hasattr(db.table, "h"):
        raise NotImplementedError("fused recognition takes the unsharded table (shards=1)")
    sp = speed_ladder() if speeds is None else _check_speeds(speeds)
    ctx = db.ctx
    if getattr(ctx, "hop", HOP) != HOP:
        ctx.set_overlap(NFFT - HOP)
    db.finalize()
    chans, first = [], [0]
    for q in queries:
        cs = [q] if (isinstance(q, np.ndarray) and q.ndim == 1) else list(q)
        chans.extend(cs)
        first.append(len(chans))
    first = np.asarray(first, np.uint32)
    kw = dict(amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, topn=int(topn))
    if resample_to is not None and int(resample_to) != int(Fs):   # resampled on the device and handed on there
        buf, off = resample_to_device(chans, int(Fs), int(resample_to), ctx)
        try:
            res, ms = ctx.recognize_speeds(db.table, buf, off, first, sp, fs=int(resample_to), pcm_device=True, **kw)
        finally:
            buf.free()
    else:
        arrs = [_as_pcm(c) for c in chans]
        off = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            off[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)
        res, ms = ctx.recognize_speeds(db.table, pcm, off, first, sp, fs=int(Fs), **kw)
    t0 = time()
    results = []
    for q in range(len(queries)):
        dicts = _result_dicts(db, res, q, int(res["nhash"][q]))
        for d in dicts:
            d["speed"] = float(sp[int(res["best"][q])]) / S_ONE
        results.append(dicts)
    align_time = time() - t0
    return results, {"fingerprint_time": ms[0] * 1e-3, "warp_time": ms[1] * 1e-3, "query_time": ms[2] * 1e-3,
                     "align_time": align_time, "n_hashes": res["nhash"], "speeds": sp, "speed_best": res["best"],
                     "speed_profile": res["profile"]}
