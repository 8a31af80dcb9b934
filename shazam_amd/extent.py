"""Match extents (csrc/shz_extent.hip): where in the query and in the song the aligned hashes lie.

A match answers (song, delta, aligned): delta says how the two timelines are shifted, not over which stretch they agree.
Table.match_extents runs a second, cheaper pass over the same (query hash, table row) pairs for candidates (song, d_lo, d_hi)
and returns, per candidate, the number of pairs that belong, the first and last query frame and song frame among them and a
64-bucket histogram of the pairs over the query's time.  extents_of() makes the candidates from a match result;
dense_span() turns a histogram into the stretch that is robust against single chance pairs.

With fit=True the pass also returns four integer moments of every candidate's pairs: line_fit() turns them into
the least-squares line of the offset difference over the query's time, tempo_of() its slope into the tempo a warped query really
runs at, own_frames() a range of warped frames into the query's own."""
from __future__ import annotations

import numpy as np

# Pairs a bucket must hold to count as part of the matched stretch.  q_first / q_last move with ONE chance pair far away from
# the true stretch; a bucket of dense_span needs DENSE_MIN_COUNT.  Set between the distributions scripts/extent_bench.py measured
# on an MI355X (profiles/extent_bench.json): 20,000 music-like synthetic songs of 10 s, 200 queries of 10 s that
# hold 4 s of their song between two stretches of noise, buckets of 4 frames.  Chance: the true song's own pairs OUTSIDE the
# planted stretch occupied 4 buckets in 200 queries, with 1 to 3 pairs each; an unrelated song tested at the true song's delta
# (1,000 candidates) occupied 138 buckets, median 1 pair, 90 % at most 3, the largest 11.  True: inside the stretch a bucket
# holds 47 pairs at the median and 8 at the 10th percentile (one in a hundred holds none: quiet frames).  4 lies above every
# stray bucket of the true song seen and below nine tenths of its true buckets; at 2 the span of 2 of the 200 true songs left
# the stretch by a bucket or more.  It does NOT tell songs apart: an unrelated runner-up of the match, taken at ITS OWN best
# delta, puts its few pairs into one bucket (median 14, up to 45) -- a dense bucket says where a candidate's pairs lie, the
# aligned count says whether the candidate is right.  Not measured: noisy or re-encoded queries, tracks of minutes (wider
# buckets collect more chance pairs).
DENSE_MIN_COUNT = 4


def extents_of(table, key32, q_off, query_off, res, tol: int = 0, hist: bool = True) -> dict:
    """Table.match_extents for the results of a Table.match on the same hashes: candidate i of query q is (res["sid"][q, i],
    res["delta"][q, i] - tol, res["delta"][q, i] + tol), cand_n = res["nres"].  With tol = 0 (a match at tolerance 0) the
    returned count equals res["aligned"], entry for entry.  With tol > 0 the range is a SUPERSET of the winning window of a
    tolerant vote: the reported delta is the window's strongest bin, not its start, so the window [d0, d0 + tol] lies inside
    [delta - tol, delta + tol] wherever it begins, and count >= aligned."""
    tol = int(tol)
    if tol < 0:
        raise ValueError("tol must be >= 0")
    sid = np.ascontiguousarray(res["sid"], np.uint32)
    delta = np.asarray(res["delta"], np.int64)
    return table.match_extents(key32, q_off, query_off, sid, (delta - tol).astype(np.int32), (delta + tol).astype(np.int32),
                               cand_n=np.minimum(np.asarray(res["nres"], np.uint32), sid.shape[1]), hist=hist)


FIT_MAX_WIDTH = 4096      # bins a candidate may span with the moments (EX_FIT_MAX_WIDTH): q u < 2^32, no sum but sum_qq wraps
FIT_MAX_COUNT = 1 << 24   # pairs from which sum_qq (q < 2^20) may have wrapped: no fit is reported there


def line_fit(count, sum_q, sum_u, sum_qq, sum_qu, d_lo):
    """The least-squares line d = slope * q + intercept through a candidate's pairs, from its moments (Table.match_extents(...,
    fit=True), Context.recognize_warps(..., extents=True)): q = q_off, u = d - d_lo, so
        slope = (n sum_qu - sum_q sum_u) / (n sum_qq - sum_q^2)        intercept = d_lo + (sum_u - slope sum_q) / n
    in exact Python integers, returned as (slope, intercept), two fractions.Fraction.  None with fewer than 2 pairs, where
    all pairs share one q (the denominator is 0), and from 2^24 pairs on (sum_qq may have wrapped).  Every pair weighs the
    same: chance pairs inside the candidate's range pull the line."""
    from fractions import Fraction
    n, sq, su, sqq, squ = int(count), int(sum_q), int(sum_u), int(sum_qq), int(sum_qu)
    if n < 2 or n >= FIT_MAX_COUNT:
        return None
    den = n * sqq - sq * sq
    if den == 0:
        return None
    slope = Fraction(n * squ - sq * su, den)
    return slope, int(d_lo) + (su - slope * sq) / n


def tempo_of(t16, slope):
    """The tempo a query really runs at, given the time factor t16 (Q16) its hashes were warped with and the slope of
    line_fit on them: t16 / 65536 * (1 + slope).  With t' = t t16 / 65536 the warped time of query frame t and a true tempo
    a, the song plays at t a = t' a 65536 / t16, so d = off - t' = t' (a 65536 / t16 - 1) + c: the slope is a / rung - 1."""
    from fractions import Fraction
    return Fraction(int(t16), 65536) * (1 + slope)


def own_frames(first, last, t16):
    """The query's OWN frames [t_first, t_last] whose warped frames map(t) = (t t16 + 32768) >> 16 lie in [first, last]:
    the smallest t with map(t) >= first and the largest t with map(t) <= last.  map(t) >= first means t t16 >= (first << 16)
    - 32768, map(t) <= last means t t16 + 32768 < (last + 1) << 16."""
    first, last, t16 = int(first), int(last), int(t16)
    lo = max(0, -((32768 - (first << 16)) // t16))            # ceil(((first << 16) - 32768) / t16)
    hi = (((last + 1) << 16) - 32769) // t16
    return lo, hi


def dense_span(hist, shift: int, min_count: int = DENSE_MIN_COUNT):
    """[start_frame, end_frame) of the query covered by the first .. last bucket of hist (64 counts, bucket b = the frames
    [b << shift, (b + 1) << shift)) that holds at least min_count pairs; None where no bucket does.  One chance pair far
    away moves q_first / q_last but not this."""
    h = np.asarray(hist).reshape(-1)
    if len(h) != 64:
        raise ValueError("hist has 64 buckets")
    at = np.flatnonzero(h >= int(min_count))
    if len(at) == 0:
        return None
    return int(at[0]) << int(shift), (int(at[-1]) + 1) << int(shift)
