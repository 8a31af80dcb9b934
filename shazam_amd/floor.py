"""The vote floor: how far above chance a match stands.

With the floor on (``Context.floor()``, ``Table.match(..., floor=True)``) the library returns two EXACT integer histograms
per query: ``song_hist[b]`` -- the songs with any vote whose best count (their ``aligned``) falls into bucket b -- and
``bin_hist[b]`` -- the single (song, offset difference) bins whose count falls into bucket b.  The buckets (32): a count
c <= 16 has bucket c - 1, a larger one min(31, floor(log2 c) + 12); ``bucket_of`` / ``bucket_lo`` restate shz_vote_bucket.

What this module adds on the host is an ESTIMATOR, and a heuristic one: it assumes that the counts chance reaches fall off
geometrically, fits that tail to the exact buckets (counts 1 .. 16) and extrapolates it to the count in question.  The
histograms are the exact part; the score is a model of them.  A true match of 16 aligned hashes or fewer lies inside the
fitted range and is indistinguishable from chance by construction.  Measured on synthetic audio only:
there, at 1,000 and 4,000 songs, the score on the BIN histogram (which="bins") separated queries whose song is in the table
from queries whose song is not, and the default, the SONG histogram, did not -- a song's best count is a maximum over its
bins, and the histogram of maxima is peaked rather than falling when every song has a vote.
"""
import math

import numpy as np

NBUCKETS = 32
EXACT = 16          # buckets 0 .. 15 hold the exact counts 1 .. 16


def bucket_of(count: int) -> int:
    """The bucket of a count >= 1 (shz_vote_bucket)."""
    c = int(count)
    if c < 1:
        raise ValueError(f"count {count}: a bucket holds counts >= 1")
    if c <= EXACT:
        return c - 1
    return min(NBUCKETS - 1, (c.bit_length() - 1) + 12)


def bucket_lo(bucket: int) -> int:
    """The smallest count of a bucket: the inverse of bucket_of."""
    b = int(bucket)
    if not 0 <= b < NBUCKETS:
        raise ValueError(f"bucket {bucket}")
    if b < EXACT:
        return b + 1
    return 17 if b == EXACT else 1 << (b - 12)


def _row(hist):
    h = np.asarray(hist)
    if h.shape != (NBUCKETS,):
        raise ValueError(f"a histogram row has {NBUCKETS} buckets, got shape {h.shape}")
    return h


def tail_counts(hist):
    """tail[b] = the entries of hist in bucket b or above (int64, [32]): how many songs (bins) reached bucket_lo(b)."""
    h = _row(hist).astype(np.int64)
    return np.cumsum(h[::-1])[::-1]


def fit_tail(hist):
    """(alpha, beta) of the least-squares line ln n_c = alpha + beta c over the exact buckets (c = 1 .. 16) with n_c > 0,
    weighted by n_c, in float64 and in ascending c (a fixed summation order); None with fewer than two such buckets or with
    beta >= 0 (no falling tail to extrapolate).  A heuristic: see the module's docstring."""
    h = _row(hist)
    pts = [(float(c), float(h[c - 1])) for c in range(1, EXACT + 1) if int(h[c - 1]) > 0]
    if len(pts) < 2:
        return None
    sw = sx = sy = 0.0
    for c, n in pts:
        sw += n
        sx += n * c
        sy += n * math.log(n)
    mx, my = sx / sw, sy / sw
    sxx = sxy = 0.0
    for c, n in pts:
        sxx += n * (c - mx) * (c - mx)
        sxy += n * (c - mx) * (math.log(n) - my)
    if sxx <= 0.0:
        return None
    beta = sxy / sxx
    if not beta < 0.0:
        return None
    return my - beta * mx, beta


def expected_above(hist, count):
    """The entries the fitted tail expects at `count` or above: sum over c >= count of exp(alpha + beta c) =
    exp(alpha + beta count) / (1 - exp(beta)); None where fit_tail gives None."""
    f = fit_tail(hist)
    if f is None:
        return None
    alpha, beta = f
    return math.exp(alpha + beta * float(count)) / (1.0 - math.exp(beta))


def score(aligned, hist=None, which="songs", song_hist=None, bin_hist=None):
    """-log10 of the songs (which="songs", the default) or single bins (which="bins") that chance is expected to put at
    `aligned` or above for this query: 3 means one in a thousand.  hist: the row to use; or give song_hist / bin_hist and
    let `which` select.  None where nothing can be fitted (fit_tail) or aligned is 0.  A heuristic (module docstring)."""
    if which not in ("songs", "bins"):
        raise ValueError(f"which must be 'songs' or 'bins', got {which!r}")
    if hist is None:
        hist = song_hist if which == "songs" else bin_hist
    if hist is None:
        raise ValueError("score: no histogram given")
    if int(aligned) < 1:
        return None
    e = expected_above(hist, aligned)
    if e is None:
        return None
    return -math.log10(e) if e > 0.0 else math.inf


def floor_entry(song_hist, bin_hist, aligned, which="songs"):
    """The "floor" entry of a recognise result: the two rows, and expected_above / score of the query's best `aligned`."""
    hist = song_hist if which == "songs" else bin_hist
    a = int(aligned)
    return {"song_hist": np.asarray(song_hist, np.uint32).copy(), "bin_hist": np.asarray(bin_hist, np.uint32).copy(),
            "expected_above": expected_above(hist, a) if a >= 1 else None, "score": score(a, hist)}


def keep_windows(nres, aligned, song_hist, min_score, which="songs"):
    """scan(min_score=...): a copy of nres with the windows cleared whose best result scores below min_score.  aligned:
    [n_windows, topn] (column 0 is the best); song_hist: [n_windows, 32] (the rows `which` selects).  A window whose score is
    None -- nothing to compare against -- counts: min_aligned alone decides there."""
    out = np.array(nres, copy=True)
    for w in range(len(out)):
        if out[w] == 0:
            continue
        s = score(int(aligned[w, 0]), song_hist[w], which=which)
        if s is not None and s < min_score:
            out[w] = 0
    return out
