"""The key cap: which keys of a table vote.

A key that thousands of songs share votes for all of them and identifies none; it costs its votes' expand, sort and fold all
the same.  ``Table.key_hist()`` says how many rows the keys of a table hold -- ``keys[b]`` distinct keys and ``rows[b]`` rows
in bucket b of ``shazam_amd.floor.bucket_of`` (1 .. 16 rows exact, then powers of two) -- and ``Context.key_cap`` /
``max_key_rows=`` leave the keys above a bound out of a match, at the probe.  This module is the arithmetic between the two.
A histogram knows a key's size only up to its bucket, so everything here is exact at bucket edges (``bucket_hi``) and says
so elsewhere; the arithmetic is in integers and ``Fraction``, never a float comparison.
"""
from fractions import Fraction

import numpy as np

from .floor import NBUCKETS, bucket_lo, bucket_of


CAP_MAX = (1 << 64) - 1      # the largest cap (shz_set_key_cap takes 64 bits): no key exceeds it


def bucket_hi(b: int) -> int:
    """The largest count of a bucket; the last one is open above: CAP_MAX."""
    b = int(b)
    if not 0 <= b < NBUCKETS:
        raise ValueError(f"bucket {b}")
    return CAP_MAX if b == NBUCKETS - 1 else bucket_lo(b + 1) - 1


def _rows(hist):
    r = np.asarray(hist["rows"] if isinstance(hist, dict) else hist)
    if r.shape != (NBUCKETS,):
        raise ValueError(f"a key histogram has {NBUCKETS} buckets, got shape {r.shape}")
    return [int(x) for x in r]


def rows_kept(hist, cap: int) -> int:
    """The table rows that stay under the cap (0: off, all of them): the rows of the buckets that lie wholly at or below it.
    Exact where the cap is a bucket's upper edge (every cap up to 16, then 31, 63, ...) or at least hist["max_rows"]; between
    two edges it is the lower bound that the histogram can vouch for -- the keys of the cap's own bucket are not counted."""
    rows = _rows(hist)
    cap = int(cap)
    if cap < 0:
        raise ValueError(f"cap {cap}")
    if cap == 0 or (isinstance(hist, dict) and "max_rows" in hist and cap >= int(hist["max_rows"])):
        return sum(rows)
    return sum(rows[b] for b in range(NBUCKETS) if bucket_hi(b) <= cap)


def cap_for(hist, keep) -> int:
    """The smallest bucket upper edge c such that the keys of at most c rows hold at least `keep` of all rows: the cap that
    drops the largest keys and no more than 1 - keep of the table.  keep: a Fraction, or a float converted once (0.95 is taken
    as the binary fraction it is).  keep = 1 gives the edge of the largest occupied bucket -- nothing is dropped --, keep = 0
    the smallest cap, 1.  Where only the last, open bucket can reach `keep`, the cap is hist["max_rows"] (a plain list of
    rows knows no maximum: CAP_MAX).  An empty histogram gives 0, the cap that is off."""
    rows = _rows(hist)
    keep = keep if isinstance(keep, Fraction) else Fraction(keep)
    if not 0 <= keep <= 1:
        raise ValueError(f"keep {keep} is not in [0, 1]")
    total = sum(rows)
    if total == 0:
        return 0
    kept = 0
    for b in range(NBUCKETS - 1):
        kept += rows[b]
        if kept >= keep * total:          # Fraction against int: exact
            return bucket_hi(b)
    return int(hist["max_rows"]) if isinstance(hist, dict) and "max_rows" in hist else CAP_MAX


def share_kept(hist, cap: int) -> Fraction:
    """rows_kept as a share of all rows (1 for an empty table)."""
    total = sum(_rows(hist))
    return Fraction(rows_kept(hist, cap), total) if total else Fraction(1)


__all__ = ["CAP_MAX", "bucket_hi", "rows_kept", "cap_for", "share_kept", "bucket_of", "bucket_lo"]
