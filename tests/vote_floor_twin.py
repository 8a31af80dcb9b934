"""Test helper for the vote floor (not a conftest, not collected): the definition of shz_set_vote_floor's two histograms in
plain Python, on the (sid, delta) matches that vote_tol_twin.matches_of yields."""
from collections import Counter

import numpy as np

from vote_tol_twin import matches_of, vote_tol

NB = 32


def bucket_of(c: int) -> int:
    """c <= 16 -> c - 1 (exact counts), else min(31, floor(log2 c) + 12)"""
    c = int(c)
    assert c >= 1
    return c - 1 if c <= 16 else min(31, (c.bit_length() - 1) + 12)


def bucket_lo(b: int) -> int:
    return b + 1 if b < 16 else (17 if b == 16 else 1 << (b - 12))


def floor_of(matches, tol: int):
    """(song_hist, bin_hist), [32] int64 each: bin_hist over the multiplicities c(s, d) of the single bins, whatever the
    tolerance; song_hist over every song's best count -- what vote_tol reports as its aligned at that tolerance."""
    matches = [(int(s), int(d)) for s, d in matches]
    song, bins = np.zeros(NB, np.int64), np.zeros(NB, np.int64)
    for c in Counter(matches).values():
        bins[bucket_of(c)] += 1
    n_songs = len({s for s, _ in matches})
    for _, _, aligned in vote_tol(matches, tol, max(n_songs, 1)):
        song[bucket_of(aligned)] += 1
    return song, bins


def expected_floor(tk, ts, to, qk, qo, qoff, tol: int):
    """Table.match(floor=True) at tolerance tol: (song_hist, bin_hist), [n_queries, 32] uint32 each."""
    rows = list(zip(tk.tolist(), ts.tolist(), to.tolist()))
    nq = len(qoff) - 1
    sh, bh = np.zeros((nq, NB), np.uint32), np.zeros((nq, NB), np.uint32)
    for q in range(nq):
        a, b = int(qoff[q]), int(qoff[q + 1])
        m, _, _ = matches_of(rows, zip(qk[a:b].tolist(), qo[a:b].tolist()))
        sh[q], bh[q] = floor_of(m, tol)
    return sh, bh
