"""Test helper for the song filter (not a conftest, not collected): the definition of shz_set_song_filter in plain Python --
a filtered match on a table gives the arrays that the plain match gives on a table holding only the allowed songs' rows."""
import numpy as np

from vote_floor_twin import NB, expected_floor
from vote_tol_twin import expected_match


def allowed_rows(ts, ids, exclude):
    """mask of the table rows whose song passes the set: listed != exclude"""
    listed = np.isin(np.asarray(ts, np.uint32), np.asarray(sorted({int(i) for i in ids}), np.uint32))
    return listed != bool(exclude)


def _sets_of(sets, set_of, nq):
    sets = [list(s) for s in sets]
    set_of = [0] * nq if set_of is None else [int(i) for i in set_of]
    assert len(set_of) == nq and all(0 <= i < len(sets) for i in set_of)
    return sets, set_of


def _one_query(qk, qo, qoff, q):
    a, b = int(qoff[q]), int(qoff[q + 1])
    return qk[a:b], qo[a:b], np.array([0, b - a], np.uint64)


def expected_match_sets(tk, ts, to, qk, qo, qoff, tol, topn, sets, set_of=None, exclude=False):
    """Table.match under a song filter, per query: ([(sid, delta, aligned, dedup)] ranked, npairs, nhash) --
    vote_tol_twin.expected_match on the table rows whose song passes the query's set; nhash comes from the query alone."""
    nq = len(qoff) - 1
    sets, set_of = _sets_of(sets, set_of, nq)
    masks = [allowed_rows(ts, s, exclude) for s in sets]
    out = []
    for q in range(nq):
        m = masks[set_of[q]]
        out.extend(expected_match(tk[m], ts[m], to[m], *_one_query(qk, qo, qoff, q), tol, topn))
    return out


def expected_floor_sets(tk, ts, to, qk, qo, qoff, tol, sets, set_of=None, exclude=False):
    """Table.match(floor=True) under a song filter: (song_hist, bin_hist), [n_queries, 32] uint32 each, of the kept votes."""
    nq = len(qoff) - 1
    sets, set_of = _sets_of(sets, set_of, nq)
    masks = [allowed_rows(ts, s, exclude) for s in sets]
    sh, bh = np.zeros((nq, NB), np.uint32), np.zeros((nq, NB), np.uint32)
    for q in range(nq):
        m = masks[set_of[q]]
        a, b = expected_floor(tk[m], ts[m], to[m], *_one_query(qk, qo, qoff, q), tol)
        sh[q], bh[q] = a[0], b[0]
    return sh, bh
