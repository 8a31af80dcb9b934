"""Test helper for the key cap (not a conftest, not collected): the definition of shz_set_key_cap in plain Python -- with cap
c >= 1 a match gives the arrays that the plain match gives on a table lacking every row whose key holds more than c rows; the
rows counted are the distinct (key, song, offset) rows of the whole table; cap 0 is off."""
import numpy as np

from extent_twin import expected_extents
from song_filter_twin import expected_floor_sets, expected_match_sets
from vote_floor_twin import expected_floor
from vote_tol_twin import expected_match


def key_sizes(tk, ts, to):
    """{key: distinct rows}"""
    rows = set(zip(np.asarray(tk).tolist(), np.asarray(ts).tolist(), np.asarray(to).tolist()))
    n = {}
    for k, _, _ in rows:
        n[k] = n.get(k, 0) + 1
    return n


def kept_rows(tk, cap, ts=None, to=None):
    """mask of the table rows that stay: those whose key holds at most cap rows (cap 0: all).  tk alone: its entries are
    taken as distinct rows; with ts and to, duplicate (key, song, offset) rows count once."""
    tk = np.asarray(tk, np.uint32)
    cap = int(cap)
    if cap == 0:
        return np.ones(len(tk), bool)
    if ts is None:
        keys, counts = np.unique(tk, return_counts=True)
        n = dict(zip(keys.tolist(), counts.tolist()))
    else:
        n = key_sizes(tk, ts, to)
    return np.asarray([n[k] <= cap for k in tk.tolist()], bool).reshape(len(tk))


def masked(tk, ts, to, cap):
    m = kept_rows(tk, cap, ts, to)
    return tk[m], ts[m], to[m]


def expected_match_cap(tk, ts, to, qk, qo, qoff, tol, topn, cap):
    """Table.match(max_key_rows=cap), per query: ([(sid, delta, aligned, dedup)] ranked, npairs, nhash); nhash comes from the
    query alone."""
    return expected_match(*masked(tk, ts, to, cap), qk, qo, qoff, tol, topn)


def expected_floor_cap(tk, ts, to, qk, qo, qoff, tol, cap):
    """... (floor=True): (song_hist, bin_hist) of the kept votes"""
    return expected_floor(*masked(tk, ts, to, cap), qk, qo, qoff, tol)


def expected_match_cap_sets(tk, ts, to, qk, qo, qoff, tol, topn, cap, sets, set_of=None, exclude=False):
    """the cap with a song filter on top: both masks"""
    return expected_match_sets(*masked(tk, ts, to, cap), qk, qo, qoff, tol, topn, sets, set_of, exclude)


def expected_floor_cap_sets(tk, ts, to, qk, qo, qoff, tol, cap, sets, set_of=None, exclude=False):
    return expected_floor_sets(*masked(tk, ts, to, cap), qk, qo, qoff, tol, sets, set_of, exclude)


def expected_extents_cap(tk, ts, to, qk, qo, qoff, cand_sid, d_lo, d_hi, cap, cand_n=None):
    """Table.match_extents inside ctx.key_cap(cap): extent_twin on the masked table"""
    return expected_extents(*masked(tk, ts, to, cap), qk, qo, qoff, cand_sid, d_lo, d_hi, cand_n)


def dropped(tk, ts, to, qk, qo, qoff, cap):
    """(groups, pairs) the cap drops over all queries: a group is a distinct (query, key) whose key holds more than cap rows
    (a key without rows is none), its pairs are the key's rows x the query's distinct offsets under that key"""
    if int(cap) == 0:
        return 0, 0
    n = key_sizes(tk, ts, to)
    groups = pairs = 0
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        offs = {}
        for k, o in set(zip(np.asarray(qk[a:b]).tolist(), np.asarray(qo[a:b]).tolist())):
            offs[k] = offs.get(k, 0) + 1
        for k, e in offs.items():
            if n.get(k, 0) > int(cap):
                groups += 1
                pairs += n[k] * e
    return groups, pairs
