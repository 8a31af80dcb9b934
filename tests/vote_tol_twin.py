"""Test helper for the tolerant vote (not a conftest, not collected): the definition of shz_set_vote_tolerance in plain
Python, on the (sid, delta) matches that oracle.cpu_ref.vote takes."""
from collections import Counter


def vote_tol(matches, tol: int, topn: int = 2):
    """[(sid, delta, aligned)] of the top songs.  c[sid][d] = votes per song and offset difference, S(sid, d) = the sum of
    c[sid][d .. d + tol].  Per song: the windows that start at an occupied d, the first maximum of S in ascending d wins;
    aligned = that S, delta = the bin inside the window with the largest count of its own (ties: the smaller delta).
    Songs by aligned descending, ties to the smaller song id.  tol = 0 is oracle.cpu_ref.vote."""
    tol = int(tol)
    assert 0 <= tol <= 31
    c = {}
    for sid, d in matches:
        c.setdefault(int(sid), Counter())[int(d)] += 1
    songs = []
    for sid in sorted(c):
        bins = c[sid]
        best = None
        for d in sorted(bins):
            s = sum(bins.get(e, 0) for e in range(d, d + tol + 1))
            if best is None or s > best[0]:
                best = (s, d)
        s, d0 = best
        delta = max(range(d0, d0 + tol + 1), key=lambda e: (bins.get(e, 0), -e))
        songs.append((sid, delta, s))
    songs.sort(key=lambda x: (-x[2], x[0]))
    return songs[:topn]


def matches_of(rows, hashes):
    """return_matches on plain lists: rows = (key, sid, off) of the table, hashes = (key, q_off) of one query, both taken as
    sets.  Returns (matches [(sid, db_off - q_off)], dedup {sid: rows whose key is queried}, distinct hashes)."""
    by_key = {}
    for k, s, o in sorted(set((int(k), int(s), int(o)) for k, s, o in rows)):
        by_key.setdefault(k, []).append((s, o))
    hs = sorted(set((int(k), int(q)) for k, q in hashes))
    matches, dedup, seen = [], {}, set()
    for k, q in hs:
        for s, o in by_key.get(k, ()):
            matches.append((s, o - q))
            if k not in seen:
                dedup[s] = dedup.get(s, 0) + 1
        seen.add(k)
    return matches, dedup, len(hs)


def expected_match(tk, ts, to, qk, qo, qoff, tol: int, topn: int):
    """Table.match at tolerance tol, per query: ([(sid, delta, aligned, dedup)] ranked, npairs, nhash)."""
    rows = list(zip(tk.tolist(), ts.tolist(), to.tolist()))
    out = []
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        m, dedup, nhash = matches_of(rows, zip(qk[a:b].tolist(), qo[a:b].tolist()))
        out.append(([(s, d, c, dedup[s]) for s, d, c in vote_tol(m, tol, topn)], len(m), nhash))
    return out


def assert_match(res, want, what=""):
    """the arrays of Table.match against expected_match's lists: every counter, every ranked row, zeros behind them"""
    for q, (ranked, npairs, nhash) in enumerate(want):
        assert int(res["npairs"][q]) == npairs and int(res["nhash"][q]) == nhash, (what, q)
        got = [(int(res["sid"][q, i]), int(res["delta"][q, i]), int(res["aligned"][q, i]), int(res["dedup"][q, i]))
               for i in range(int(res["nres"][q]))]
        assert got == ranked, (what, q, got[:3], ranked[:3])
        for name in ("sid", "delta", "aligned", "dedup"):
            assert not res[name][q, len(ranked):].any(), (what, q, name)
