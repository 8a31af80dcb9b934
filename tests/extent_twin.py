"""Test helper for the match extents (not a conftest, not collected): the definition of shz_match_extents in plain Python,
on plain lists.  Imports nothing from the library."""


def shift_of(q_offs) -> int:
    """the smallest s >= 0 with (largest q_off >> s) < 64; 0 for an empty query"""
    top = max((int(o) for o in q_offs), default=0)
    s = 0
    while (top >> s) >= 64:
        s += 1
    return s


def extents(rows, hashes, cands):
    """rows = (key, sid, off) of the table, hashes = (key, q_off) of ONE query, both taken as sets; cands = [(sid, d_lo, d_hi)],
    d_lo <= d_hi, signed and inclusive.  A pair is a (hash, row) of equal key, d = off - q_off; it belongs to every candidate
    with row.sid == sid and d_lo <= d <= d_hi.  Returns (per candidate a dict count, q_first, q_last, t_first, t_last,
    hist[64]; shift): hist[b] = pairs that belong with q_off >> shift == b; everything 0 where count == 0."""
    by_key = {}
    for k, s, o in set((int(k), int(s), int(o)) for k, s, o in rows):
        by_key.setdefault(k, []).append((s, o))
    hs = sorted(set((int(k), int(q)) for k, q in hashes))
    shift = shift_of(q for _, q in hs)
    out = []
    for sid, d_lo, d_hi in cands:
        sid, d_lo, d_hi = int(sid), int(d_lo), int(d_hi)
        assert d_lo <= d_hi
        qs, ts, hist = [], [], [0] * 64
        for k, q in hs:
            for s, o in by_key.get(k, ()):
                if s == sid and d_lo <= o - q <= d_hi:
                    qs.append(q)
                    ts.append(o)
                    hist[q >> shift] += 1
        if qs:
            out.append({"count": len(qs), "q_first": min(qs), "q_last": max(qs), "t_first": min(ts), "t_last": max(ts), "hist": hist})
        else:
            out.append({"count": 0, "q_first": 0, "q_last": 0, "t_first": 0, "t_last": 0, "hist": hist})
    return out, shift


SCALARS = ("count", "q_first", "q_last", "t_first", "t_last")


def expected_extents(tk, ts, to, qk, qo, qoff, cand_sid, d_lo, d_hi, cand_n=None):
    """Table.match_extents as nested lists: per query (list of candidate dicts over ALL ncand slots -- zeros at and past
    cand_n[q] --, shift)."""
    rows = list(zip(tk.tolist(), ts.tolist(), to.tolist()))
    nq = len(qoff) - 1
    ncand = len(cand_sid[0]) if nq else 0
    out = []
    for q in range(nq):
        a, b = int(qoff[q]), int(qoff[q + 1])
        n = ncand if cand_n is None else int(cand_n[q])
        cands = [(cand_sid[q][c], d_lo[q][c], d_hi[q][c]) for c in range(n)]
        got, shift = extents(rows, zip(qk[a:b].tolist(), qo[a:b].tolist()), cands)
        got += [{"count": 0, "q_first": 0, "q_last": 0, "t_first": 0, "t_last": 0, "hist": [0] * 64} for _ in range(ncand - n)]
        out.append((got, shift))
    return out


def assert_extents(res, want, what="", hist=True):
    """the arrays of Table.match_extents against expected_extents' lists: exact, the zeros past cand_n included"""
    assert len(res["shift"]) == len(want), what
    for q, (cands, shift) in enumerate(want):
        assert int(res["shift"][q]) == shift, (what, q, int(res["shift"][q]), shift)
        for c, w in enumerate(cands):
            got = {k: int(res[k][q, c]) for k in SCALARS}
            assert got == {k: w[k] for k in SCALARS}, (what, q, c, got, {k: w[k] for k in SCALARS})
            if hist:
                assert res["hist"][q, c].tolist() == w["hist"], (what, q, c)
