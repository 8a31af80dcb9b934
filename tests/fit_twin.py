"""Test helper for the moments of the match extents (not a conftest, not collected): the definition of the four sums of
shz_match_extents_fit in plain Python on top of tests/extent_twin.py, and the query's own frames of a warped range.  Imports
nothing from the library."""
from extent_twin import expected_extents

SUMS = ("sum_q", "sum_u", "sum_qq", "sum_qu")
M64 = (1 << 64) - 1


def moments(rows, hashes, cands):
    """rows = (key, sid, off) of the table, hashes = (key, q_off) of ONE query, both taken as sets; cands = [(sid, d_lo, d_hi)].
    Per candidate and every pair that belongs (extent_twin.extents' rule) q = q_off and u = (off - q_off) - d_lo: a dict
    sum_q, sum_u, sum_qq, sum_qu, each modulo 2^64; all 0 where nothing belongs."""
    by_key = {}
    for k, s, o in set((int(k), int(s), int(o)) for k, s, o in rows):
        by_key.setdefault(k, []).append((s, o))
    hs = sorted(set((int(k), int(q)) for k, q in hashes))
    out = []
    for sid, d_lo, d_hi in cands:
        sid, d_lo, d_hi = int(sid), int(d_lo), int(d_hi)
        m = dict.fromkeys(SUMS, 0)
        for k, q in hs:
            for s, o in by_key.get(k, ()):
                if s == sid and d_lo <= o - q <= d_hi:
                    u = o - q - d_lo
                    m["sum_q"] += q
                    m["sum_u"] += u
                    m["sum_qq"] += q * q
                    m["sum_qu"] += q * u
        out.append({f: v & M64 for f, v in m.items()})
    return out


def expected_moments(tk, ts, to, qk, qo, qoff, cand_sid, d_lo, d_hi, cand_n=None):
    """Table.match_extents(..., fit=True)'s sums as nested lists: per query a list of dicts over ALL ncand slots, zeros at
    and past cand_n[q]."""
    rows = list(zip(tk.tolist(), ts.tolist(), to.tolist()))
    nq = len(qoff) - 1
    ncand = len(cand_sid[0]) if nq else 0
    out = []
    for q in range(nq):
        a, b = int(qoff[q]), int(qoff[q + 1])
        n = ncand if cand_n is None else int(cand_n[q])
        got = moments(rows, zip(qk[a:b].tolist(), qo[a:b].tolist()), [(cand_sid[q][c], d_lo[q][c], d_hi[q][c]) for c in range(n)])
        out.append(got + [dict.fromkeys(SUMS, 0) for _ in range(ncand - n)])
    return out


def assert_moments(res, want, what=""):
    for q, cands in enumerate(want):
        for c, w in enumerate(cands):
            got = {f: int(res[f][q, c]) for f in SUMS}
            assert got == w, (what, q, c, got, w)


def warp_map(t: int, t16: int) -> int:
    """the warped frame of query frame t at the time factor t16 (Q16)"""
    return (int(t) * int(t16) + 32768) >> 16


def own_frames(first: int, last: int, t16: int, limit: int = 1 << 21):
    """(the smallest t >= 0 with warp_map(t) >= first, the largest t with warp_map(t) <= last), by search over the frames;
    the second is -1 where even frame 0 maps behind last (it cannot: warp_map(0) = 0)"""
    lo = next(t for t in range(limit) if warp_map(t, t16) >= first)
    hi = -1
    for t in range(limit):
        if warp_map(t, t16) > last:
            break
        hi = t
    return lo, hi


__all__ = ["SUMS", "moments", "expected_moments", "assert_moments", "warp_map", "own_frames", "expected_extents"]
