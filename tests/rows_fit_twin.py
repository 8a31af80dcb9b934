"""Test helper for the extents of warped songs (not a conftest, not collected): the definition of
shz_match_songs_warps_extents, composed from rows_warp_twin.warp_rows (the row warp), extent_twin.extents (the extent pass) and
fit_twin.moments (the four sums).  Imports nothing from the library."""
import numpy as np

from extent_twin import SCALARS, extents
from fit_twin import SUMS, moments
from rows_warp_twin import warp_rows


def song_rows(tk, ts, to, sid):
    """(key32, off) of the table's rows of song sid, as sets are: every (key, off) once, ascending"""
    m = np.asarray(ts) == int(sid)
    rows = sorted(set(zip(np.asarray(tk)[m].tolist(), np.asarray(to)[m].tolist())))
    return np.asarray([k for k, _ in rows], np.int64), np.asarray([o for _, o in rows], np.int64)


def match_songs_warps_extents(tk, ts, to, job_sid, tempos, pitches, cand_sid, d_lo, d_hi, cand_n=None, hist=False):
    """Table.match_songs_warps_extents on the rows (tk, ts, to) of a table (Table.export()): job j is song job_sid[j] under
    the row warp (tempos[j], pitches[j]); its query is the SET of its kept warped rows, its candidates are row j of the
    [n, ncand] arrays, of which it uses the first cand_n[j] (None: all).  Returns the dict of the library call: count, q_first,
    q_last, t_first, t_last [n, ncand] (uint32), hist [n, ncand, 64] or None, shift [n], sum_q, sum_u, sum_qq, sum_qu
    [n, ncand] (uint64, modulo 2^64), kept [n] (uint64: the kept warped rows BEFORE the set collapses them)."""
    n = len(job_sid)
    cs = np.asarray(cand_sid, np.int64).reshape(n, -1) if n else np.zeros((0, 1), np.int64)
    lo, hi = np.asarray(d_lo, np.int64).reshape(cs.shape), np.asarray(d_hi, np.int64).reshape(cs.shape)
    ncand = cs.shape[1]
    cn = np.full(n, ncand, np.int64) if cand_n is None else np.asarray(cand_n, np.int64).reshape(-1)
    rows = list(zip(np.asarray(tk).tolist(), np.asarray(ts).tolist(), np.asarray(to).tolist()))
    res = {f: np.zeros((n, ncand), np.uint32) for f in SCALARS}
    res.update({f: np.zeros((n, ncand), np.uint64) for f in SUMS})
    res["hist"] = np.zeros((n, ncand, 64), np.uint32) if hist else None
    res["shift"] = np.zeros(n, np.uint32)
    res["kept"] = np.zeros(n, np.uint64)
    for j in range(n):
        k, o = song_rows(tk, ts, to, job_sid[j])
        wk, wo, _ = warp_rows(k, o, int(tempos[j]), int(pitches[j]))
        res["kept"][j] = len(wk)
        hashes = list(zip(wk.tolist(), wo.tolist()))
        cands = [(int(cs[j, c]), int(lo[j, c]), int(hi[j, c])) for c in range(int(cn[j]))]
        ext, shift = extents(rows, hashes, cands)
        mom = moments(rows, hashes, cands)
        res["shift"][j] = shift
        for c in range(len(cands)):
            for f in SCALARS:
                res[f][j, c] = ext[c][f]
            for f in SUMS:
                res[f][j, c] = mom[c][f]
            if hist:
                res["hist"][j, c] = ext[c]["hist"]
    return res


class TwinTable:
    """A table that answers the two calls catalog.pair_extents_warps makes -- song_hashes(ids, counts_only=True) and
    match_songs_warps_extents -- from plain rows through the twin; `calls` keeps the arguments of every library call."""

    def __init__(self, tk, ts, to):
        rows = sorted(set(zip(np.asarray(tk).tolist(), np.asarray(ts).tolist(), np.asarray(to).tolist())))
        self.tk, self.ts, self.to = (np.asarray([r[i] for r in rows], np.int64) for i in range(3))
        self.calls = []

    def export(self):
        return self.tk.astype(np.uint32), self.ts.astype(np.uint32), self.to.astype(np.uint32)

    def song_hashes(self, sids, counts_only=False):
        parts = [song_rows(self.tk, self.ts, self.to, s) for s in np.asarray(sids).reshape(-1)]
        ro = np.concatenate([[0], np.cumsum([len(k) for k, _ in parts])]).astype(np.uint64)
        if counts_only or not parts:
            return ro, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return ro, np.concatenate([k for k, _ in parts]).astype(np.uint32), np.concatenate([o for _, o in parts]).astype(np.uint32)

    def match_songs_warps_extents(self, job_sid, tempos, pitches, cand_sid, d_lo, d_hi, cand_n=None, hist=False, timings=False):
        self.calls.append(dict(job_sid=np.asarray(job_sid).tolist(), tempos=np.asarray(tempos).tolist(), pitches=np.asarray(pitches).tolist(),
                               cand_sid=np.asarray(cand_sid).tolist(), d_lo=np.asarray(d_lo).tolist(), d_hi=np.asarray(d_hi).tolist()))
        res = match_songs_warps_extents(self.tk, self.ts, self.to, job_sid, tempos, pitches, cand_sid, d_lo, d_hi, cand_n, hist)
        if timings:
            res["ms"] = (0.0, 0.0, 0.0)
        return res


FIELDS = SCALARS + SUMS + ("shift", "kept")


def assert_same(got, want, what="", hist=False):
    """the dict of the library call against the twin's: exact, every array"""
    for f in FIELDS + (("hist",) if hist else ()):
        assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (what, f, np.asarray(got[f]).tolist(), np.asarray(want[f]).tolist())
