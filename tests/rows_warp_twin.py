"""Test helpers for the row warp (not a conftest, not collected): the integer map of shz_warp_rows stated in numpy, and a
dict-table reference for shz_match_songs_warps built on speed_twin.aligned_votes with the song itself left out."""
import numpy as np

from speed_twin import F_MAX, S_ONE, aligned_votes, q16  # noqa: F401  (re-exported for the tests)

MAX_DT = 200


def warp_rows(key32, off, t16: int, f16: int):
    """The rows (key32 = f1 << 20 | f2 << 8 | dt, off = t1) under the warp (t16, f16), in 64-bit integers: both peaks of a row
    moved by t' = (t t16 + 32768) >> 16 and f' = (2 65536 f + f16) // (2 f16), the key formed again; rows with f1' > 2048,
    f2' > 2048 or dt' > 200 dropped, the rest in input order.  Returns (key32', off', keep) -- two uint32 columns of the kept
    rows and the mask over the input."""
    k, o, t16, f16 = np.asarray(key32).astype(np.int64), np.asarray(off).astype(np.int64), int(t16), int(f16)
    f1, f2, dt = k >> 20, (k >> 8) & 0xFFF, k & 0xFF
    t1 = (o * t16 + 32768) >> 16
    t2 = ((o + dt) * t16 + 32768) >> 16
    g1 = (2 * S_ONE * f1 + f16) // (2 * f16)
    g2 = (2 * S_ONE * f2 + f16) // (2 * f16)
    d = t2 - t1
    keep = (g1 <= F_MAX) & (g2 <= F_MAX) & (d <= MAX_DT)
    out = (g1 << 20) | (g2 << 8) | d
    return out[keep].astype(np.uint32), t1[keep].astype(np.uint32), keep


def warp_rows_batch(key32, off, row_off, tempos, pitches):
    """shz_warp_rows in numpy: (key32', off', out_row_off) in the library's order -- for song q, for warp v, the kept rows
    of q in input order; out_row_off has n_songs * n_warps + 1 entries."""
    assert len(tempos) == len(pitches)
    ks, os_, ro = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [0]
    for q in range(len(row_off) - 1):
        a, b = int(row_off[q]), int(row_off[q + 1])
        for t16, f16 in zip(tempos, pitches):
            k, o, _ = warp_rows(key32[a:b], off[a:b], int(t16), int(f16))
            ks.append(k)
            os_.append(o)
            ro.append(ro[-1] + len(k))
    return np.concatenate(ks), np.concatenate(os_), np.asarray(ro, np.uint64)


def table_of_rows(key32, sid, off):
    """key32 -> [(sid, offset)] from the rows of a table, every (key, sid, offset) once"""
    table = {}
    for k, s, o in sorted(set(zip(np.asarray(key32).tolist(), np.asarray(sid).tolist(), np.asarray(off).tolist()))):
        table.setdefault(k, []).append((s, o))
    return table


def match_songs_warps(table: dict, songs: dict, sids, tempos, pitches, topn: int):
    """The reference of shz_match_songs_warps on a dict table: songs maps sid -> (key32, off), the song's rows.  Returns
    res[q][v] = (ranked [(sid, delta, aligned)] without the song itself, at most topn; distinct warped rows)."""
    res = []
    for s in sids:
        k, o = songs.get(int(s), (np.zeros(0, np.int64), np.zeros(0, np.int64)))
        per = []
        for t16, f16 in zip(tempos, pitches):
            wk, wo, _ = warp_rows(k, o, int(t16), int(f16))
            ranked, _, nhash = aligned_votes(wk, wo, table, topn + 1)
            per.append(([r for r in ranked if r[0] != int(s)][:topn], nhash))
        res.append(per)
    return res
