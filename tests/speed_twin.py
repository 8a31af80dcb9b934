"""Test helpers for speed-tolerant recognition (not a conftest, not collected): the integer warp of shz_warp_pair_hash stated
in numpy, and the speed change the tests apply to their queries, which is not made by the code under test."""
import numpy as np

from oracle import cpu_ref as O

S_ONE = 65536          # the factor 1.0 in Q16
F_MAX = 2048           # the last bin of the 4096-point spectrogram


def q16(s: float) -> int:
    """round(s * 65536)"""
    return int(round(float(s) * S_ONE))


def warp_peaks(f, t, s16: int):
    """The peaks (f, t) of a query that plays s16 / 65536 times as fast as the table's copy, mapped to the table's domain:
    t' = (t s16 + 32768) >> 16, f' = (2 65536 f + s16) // (2 s16) in 64-bit integers, peaks with f' > 2048 dropped, the rest
    ordered by (t', f', original index).  Returns (f', t') as int64."""
    f, t, s16 = np.asarray(f).astype(np.int64), np.asarray(t).astype(np.int64), int(s16)
    tp = (t * s16 + 32768) >> 16
    fp = (2 * S_ONE * f + s16) // (2 * s16)
    keep = np.flatnonzero(fp <= F_MAX)
    order = keep[np.lexsort((keep, fp[keep], tp[keep]))]
    return fp[order], tp[order]


def warp_pair(f, t, s16: int, fan_value: int = 5):
    """(key32, t1) of the warped peaks, paired like generate_hashes (oracle.cpu_ref.pair_keys)."""
    return O.pair_keys(*warp_peaks(f, t, s16), fan_value)


def warp_pair_batch(peak_f, peak_t, peak_off, query_clip0, speeds, fan_value: int = 5):
    """shz_warp_pair_hash in numpy: (key32, t1, hash_off) in the library's order -- for query q, for speed v, for every clip c
    of q: the hashes of (c, v); hash_off has n_clips * n_speeds + 1 entries in that order."""
    ks, ts, off = [], [], [0]
    for q in range(len(query_clip0) - 1):
        for s16 in speeds:
            for c in range(int(query_clip0[q]), int(query_clip0[q + 1])):
                a, b = int(peak_off[c]), int(peak_off[c + 1])
                k, t1 = warp_pair(peak_f[a:b], peak_t[a:b], int(s16), fan_value)
                ks.append(k)
                ts.append(t1)
                off.append(off[-1] + len(k))
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)
    return cat(ks), cat(ts), np.asarray(off, np.uint64)


def speed_up(x, s: float):
    """x played s times as fast, by linear interpolation: y[n] = x(n s), rounded to int16."""
    x = np.asarray(x).astype(np.float64)
    n = int((len(x) - 1) / float(s)) + 1 if len(x) else 0
    pos = np.arange(n, dtype=np.float64) * float(s)
    return np.clip(np.rint(np.interp(pos, np.arange(len(x), dtype=np.float64), x)), -32768, 32767).astype(np.int16)


def aligned_votes(key32, t1, table: dict, topn: int = 2):
    """The vote of recognizer.py:222-338 for one query given as packed hashes: table maps key32 -> list of (sid, offset).
    Set semantics on (key, t1); returns (ranked [(sid, delta, aligned)], dedup {sid: rows}, distinct hashes)."""
    pairs = sorted(set(zip(np.asarray(key32).tolist(), np.asarray(t1).tolist())))
    matches, dedup, seen = [], {}, set()
    for k, q in pairs:
        for sid, off in table.get(k, ()):
            matches.append((sid, off - q))
            if k not in seen:
                dedup[sid] = dedup.get(sid, 0) + 1
        seen.add(k)
    return O.vote(matches, topn), dedup, len(pairs)


def table_of(songs_keys):
    """key32 -> [(sid, offset)] with UNIQUE(sid, offset, hash); songs_keys: list of (key32, t1), song ids from 1."""
    table = {}
    for sid, (k, t1) in enumerate(songs_keys, 1):
        for kk, tt in sorted(set(zip(np.asarray(k).tolist(), np.asarray(t1).tolist()))):
            table.setdefault(kk, []).append((sid, tt))
    return table


def best_variant(top1_aligned, speeds) -> int:
    """Index of the greatest top-1 aligned count; ties to the factor nearest 65536, then to the lower index."""
    return min(range(len(speeds)), key=lambda v: (-int(top1_aligned[v]), abs(int(speeds[v]) - S_ONE), v))
