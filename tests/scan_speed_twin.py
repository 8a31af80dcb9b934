"""Test helpers for the speed-tolerant scan (not a conftest, not collected): the window cut of shz_scan_speeds and the
local-continuity timeline of shz_scan_timeline_speeds, stated in numpy / plain Python."""
import numpy as np

import speed_twin as T

S_ONE = 65536


def W(x: int, s16: int) -> int:
    """The warp's time map in unbounded integers: (x s16 + 32768) >> 16."""
    return (int(x) * int(s16) + 32768) >> 16


def window_count(frames: int, window: int, step: int) -> int:
    return 0 if frames == 0 else 1 if frames <= window else -(-(frames - window) // step) + 1


def cut_windows(chan_hashes, n_wins: int, window: int, step: int, s16: int):
    """The queries of one recording at one rung.  chan_hashes: per channel (key32, t1') of the warped list (t1' does not
    decrease).  Window w is the union over the channels of the entries with W(s) <= t1' < W(s + window), s = w step, its
    query offsets t1' - W(s).  Returns a list of (key32, q_off) per window, channels one behind the other."""
    out = []
    for w in range(n_wins):
        s = w * step
        lo, hi = W(s, s16), W(s + window, s16)
        ks, qs = [], []
        for k, t1 in chan_hashes:
            t1 = np.asarray(t1).astype(np.int64)
            m = (t1 >= lo) & (t1 < hi)
            ks.append(np.asarray(k)[m].astype(np.uint32))
            qs.append((t1[m] - lo).astype(np.uint32))
        out.append((np.concatenate(ks) if ks else np.zeros(0, np.uint32), np.concatenate(qs) if qs else np.zeros(0, np.uint32)))
    return out


def host_queries(chan_peaks, frames, window, step, speeds, fan_value=5):
    """Every (window, rung) query of a batch, window-major and rung-minor: chan_peaks[r] = [(f, t) per channel], frames[r] =
    the recording's frames.  Returns (key32, q_off, query_off, win_off) for Table.match: query (w, v) at index w * K + v."""
    keys, qoffs, query_off, win_off = [], [], [0], [0]
    K = len(speeds)
    for peaks, F in zip(chan_peaks, frames):
        nw = window_count(int(F), window, step) if peaks else 0
        per_rung = []
        for s16 in speeds:
            hashes = [T.warp_pair(f, t, int(s16), fan_value) for f, t in peaks]
            per_rung.append(cut_windows(hashes, nw, window, step, int(s16)))
        for w in range(nw):
            for v in range(K):
                k, q = per_rung[v][w]
                keys.append(k)
                qoffs.append(q)
                query_off.append(query_off[-1] + len(k))
        win_off.append(win_off[-1] + nw)
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)   # noqa: E731
    return cat(keys), cat(qoffs), np.asarray(query_off, np.uint64), np.asarray(win_off, np.uint64)


def fold_best(match, n_wins: int, speeds, topn: int):
    """Table.match's arrays over (window, rung) queries -> what shz_scan_speeds returns: profile, best, the best rung's rows."""
    K = len(speeds)
    top1 = np.where(match["nres"] > 0, match["aligned"][:, 0], 0).astype(np.uint32).reshape(n_wins, K)
    best = np.asarray([T.best_variant(top1[w], speeds) for w in range(n_wins)], np.uint32)
    pick = np.arange(n_wins, dtype=np.int64) * K + best
    out = {k: match[k][pick] for k in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")}
    out["profile"], out["best"] = top1, best
    return out


def timeline(win_off, sid, delta, aligned, nres, best, step, speeds, min_aligned, max_gap=1, rung_tol=1, shift_tol=2):
    """shz_scan_timeline_speeds in plain Python: a list of dicts rec, sid, first, last, hits, best, pos_first, pos_last, rung."""
    sid, delta, aligned = (np.asarray(a).reshape(len(nres), -1)[:, 0] for a in (sid, delta, aligned))
    segs = []
    for r in range(len(win_off) - 1):
        cur = None
        for w in range(int(win_off[r + 1]) - int(win_off[r])):
            g = int(win_off[r]) + w
            if int(nres[g]) < 1 or int(aligned[g]) < min_aligned:
                continue
            s, a, v, pos = int(sid[g]), int(aligned[g]), int(best[g]), int(delta[g])
            if (cur is not None and s == cur["sid"] and w - cur["last"] - 1 <= max_gap and abs(v - cur["_v"]) <= rung_tol and
                    abs(pos - cur["pos_last"] - W((w - cur["last"]) * step, speeds[v])) <= shift_tol):
                cur.update(last=w, hits=cur["hits"] + 1, best=max(cur["best"], a), pos_last=pos, _v=v)
                cur["_n"][v] += 1
                continue
            if cur is not None:
                segs.append(cur)
            cur = dict(rec=r, sid=s, first=w, last=w, hits=1, best=a, pos_first=pos, pos_last=pos, _v=v, _n=[0] * len(speeds))
            cur["_n"][v] = 1
        if cur is not None:
            segs.append(cur)
    for c in segs:
        c["rung"] = T.best_variant(c.pop("_n"), speeds)
        del c["_v"]
    return segs
