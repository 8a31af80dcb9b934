"""Test helpers for the scan over warp pairs (not a conftest, not collected): the window cut of shz_scan_warps with the time
factor alone, the host recipe with an optional per-window selection, the best-variant fold and the timeline of
shz_scan_timeline_warps, stated in numpy / plain Python on warp_twin.py and scan_speed_twin.py."""
import numpy as np

import scan_speed_twin as ST
import warp_twin as WT

S_ONE = 65536
NO_WARP = 0xFFFFFFFF
ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
W, window_count = ST.W, ST.window_count


def cut_windows(chan_hashes, n_wins: int, window: int, step: int, t16: int):
    """The queries of one recording at one warp: scan_speed_twin's cut with the TIME factor -- the pitch never enters a time."""
    return ST.cut_windows(chan_hashes, n_wins, window, step, int(t16))


def full_selection(n_wins: int, n_warps: int):
    return (np.arange(n_wins + 1, dtype=np.uint64) * n_warps, np.tile(np.arange(n_warps, dtype=np.uint32), n_wins))


def host_queries(chan_peaks, frames, window, step, tempos, pitches, select=None, fan_value=5):
    """Every query of a batch: chan_peaks[r] = [(f, t) per channel], frames[r] = the recording's frames.  Dense: query
    (w, v) at index w * K + v.  select=(sel_off, sel_warp): one query a slot, in slot order.  Returns (key32, q_off,
    query_off, win_off, work): work = (hashes of every recording at every warp in use, cut entries)."""
    K = len(tempos)
    n_wins = [window_count(int(F), window, step) if peaks else 0 for peaks, F in zip(chan_peaks, frames)]
    win_off = np.concatenate([[0], np.cumsum(n_wins)]).astype(np.uint64)
    if select is None:
        select = full_selection(int(win_off[-1]), K)
    so, sw = (np.asarray(a).astype(np.int64) for a in select)
    used = np.unique(sw[:int(so[-1])]).tolist()
    keys, qoffs, query_off, n_hashes = [], [], [0], 0
    for r, (peaks, nw) in enumerate(zip(chan_peaks, n_wins)):
        cuts = {}
        for v in used:
            hashes = [WT.warp_pair_tf(f, t, int(tempos[v]), int(pitches[v]), fan_value) for f, t in peaks]
            n_hashes += sum(len(k) for k, _ in hashes) if nw else 0
            cuts[v] = cut_windows(hashes, nw, window, step, int(tempos[v]))
        for w in range(nw):
            g = int(win_off[r]) + w
            for v in sw[so[g]:so[g + 1]].tolist():
                k, q = cuts[v][w]
                keys.append(k)
                qoffs.append(q)
                query_off.append(query_off[-1] + len(k))
    cat = lambda xs: np.concatenate(xs).astype(np.uint32) if xs else np.zeros(0, np.uint32)   # noqa: E731
    return cat(keys), cat(qoffs), np.asarray(query_off, np.uint64), win_off, (n_hashes, query_off[-1])


def fold_best(match, n_wins: int, tempos, pitches, topn: int, select=None):
    """Table.match's arrays over the queries -> what shz_scan_warps returns: profile (dense: [n_wins, K]; with a selection:
    slot-aligned), best, the best variant's rows; a window without a slot: zeros and NO_WARP."""
    K = len(tempos)
    dense = select is None
    so, sw = (np.asarray(a).astype(np.int64) for a in (full_selection(n_wins, K) if dense else select))
    top1 = np.where(match["nres"] > 0, match["aligned"][:, 0], 0).astype(np.uint32) if len(match["nres"]) else np.zeros(0, np.uint32)
    out = {k: np.zeros((n_wins,) + match[k].shape[1:], match[k].dtype) for k in ARRAYS}
    best = np.full(n_wins, NO_WARP, np.uint32)
    for w in range(n_wins):
        a, b = int(so[w]), int(so[w + 1])
        if a == b:
            continue
        vs = sw[a:b]
        j = WT.best_variant_tf(top1[a:b], [tempos[v] for v in vs], [pitches[v] for v in vs])
        best[w] = vs[j]
        for k in ARRAYS:
            out[k][w] = match[k][a + j]
    out["profile"], out["best"] = (top1.reshape(n_wins, K) if dense else top1), best
    return out


def timeline(win_off, sid, delta, aligned, nres, best, step, tempos, pitches, min_aligned, max_gap=1, tempo_tol=0, pitch_tol=0,
             shift_tol=2):
    """shz_scan_timeline_warps in plain Python: a list of dicts rec, sid, first, last, hits, best, pos_first, pos_last, warp."""
    sid, delta, aligned = (np.asarray(a).reshape(len(nres), -1)[:, 0] for a in (sid, delta, aligned))
    segs = []
    for r in range(len(win_off) - 1):
        cur = None
        for w in range(int(win_off[r + 1]) - int(win_off[r])):
            g = int(win_off[r]) + w
            if int(nres[g]) < 1 or int(aligned[g]) < min_aligned:
                continue
            s, a, v, pos = int(sid[g]), int(aligned[g]), int(best[g]), int(delta[g])
            if (cur is not None and s == cur["sid"] and w - cur["last"] - 1 <= max_gap and
                    abs(int(tempos[v]) - int(tempos[cur["_v"]])) <= tempo_tol and
                    abs(int(pitches[v]) - int(pitches[cur["_v"]])) <= pitch_tol and
                    abs(pos - cur["pos_last"] - W((w - cur["last"]) * step, tempos[v])) <= shift_tol):
                cur.update(last=w, hits=cur["hits"] + 1, best=max(cur["best"], a), pos_last=pos, _v=v)
                cur["_n"][v] += 1
                continue
            if cur is not None:
                segs.append(cur)
            cur = dict(rec=r, sid=s, first=w, last=w, hits=1, best=a, pos_first=pos, pos_last=pos, _v=v, _n=[0] * len(tempos))
            cur["_n"][v] = 1
        if cur is not None:
            segs.append(cur)
    for c in segs:
        c["warp"] = WT.best_variant_tf(c.pop("_n"), tempos, pitches)
        del c["_v"]
    return segs
