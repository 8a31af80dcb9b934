"""Test helper for the scan extents (not a conftest, not collected): the definition of shz_scan_zones and of the zone
results of shz_scan_extents in plain Python and numpy.  Imports nothing from the library.

A scan and its timeline give segments (recording r, song sid, shift h = song frame - recording frame, first window a, last
window b).  With W = window_frames, S = step_frames, F = the recording's frame count, M = margin_frames every segment gets
three ZONES, half-open ranges [lo, hi) of recording frames:

  0 whole  [max(0, aS - M), min(F, bS + W + M))   the pairs of the whole play, its span in the song, a coarse histogram
  1 head   [max(0, aS - M), min(F, aS + W))       where the play starts, at a fine bucket width
  2 tail   [bS,             min(F, bS + W + M))   where the play ends, at a fine bucket width

clamped against the segments of the SAME identity (r, sid, h): with L = the largest b_k S + W over earlier ones, the lo of
zones 0 and 1 is at least min(L, aS); with R = the smallest a_k S over later ones, the hi of zones 0 and 2 is at most
max(R, bS + W).  Every bound is then clamped into [0, F]; a zone with lo >= hi after that is EMPTY and is reported as
hi = lo.  Zone z of segment i sits at 3 i + z.

The query of a zone is the set, over the recording's channels, of (key32, t1 - lo) for the hashes with lo <= t1 < hi; its one
candidate is (sid, h + lo - tol, h + lo + tol); its result is what tests/extent_twin.py defines for that query and
candidate, q_first / q_last reported in recording frames (+ lo) where count > 0."""
import extent_twin


def zones(segs, frames, W, S, M):
    """segs = [(r, sid, h, a, b)] in the timeline's order; frames[r] = F_r.  Returns [(lo, hi)] * 3 len(segs)."""
    W, S, M = int(W), int(S), int(M)
    out = []
    for i, (r, sid, h, a, b) in enumerate(segs):
        r, a, b, F = int(r), int(a), int(b), int(frames[int(r)])
        same = lambda k: (int(segs[k][0]), int(segs[k][1]), int(segs[k][2])) == (r, int(sid), int(h))   # noqa: E731
        lo = max(0, a * S - M)
        hi = b * S + W + M
        before = [int(segs[k][4]) * S + W for k in range(i) if same(k)]
        after = [int(segs[k][3]) * S for k in range(i + 1, len(segs)) if same(k)]
        if before:
            lo = max(lo, min(max(before), a * S))
        if after:
            hi = min(hi, max(min(after), b * S + W))
        for zl, zh in ((lo, hi), (lo, a * S + W), (b * S, hi)):
            zl, zh = min(zl, F), min(zh, F)
            out.append((zl, max(zl, zh)))
    return out


def zone_query(chan_hashes, clips, lo, hi):
    """chan_hashes[c] = (key32, t1) arrays of channel c; clips = the recording's channels -> the set {(key, t1 - lo)}"""
    q = set()
    for c in clips:
        k, t1 = chan_hashes[c]
        for kk, tt in zip(k.tolist(), t1.tolist()):
            if lo <= tt < hi:
                q.add((kk, tt - lo))
    return q


def zone_results(rows, chan_hashes, rec_clip0, segs, frames, W, S, M, tol):
    """rows = (key, sid, off) of the table.  Per zone (3 i + z) a dict: lo, hi, count, q_first, q_last (recording frames),
    t_first, t_last, hist[64], shift."""
    rows = list(rows)
    out = []
    for (r, sid, h, a, b), z3 in zip(segs, zip(*[iter(zones(segs, frames, W, S, M))] * 3)):
        for lo, hi in z3:
            q = zone_query(chan_hashes, range(int(rec_clip0[int(r)]), int(rec_clip0[int(r) + 1])), lo, hi)
            (res,), shift = extent_twin.extents(rows, q, [(int(sid), int(h) + lo - int(tol), int(h) + lo + int(tol))])
            d = dict(res, lo=lo, hi=hi, shift=shift)
            if d["count"]:
                d["q_first"] += lo
                d["q_last"] += lo
            out.append(d)
    return out
