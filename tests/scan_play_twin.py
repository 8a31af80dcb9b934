"""Test helper for the warped scan extents (not a conftest, not collected): the definitions of shz_scan_play_zones and of the
zone results and work counts of shz_scan_plays in plain Python over warp_twin / scan_warp_twin / scan_extent_twin / extent_twin
/ fit_twin.  Imports nothing from the library.

A segment is (r, sid, a, b, p_a, p_b, t16, f16): recording, song, first and last window, the song frames at the starts of those
windows, and its own Q16 pair.  With W(x) = (x t16 + 32768) >> 16:

  zones      [lo, hi) in the recording's own frames = scan_extent_twin.zones with every shift 0 (the identity that clamps the
             margins is (r, sid)); their warped borders W(lo), W(hi); zone z of segment i at 3 i + z: whole, head, tail
  query      the union over the recording's channels of (key32, t1' - W(lo)) for the entries of the FULL warped hash list of
             the whole channel at (t16, f16) with W(lo) <= t1' < W(hi)
  candidate  c_a = p_a - W(a S) + W(lo), c_b = p_b - W(b S) + W(lo), w = tolerance + drift_bins:
             zone 0 (sid, min(c_a, c_b) - w, max(c_a, c_b) + w), zone 1 (sid, c_a - w, c_a + w), zone 2 (sid, c_b - w, c_b + w);
             wholly outside int32: no candidate; else clamped to int32
  result     extent_twin.extents and fit_twin.moments for that query and candidate, q_first / q_last + W(lo) where count > 0

The work counts follow the device stage's JOBS, which are part of the contract: one job per (segment, channel) keeps the
channel's peaks with W(lo0) <= W(t) <= W(hi0) - 1 + 200 ([lo0, hi0) = zone 0); work = (peaks kept over all jobs, hashes of
warp_pair_tf on every job's kept peaks, entries cut over all zones and channels)."""
import numpy as np

import extent_twin
import fit_twin
import scan_extent_twin
import scan_warp_twin as SW
import warp_twin as WT

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAX_DT = 200
W = SW.W
ZONE_KEYS = ("lo", "hi", "d_lo", "d_hi", "count", "q_first", "q_last", "t_first", "t_last", "shift") + fit_twin.SUMS


def play_zones(segs, frames, window, step, margin, w):
    """shz_scan_play_zones: per zone (3 i + z) a dict lo, hi, wlo, whi, d_lo, d_hi, cand_n."""
    own = scan_extent_twin.zones([(r, sid, 0, a, b) for r, sid, a, b, *_ in segs], frames, window, step, margin)
    out = []
    for i, (r, sid, a, b, p_a, p_b, t16, *_) in enumerate(segs):
        for z in range(3):
            lo, hi = own[3 * i + z]
            wlo, whi = W(lo, t16), W(hi, t16)
            c_a = int(p_a) - W(int(a) * int(step), t16) + wlo
            c_b = int(p_b) - W(int(b) * int(step), t16) + wlo
            d_lo, d_hi = ((min(c_a, c_b), max(c_a, c_b)), (c_a, c_a), (c_b, c_b))[z]
            d_lo, d_hi = d_lo - int(w), d_hi + int(w)
            if d_lo > I32_MAX or d_hi < I32_MIN:
                out.append(dict(lo=lo, hi=hi, wlo=wlo, whi=whi, d_lo=0, d_hi=0, cand_n=0))
            else:
                out.append(dict(lo=lo, hi=hi, wlo=wlo, whi=whi, d_lo=max(d_lo, I32_MIN), d_hi=min(d_hi, I32_MAX), cand_n=1))
    return out


def refusal(segs, frames, window, step, margin, w):
    """What shz_scan_play_zones refuses about segments shz_scan_zones accepts: "invalid" (a time factor outside [32768, 131072]),
    "unsupported" (a zone of 2^20 warped frames or more; then a used candidate 4,096 bins or more wide), or None."""
    if any(not 32768 <= int(s[6]) <= 131072 for s in segs):
        return "invalid"
    zs = play_zones(segs, frames, window, step, margin, w)
    if any(z["whi"] - z["wlo"] >= 1 << 20 for z in zs):
        return "unsupported"
    if any(z["cand_n"] and z["d_hi"] - z["d_lo"] >= 4096 for z in zs):
        return "unsupported"
    return None


class Lists:
    """The full warped hash lists of the channels, computed once per (channel, pair, fan)."""

    def __init__(self, chan_peaks, fan_value=5):
        self.peaks, self.fan, self.cache = chan_peaks, int(fan_value), {}

    def full(self, c, t16, f16):
        key = (int(c), int(t16), int(f16))
        if key not in self.cache:
            f, t = self.peaks[c]
            k, t1 = WT.warp_pair_tf(f, t, int(t16), int(f16), self.fan)
            self.cache[key] = (np.asarray(k).astype(np.int64), np.asarray(t1).astype(np.int64))
        return self.cache[key]

    def cut(self, c, t16, f16, wlo, whi):
        """the entries of channel c's full list with wlo <= t1' < whi: (key32, t1' - wlo) as two lists"""
        k, t1 = self.full(c, t16, f16)
        m = (t1 >= wlo) & (t1 < whi)
        return k[m].tolist(), (t1[m] - wlo).tolist()

    def job(self, c, t16, f16, wlo0, whi0):
        """(peaks kept, hashes written) of the job of channel c for a zone 0 of warped borders [wlo0, whi0)"""
        f, t = (np.asarray(x).astype(np.int64) for x in self.peaks[c])
        wt = (t * int(t16) + 32768) >> 16
        m = (wt >= wlo0) & (wt <= whi0 - 1 + MAX_DT)
        return int(m.sum()), len(WT.warp_pair_tf(f[m], t[m], int(t16), int(f16), self.fan)[0])


def zone_results(rows, chan_peaks, rec_clip0, segs, frames, window, step, margin, w, fan_value=5):
    """rows = (key, sid, off) of the table; chan_peaks[c] = (f, t) of channel c.  Returns (per zone a dict of ZONE_KEYS and
    hist[64], work): what shz_scan_plays writes."""
    by_sid = {}                                   # song -> key -> its rows, indexed once
    for k, s, o in rows:
        by_sid.setdefault(int(s), {}).setdefault(int(k), []).append((int(k), int(s), int(o)))
    L = Lists(chan_peaks, fan_value)
    zs = play_zones(segs, frames, window, step, margin, w)
    out, items, hashes, entries = [], 0, 0, 0
    for i, (r, sid, a, b, p_a, p_b, t16, f16) in enumerate(segs):
        chans = range(int(rec_clip0[int(r)]), int(rec_clip0[int(r) + 1]))
        for c in chans:
            n, h = L.job(c, t16, f16, zs[3 * i]["wlo"], zs[3 * i]["whi"])
            items, hashes = items + n, hashes + h
        for z in zs[3 * i:3 * i + 3]:
            q = set()
            for c in chans:
                k, qo = L.cut(c, t16, f16, z["wlo"], z["whi"])
                entries += len(k)
                q.update(zip(k, qo))
            cands = [(int(sid), z["d_lo"], z["d_hi"])] * z["cand_n"]
            # (a pair needs the candidate's song and the hash's key: the rows of that song under the query's keys suffice)
            index = by_sid.get(int(sid), {})
            srows = [row for k in {k for k, _ in q} for row in index.get(k, ())]
            res, shift = extent_twin.extents(srows, q, cands)
            d = dict(res[0]) if res else {"count": 0, "q_first": 0, "q_last": 0, "t_first": 0, "t_last": 0, "hist": [0] * 64}
            d.update(fit_twin.moments(srows, q, cands)[0] if cands else dict.fromkeys(fit_twin.SUMS, 0))
            d.update(lo=z["lo"], hi=z["hi"], d_lo=z["d_lo"], d_hi=z["d_hi"], shift=shift, wlo=z["wlo"])
            if d["count"]:
                d["q_first"] += z["wlo"]
                d["q_last"] += z["wlo"]
            out.append(d)
    return out, (items, hashes, entries)


def assert_zones(zone, want, what=""):
    """Context.scan_plays' arrays [n_segs, 3] against zone_results' list: every field and every histogram, exact"""
    flat = {k: zone[k].reshape(-1) for k in ZONE_KEYS}
    hist = None if zone.get("hist") is None else zone["hist"].reshape(-1, 64)
    assert len(flat["lo"]) == len(want), (what, len(flat["lo"]), len(want))
    for z, tw in enumerate(want):
        got = {k: int(flat[k][z]) for k in ZONE_KEYS}
        assert got == {k: tw[k] for k in ZONE_KEYS}, (what, z, got, {k: tw[k] for k in ZONE_KEYS})
        if hist is not None:
            assert hist[z].tolist() == tw["hist"], (what, "hist", z)
