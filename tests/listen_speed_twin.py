"""Test helpers for the listeners at a ladder (not a conftest, not collected): the peak windows of
shz_listeners_push_warps stated in numpy.  Inputs are the oracle's peaks of every channel's WHOLE signal and the settled
horizons after a push; nothing here comes from the code under test.  The hashes go through speed_twin.warp_pair /
warp_twin.warp_pair_tf on the rebased peaks, the vote through speed_twin.aligned_votes, the choice through best_variant /
best_variant_tf."""
import numpy as np

import speed_twin as T
import warp_twin as W

NFFT, HOP, RADIUS = 4096, 2048, 10


def horizon(samples: int, ended: bool = False, hop: int = HOP) -> int:
    """Settled frames of a stream that has received `samples` samples: a frame is settled once the frame 10 behind it is
    complete; at the end every frame is (fewer than 4096 samples: the one zero-padded frame)."""
    complete = (samples - NFFT) // hop + 1 if samples >= NFFT else 0
    if ended:
        return complete if samples >= NFFT else 1
    return max(0, complete - RADIUS)


def window(peaks, horizons, window_frames: int):
    """peaks: per channel (f, t) of the whole signal, (t asc, f asc); horizons: per channel H_c after the push.  Returns
    (w0, [(f, t)] per channel): w0 = max(0, min_c H_c - window_frames), channel c's window the peaks with w0 <= t < H_c
    (absolute t).  No cut at min_c H_c: a channel that runs ahead keeps its settled peaks."""
    w0 = max(0, min(int(h) for h in horizons) - int(window_frames))
    out = []
    for (f, t), h in zip(peaks, horizons):
        f, t = np.asarray(f), np.asarray(t)
        keep = (t >= w0) & (t < int(h))
        out.append((f[keep].astype(np.uint16), t[keep].astype(np.uint32)))
    return w0, out


def hashes(win, w0: int, tempos, pitches=None, fan_value: int = 5):
    """Per warp v the (key32, t1) of the listener's query: every channel's window rebased to t - w0, warped by
    (tempos[v], pitches[v]) (pitches=None: a speed ladder, through speed_twin.warp_pair), paired; the channels one behind
    the other."""
    out = []
    for v in range(len(tempos)):
        ks, ts = [], []
        for f, t in win:
            rel = np.asarray(t).astype(np.int64) - int(w0)
            if pitches is None:
                k, t1 = T.warp_pair(f, rel, int(tempos[v]), fan_value)
            else:
                k, t1 = W.warp_pair_tf(f, rel, int(tempos[v]), int(pitches[v]), fan_value)
            ks.append(np.asarray(k, np.uint32))
            ts.append(np.asarray(t1, np.uint32))
        out.append((np.concatenate(ks) if ks else np.zeros(0, np.uint32), np.concatenate(ts) if ts else np.zeros(0, np.uint32)))
    return out


def expected(win, w0: int, table: dict, tempos, pitches=None, topn: int = 2, fan_value: int = 5) -> dict:
    """What one listener's push returns: profile [K], best, and nres / nhash / sid / delta / aligned / dedup of the best
    variant (rows beyond nres are 0)."""
    K = len(tempos)
    profile, per = np.zeros(K, np.uint32), []
    for v, (k, t1) in enumerate(hashes(win, w0, tempos, pitches, fan_value)):
        ranked, dedup, nhash = T.aligned_votes(k, t1, table, topn)
        per.append((ranked, dedup, nhash))
        profile[v] = ranked[0][2] if ranked else 0
    best = T.best_variant(profile, tempos) if pitches is None else W.best_variant_tf(profile, tempos, pitches)
    ranked, dedup, nhash = per[best]
    exp = {"profile": profile, "best": best, "nres": len(ranked), "nhash": nhash, "sid": np.zeros(topn, np.uint32),
           "delta": np.zeros(topn, np.int32), "aligned": np.zeros(topn, np.uint32), "dedup": np.zeros(topn, np.uint32)}
    for n, (sid, delta, aligned) in enumerate(ranked):
        exp["sid"][n], exp["delta"][n], exp["aligned"][n], exp["dedup"][n] = sid, delta, aligned, dedup[sid]
    return exp


def assert_listener(res, l: int, exp: dict):
    """res: Listeners.push_warps' arrays; listener l against expected()"""
    assert np.array_equal(res["profile"][l], exp["profile"]), ("profile", l, res["profile"][l].tolist(), exp["profile"].tolist())
    assert int(res["best"][l]) == exp["best"], ("best", l)
    n = exp["nres"]
    assert int(res["nres"][l]) == n and int(res["nhash"][l]) == exp["nhash"], ("nres / nhash", l)
    for name in ("sid", "delta", "aligned", "dedup"):
        assert np.array_equal(res[name][l, :n], exp[name][:n]), (name, l)
