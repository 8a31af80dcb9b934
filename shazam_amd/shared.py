"""Content shared between recordings, without a catalogue (csrc/shz_repeat.hip: shz_shared_*): "which
stretches of station A also aired on station B?", "which of Monday's adverts came back on Tuesday?", "where does this tape
overlap that one?" -- and, with a day cut into two recordings, the night re-run of daytime content that find_repeats cannot
see because no pair crosses recordings there.

A JOB is a pair of recordings (a, b).  A hash of a at time t_a and a hash of b with the same key at time t_b vote for the
SIGNED lag t_b - t_a; a stretch that airs in both piles its votes on one lag over a contiguous stretch of t_a.  The device
counts the votes per cell (job, lag, block of 2^cell_shift frames of a), the host joins neighbouring cells into shared
stretches with the fold of find_repeats (shz_repeats_fold), the jobs standing in for its recordings.  Every recording of a
call is fingerprinted once, however many jobs name it, and its hashes never leave the device."""
from __future__ import annotations

import numpy as np

from ._ffi import HOP, SHARED_LAG_BIAS
from .repeats import FIRST_ROOM, MAX_LAG, _fold

MAX_JOBS = 4096          # jobs of one library call (shz_shared_*): more are split
MAX_RECS = 4096          # recordings of one library call: a call carries only those its jobs name


def _all_pairs(n_recs: int) -> list:
    """pairs=None: every a < b"""
    return [(a, b) for a in range(n_recs) for b in range(a + 1, n_recs)]


def _check_pairs(pairs, n_recs: int) -> list:
    pairs = _all_pairs(n_recs) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if a == b or not (0 <= a < n_recs and 0 <= b < n_recs):
            raise ValueError(f"pair ({a}, {b}): two different recordings below {n_recs} are needed")
    return pairs


def _lag_window(min_lag_seconds, max_lag_seconds, fs: int, hop: int):
    """Signed seconds -> signed frames; None: that end of the range the library holds, -+(2^20 - 1) frames."""
    frames = lambda s: max(-MAX_LAG, min(MAX_LAG, int(round(float(s) * fs / hop))))   # noqa: E731
    lo = -MAX_LAG if min_lag_seconds is None else frames(min_lag_seconds)
    hi = MAX_LAG if max_lag_seconds is None else frames(max_lag_seconds)
    if hi < lo:
        raise ValueError(f"max_lag_seconds gives {hi} frames, below min_lag_seconds' {lo}")
    return lo, hi


def _plan_calls(pairs) -> list:
    """The job list cut into library calls: consecutive jobs, at most MAX_JOBS of them naming at most MAX_RECS recordings.
    Returns (first job, jobs of the call, the recordings they name in ascending order) per call."""
    calls, j0, named = [], 0, set()
    for j, (a, b) in enumerate(pairs):
        if j - j0 >= MAX_JOBS or len(named | {a, b}) > MAX_RECS:
            calls.append((j0, pairs[j0:j], sorted(named)))
            j0, named = j, set()
        named |= {a, b}
    if j0 < len(pairs):
        calls.append((j0, pairs[j0:], sorted(named)))
    return calls


def _shared_dicts(cells, rep, job0: int, jobs, recs, fs: int, hop: int) -> list:
    """jobs: the call's (a, b) in the caller's numbering; recs: the caller's number of every recording of the call"""
    secs = lambda frames: round(float(frames) * hop / fs, 5)                      # noqa: E731
    local = {r: i for i, r in enumerate(recs)}
    out = []
    for i in range(len(rep["rec"])):
        j, first, last = (int(rep[k][i]) for k in ("rec", "first", "last"))
        lag, lag_lo, lag_hi = (int(rep[k][i]) - SHARED_LAG_BIAS for k in ("lag", "lag_lo", "lag_hi"))
        a, b = jobs[j]
        out.append({
            "recording_a": a, "recording_b": b,
            "a_start_seconds": secs(first), "a_end_seconds": secs(last + 1),
            "b_start_seconds": secs(max(0, first + lag)), "b_end_seconds": secs(last + lag + 1),
            "lag_seconds": secs(lag),
            "job": job0 + j, "rec_a": a, "rec_b": b, "first": first, "last": last, "lag": lag, "lag_lo": lag_lo, "lag_hi": lag_hi,
            "pairs": int(rep["pairs"][i]), "cells": int(rep["cells"][i]),
            "stats": {"hashes_a": int(cells["rec_hashes"][local[a]]), "hashes_b": int(cells["rec_hashes"][local[b]]),
                      "pairs": int(cells["job_pairs"][j]), "skipped_keys": int(cells["job_skipped_keys"][j]),
                      "skipped_rows": int(cells["job_skipped_rows"][j])},
        })
    return out


def find_shared(recordings, pairs=None, Fs: int = 44100, min_lag_seconds: float = None, max_lag_seconds: float = None,
                cell_shift: int = 5, min_cell_pairs: int = 8, lag_tol: int = 1, max_gap: int = 1, min_pairs: int = 100,
                max_run: int = 64, resample_to: int = None, ctx=None) -> list:
    """The stretches that pairs of recordings share.  recordings: 1-D int16 arrays, or lists of channels, as find_repeats takes
    them.  pairs: the jobs (a, b), "what of recording a also airs in recording b" (None: every a < b); a recording may be named
    any number of times, (a, b) and (b, a) may both be listed, and a pair listed twice is answered twice.  The lag is t_b - t_a,
    SIGNED: min_lag_seconds .. max_lag_seconds bound it (None: that end of what the library holds, -+(2^20 - 1) frames).
    cell_shift, min_cell_pairs, lag_tol, max_gap, min_pairs, max_run and resample_to as find_repeats; a key with more than
    max_run times in either recording of a job is a stop hash there.
    More than 4,096 jobs, or jobs that name more than 4,096 recordings, are cut into library calls of consecutive jobs; a call
    carries only the recordings its jobs name, so a recording named by jobs of two calls is fingerprinted twice.
    Returns one dict per shared stretch, ordered by (job, first, lag): recording_a, recording_b; a_start_seconds /
    a_end_seconds (the stretch in a), b_start_seconds / b_end_seconds (in b; the start not below 0), lag_seconds (signed); the
    integers job (index into pairs), rec_a, rec_b, first, last (frames of a, inclusive), lag (the lag with the most pairs),
    lag_lo, lag_hi (signed), pairs, cells; and stats: hashes_a, hashes_b, and the job's pairs, skipped_keys, skipped_rows."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, get_context, resample_to_device
    from .scan import _flatten
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP))
    recordings = list(recordings)
    pairs = _check_pairs(pairs, len(recordings))
    resampled = resample_to is not None and int(resample_to) != int(Fs)
    fs = int(resample_to) if resampled else int(Fs)
    lo, hi = _lag_window(min_lag_seconds, max_lag_seconds, fs, hop)
    kw = dict(max_run=int(max_run), cell_shift=int(cell_shift), min_cell_pairs=int(min_cell_pairs), fs=fs,
              amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE, cap_cells=FIRST_ROOM)
    out = []
    for job0, jobs, recs in _plan_calls(pairs):
        local = {r: i for i, r in enumerate(recs)}
        ljobs = [(local[a], local[b]) for a, b in jobs]
        chans, first = _flatten([recordings[r] for r in recs])
        if resampled:
            buf, off = resample_to_device(chans, int(Fs), fs, ctx)
            try:
                cells, _ = ctx.shared_batch(buf, off, first, ljobs, lo, hi, pcm_device=True, **kw)
            finally:
                buf.free()
        else:
            off = np.zeros(len(chans) + 1, np.uint64)
            off[1:] = np.cumsum([len(c) for c in chans])
            pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
            cells, _ = ctx.shared_batch(pcm, off, first, ljobs, lo, hi, **kw)
        out.extend(_shared_dicts(cells, _fold(cells, lag_tol, max_gap, min_pairs), job0, jobs, recs, fs, hop))
    return out


def find_shared_hashes(key32, t1, hash_off, rec_clip0=None, pairs=None, Fs: int = 44100, min_lag_seconds: float = None,
                       max_lag_seconds: float = None, cell_shift: int = 5, min_cell_pairs: int = 8, lag_tol: int = 1,
                       max_gap: int = 1, min_pairs: int = 100, max_run: int = 64, ctx=None, hop: int = None) -> list:
    """find_shared for callers who hold fingerprints: key32 / t1 the hashes of all clips (as fingerprint_batch returns them),
    hash_off their CSR over the clips, rec_clip0 the CSR of the recordings over the clips (None: every clip a recording of
    its own).  Fs and hop (None: the context's) are what the hashes' frames were counted at.  A call carries the hashes of the
    recordings its jobs name, gathered on the host."""
    from . import get_context
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP)) if hop is None else int(hop)
    hash_off = np.ascontiguousarray(hash_off, np.uint64)
    rec_clip0 = np.arange(len(hash_off), dtype=np.uint32) if rec_clip0 is None else np.ascontiguousarray(rec_clip0, np.uint32)
    pairs = _check_pairs(pairs, len(rec_clip0) - 1)
    lo, hi = _lag_window(min_lag_seconds, max_lag_seconds, int(Fs), hop)
    key32, t1 = np.asarray(key32, np.uint32), np.asarray(t1, np.uint32)
    out = []
    for job0, jobs, recs in _plan_calls(pairs):
        local = {r: i for i, r in enumerate(recs)}
        ks, ts, ho, rc = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [0], [0]
        for r in recs:                                                            # the named recordings, one behind the other
            for c in range(int(rec_clip0[r]), int(rec_clip0[r + 1])):
                a, b = int(hash_off[c]), int(hash_off[c + 1])
                ks.append(key32[a:b])
                ts.append(t1[a:b])
                ho.append(ho[-1] + b - a)
            rc.append(len(ho) - 1)
        cells = ctx.shared_hashes(np.concatenate(ks), np.concatenate(ts), ho, rc, [(local[a], local[b]) for a, b in jobs], lo, hi,
                                  int(max_run), int(cell_shift), int(min_cell_pairs))
        out.extend(_shared_dicts(cells, _fold(cells, lag_tol, max_gap, min_pairs), job0, jobs, recs, int(Fs), hop))
    return out


def shared_occurrences(shared, repeats=()) -> list:
    """The airings behind shared stretches and repeats, across recordings (host only): the cross-recording form of
    occurrences().  Every shared stretch names the intervals (rec_a, first, last) and (rec_b, first + lag, last + lag); every
    repeat names (rec, first, last) and (rec, first + lag, last + lag).  Two intervals of ONE recording are the same airing
    when they overlap by at least half of the shorter one; airings joined by a shared stretch or a repeat form a group -- an
    advert aired twice on Monday and once on Tuesday comes back as one group of three airings.  shared: find_shared's dicts
    (rec_a, rec_b, first, last, lag are read); repeats: find_repeats' (rec, first, last, lag), over the same numbering of the
    recordings.  Returns a list of dicts ordered by first airing: airings (sorted (recording, first, last), each the hull of
    the intervals merged into it), shared and repeats (indices into the lists given)."""
    items, link = [], []                            # the intervals | per stretch or repeat: ("shared" / "repeats", index)
    for n, p in enumerate(shared):
        f, l, g = int(p["first"]), int(p["last"]), int(p["lag"])
        items += [(int(p["rec_a"]), f, l), (int(p["rec_b"]), f + g, l + g)]
        link.append(("shared", n))
    for n, p in enumerate(repeats):
        r, f, l, g = int(p["rec"]), int(p["first"]), int(p["last"]), int(p["lag"])
        items += [(r, f, l), (r, f + g, l + g)]
        link.append(("repeats", n))
    up = list(range(len(items)))                    # union-find over the intervals: the same airing

    def root(u, x):
        while u[x] != x:
            u[x] = u[u[x]]
            x = u[x]
        return x

    def join(u, a, b):
        a, b = root(u, a), root(u, b)
        if a != b:
            u[max(a, b)] = min(a, b)
    order = sorted(range(len(items)), key=lambda k: items[k])
    for x, a in enumerate(order):                   # intervals of one recording by start: only those that begin inside a can overlap it
        ra, sa, ea = items[a]
        for b in order[x + 1:]:
            rb, sb, eb = items[b]
            if rb != ra or sb > ea:
                break
            over = min(ea, eb) - sb + 1
            if 2 * over >= min(ea - sa + 1, eb - sb + 1):
                join(up, a, b)
    air = [root(up, k) for k in range(len(items))]
    gup = list(range(len(items)))                   # and over the airings: joined by a stretch or a repeat
    for n in range(len(link)):
        join(gup, air[2 * n], air[2 * n + 1])
    groups = {}
    for k, (r, s, e) in enumerate(items):
        g = groups.setdefault(root(gup, air[k]), {"airs": {}, "shared": set(), "repeats": set()})
        hull = g["airs"].setdefault(air[k], [r, s, e])
        hull[1], hull[2] = min(hull[1], s), max(hull[2], e)
        kind, n = link[k // 2]
        g[kind].add(n)
    out = [{"airings": sorted(tuple(h) for h in g["airs"].values()), "shared": sorted(g["shared"]), "repeats": sorted(g["repeats"])}
           for g in groups.values()]
    out.sort(key=lambda g: g["airings"][0])
    return out
