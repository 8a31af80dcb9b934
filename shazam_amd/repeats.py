"""Repeated content inside recordings, without a catalogue (csrc/shz_repeat.hip): "which stretches of this
recording air more than once?" -- an advert, a jingle, a station ident, a song nobody has inserted yet, a programme re-run.

Two hashes of one recording with the same key at times t_i < t_j vote for the lag t_j - t_i.  A stretch that airs twice piles
its votes on one lag over a contiguous stretch of t_i: the device counts the votes per CELL (lag, block of 2^cell_shift
frames), the host joins neighbouring cells into repeats (shz_repeats_fold).  A sub-frame misalignment between two airings
splits a repeat over two neighbouring lags, which is why lag_tol defaults to 1.  Every recording is fingerprinted once and its
hashes never leave the device."""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._ffi import HOP

MAX_RECS = 4096          # recordings of one library call (shz_repeats_*): more are split
MAX_LAG = (1 << 20) - 1  # the largest lag, in frames
FIRST_ROOM = 1 << 16     # cells the first call has room for (more: the call is repeated with the room it named)


def _lags(min_lag_seconds, max_lag_seconds, fs: int, hop: int):
    lo = max(1, int(round(float(min_lag_seconds) * fs / hop)))
    hi = MAX_LAG if max_lag_seconds is None else min(MAX_LAG, int(round(float(max_lag_seconds) * fs / hop)))
    if hi < lo:
        raise ValueError(f"max_lag_seconds gives {hi} frames, below min_lag_seconds' {lo}")
    return lo, hi


def _repeat_dicts(cells, rep, rec0: int, fs: int, hop: int) -> list:
    secs = lambda frames: round(float(frames) * hop / fs, 5)                      # noqa: E731
    out = []
    for i in range(len(rep["rec"])):
        r, first, last, lag = (int(rep[k][i]) for k in ("rec", "first", "last", "lag"))
        out.append({
            "recording": rec0 + r,
            "first_start_seconds": secs(first), "first_end_seconds": secs(last + 1),
            "second_start_seconds": secs(first + lag), "second_end_seconds": secs(last + lag + 1),
            "lag_seconds": secs(lag),
            "rec": rec0 + r, "first": first, "last": last, "lag": lag, "lag_lo": int(rep["lag_lo"][i]),
            "lag_hi": int(rep["lag_hi"][i]), "pairs": int(rep["pairs"][i]), "cells": int(rep["cells"][i]),
            "stats": {"hashes": int(cells["rec_hashes"][r]), "pairs": int(cells["rec_pairs"][r]),
                      "skipped_keys": int(cells["rec_skipped_keys"][r]), "skipped_rows": int(cells["rec_skipped_rows"][r])},
        })
    return out


def _fold(cells, lag_tol, max_gap, min_pairs):
    return _ffi.repeats_fold(cells["cell_off"], cells["lag"], cells["block"], cells["pairs"], cells["first"], cells["last"],
                             lag_tol, max_gap, min_pairs)


def find_repeats(recordings, Fs: int = 44100, min_lag_seconds: float = 5.0, max_lag_seconds: float = None, cell_shift: int = 5,
                 min_cell_pairs: int = 8, lag_tol: int = 1, max_gap: int = 1, min_pairs: int = 100, max_run: int = 64,
                 resample_to: int = None, ctx=None) -> list:
    """The repeats inside every recording.  recordings: 1-D int16 arrays, or lists of channels, as scan() takes them.  Two
    airings count when they lie min_lag_seconds .. max_lag_seconds apart (None: any distance the library holds, 2^20 - 1
    frames); a cell is 2^cell_shift frames of the first airing at one lag and is kept with min_cell_pairs pairs; cells at
    most lag_tol lags and max_gap + 1 blocks apart join; a repeat has min_pairs pairs.  A key that occurs more than max_run
    times in a recording is a stop hash and votes for nothing.  resample_to: the recordings are at Fs and are resampled on
    the device to that rate first (as scan(resample_to=)); frames and seconds are then counted there.
    Returns one dict per repeat, ordered by (recording, first, lag): recording, first_start_seconds / first_end_seconds (the
    earlier airing), second_start_seconds / second_end_seconds (the later one), lag_seconds; the integers rec, first, last
    (frames of the earlier airing, inclusive), lag (the lag with the most pairs), lag_lo, lag_hi, pairs, cells; and stats,
    the recording's hashes, pairs, skipped_keys and skipped_rows."""
    out = []
    for rec0, cells, rep, fs, hop in _find_raw(recordings, Fs, min_lag_seconds, max_lag_seconds, cell_shift, min_cell_pairs, lag_tol,
                                               max_gap, min_pairs, max_run, resample_to, ctx):
        out.extend(_repeat_dicts(cells, rep, rec0, fs, hop))
    return out


def _find_raw(recordings, Fs, min_lag_seconds, max_lag_seconds, cell_shift, min_cell_pairs, lag_tol, max_gap, min_pairs, max_run,
              resample_to, ctx):
    """find_repeats' library calls: per call of at most MAX_RECS recordings (first recording, cells, repeats, fs, hop) -- the
    arrays of Context.repeats_batch and of _ffi.repeats_fold as they are."""
    from . import DEFAULT_AMP_MIN, DEFAULT_FAN_VALUE, get_context, resample_to_device
    from .scan import _flatten
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP))
    recordings = list(recordings)
    out = []
    for rec0 in range(0, len(recordings), MAX_RECS):
        chans, first = _flatten(recordings[rec0:rec0 + MAX_RECS])
        fs = int(Fs)
        kw = dict(max_run=int(max_run), cell_shift=int(cell_shift), min_cell_pairs=int(min_cell_pairs),
                  amp_min=float(DEFAULT_AMP_MIN), fan_value=DEFAULT_FAN_VALUE)
        if resample_to is not None and int(resample_to) != fs:
            fs = int(resample_to)
            lo, hi = _lags(min_lag_seconds, max_lag_seconds, fs, hop)
            buf, off = resample_to_device(chans, int(Fs), fs, ctx)
            try:
                cells, _ = ctx.repeats_batch(buf, off, first, lo, hi, fs=fs, pcm_device=True, cap_cells=FIRST_ROOM, **kw)
            finally:
                buf.free()
        else:
            lo, hi = _lags(min_lag_seconds, max_lag_seconds, fs, hop)
            off = np.zeros(len(chans) + 1, np.uint64)
            if chans:
                off[1:] = np.cumsum([len(c) for c in chans])
            pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
            cells, _ = ctx.repeats_batch(pcm, off, first, lo, hi, fs=fs, cap_cells=FIRST_ROOM, **kw)
        out.append((rec0, cells, _fold(cells, lag_tol, max_gap, min_pairs), fs, hop))
    return out


def find_repeats_hashes(key32, t1, hash_off, rec_clip0=None, Fs: int = 44100, min_lag_seconds: float = 5.0,
                        max_lag_seconds: float = None, cell_shift: int = 5, min_cell_pairs: int = 8, lag_tol: int = 1,
                        max_gap: int = 1, min_pairs: int = 100, max_run: int = 64, ctx=None, hop: int = None) -> list:
    """find_repeats for callers who hold fingerprints: key32 / t1 the hashes of all clips (as fingerprint_batch returns them),
    hash_off their CSR over the clips, rec_clip0 the CSR of the recordings over the clips (None: every clip a recording of
    its own).  Fs and hop (None: the context's) are what the hashes' frames were counted at."""
    from . import get_context
    ctx = ctx or get_context()
    hop = int(getattr(ctx, "hop", HOP)) if hop is None else int(hop)
    hash_off = np.ascontiguousarray(hash_off, np.uint64)
    rec_clip0 = np.arange(len(hash_off), dtype=np.uint32) if rec_clip0 is None else np.ascontiguousarray(rec_clip0, np.uint32)
    lo, hi = _lags(min_lag_seconds, max_lag_seconds, int(Fs), hop)
    key32, t1 = np.asarray(key32), np.asarray(t1)
    out = []
    for rec0 in range(0, len(rec_clip0) - 1, MAX_RECS):
        rc = rec_clip0[rec0:rec0 + MAX_RECS + 1]
        c0, c1 = int(rc[0]), int(rc[-1])
        ho = hash_off[c0:c1 + 1]
        a, b = int(ho[0]), int(ho[-1])
        cells = ctx.repeats_hashes(key32[a:b], t1[a:b], ho - ho[0], rc - rc[0], lo, hi, int(max_run), int(cell_shift),
                                   int(min_cell_pairs))
        out.extend(_repeat_dicts(cells, _fold(cells, lag_tol, max_gap, min_pairs), rec0, int(Fs), hop))
    return out


def _airing_groups(items) -> list:
    """The grouping behind occurrences() and shared.shared_occurrences().  items[2 n] and items[2 n + 1] are the two intervals
    (recording, start, end) that link n -- a repeat, a shared stretch -- names.  Two intervals of one recording are the same
    airing when they overlap by at least half of the shorter one; airings joined by a link form a group.  Returns, in no
    order, per group (airings, links): the airings' hulls [recording, start, end] and the set of the links in it."""
    def root(u, x):
        while u[x] != x:
            u[x] = u[u[x]]
            x = u[x]
        return x

    def join(u, a, b):
        a, b = root(u, a), root(u, b)
        if a != b:
            u[max(a, b)] = min(a, b)
    up = list(range(len(items)))                    # union-find over the intervals: the same airing
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
    gup = list(range(len(items)))                   # and over the airings: joined by a link
    for n in range(len(items) // 2):
        join(gup, air[2 * n], air[2 * n + 1])
    groups = {}
    for k, (r, s, e) in enumerate(items):
        airs, links = groups.setdefault(root(gup, air[k]), ({}, set()))
        hull = airs.setdefault(air[k], [r, s, e])
        hull[1], hull[2] = min(hull[1], s), max(hull[2], e)
        links.add(k // 2)
    return [(list(airs.values()), links) for airs, links in groups.values()]


def occurrences(repeats) -> list:
    """The airings behind a list of repeats (host only).  Every repeat names two intervals of its recording, [first, last] and
    [first + lag, last + lag]; two intervals of one recording are the same airing when they overlap by at least half of the
    shorter one.  Airings joined by a repeat form a group, so an ident aired three times comes back as ONE group of three
    intervals instead of three pairwise repeats.  repeats: find_repeats' dicts (rec, first, last, lag are read).  Returns a
    list of dicts, ordered by recording and first airing: recording, intervals (the airings' (first, last) frames, each the
    hull of the intervals merged into it, ascending) and repeats (indices into the list given)."""
    items = []
    for p in repeats:
        r, f, l, g = int(p["rec"]), int(p["first"]), int(p["last"]), int(p["lag"])
        items += [(r, f, l), (r, f + g, l + g)]
    out = [{"recording": airs[0][0], "intervals": sorted((s, e) for _, s, e in airs), "repeats": sorted(links)}
           for airs, links in _airing_groups(items)]               # (a group lies in one recording: nothing here links two)
    out.sort(key=lambda g: (g["recording"], g["intervals"][0]))
    return out
