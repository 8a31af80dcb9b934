"""Live streams: fingerprint and recognise audio that arrives chunk by chunk.

The reference's recogniser reads the microphone in CHUNK = 8192-sample pieces per channel, fingerprints the channels,
unions their hashes, matches and aligns (recognizer.py:21-25, 357-392).  Here many such sources advance at once on the
GPU (shz_streams_*, csrc/shz_stream.hip): a push settles what the new samples complete and returns the hashes that became
final, so that what a stream has emitted is always a prefix of fingerprint() of everything it received, in the
reference's generation order."""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._ffi import HOP

RATE = 44100
TOPN = 2


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from . import get_context
    return get_context()


class StreamFingerprinter:
    """n_streams independent streams on one context.  push(chunks, end) -> (key32, t1, hash_off): the hashes that became
    final, stream i's at [hash_off[i], hash_off[i+1]), t1 in frames from the stream's first sample.  The hop is the
    context's at creation (Context.set_overlap before creating for another wratio)."""

    def __init__(self, n_streams: int, Fs: int = RATE, fan_value: int = 5, amp_min=10, ctx=None, fs_in: int = None):
        self.ctx = _ctx(ctx)
        self.n_streams = int(n_streams)
        self.streams = _ffi.Streams(self.ctx, self.n_streams, int(Fs), float(amp_min), int(fan_value))
        self.resampler = None   # fs_in: the chunks arrive at fs_in and are resampled to Fs in front of push
        if fs_in is not None and int(fs_in) != int(Fs):
            from .resample import StreamResampler
            self.resampler = StreamResampler(self.n_streams, int(fs_in), int(Fs), self.ctx)

    def _pcm(self, chunks, end):
        """The chunks as the streams take them: int16, at the streams' rate."""
        if self.resampler is not None:
            return self.resampler.push(chunks, end)
        return [None if c is None else _as_pcm(c) for c in chunks]

    def push(self, chunks, end=None):
        return self.streams.push(self._pcm(chunks, end), end)

    def push_hex(self, chunks, end=None):
        """push() with the reference's return type: per stream list[(hex20, t1)]."""
        from . import hex_of_keys
        k, t1, ho = self.push(chunks, end)
        hexes = hex_of_keys(self.ctx, k) if len(k) else []
        t = t1.tolist()
        return [list(zip(hexes[ho[i]:ho[i + 1]], t[ho[i]:ho[i + 1]])) for i in range(self.n_streams)]

    def reset(self, which=None):
        self.streams.reset(which)
        if self.resampler is not None:
            self.resampler.reset(which)

    def state(self, i: int) -> dict:
        """samples received, settled frames, peaks pending, hashes emitted so far."""
        return self.streams.state(i)

    def close(self):
        self.streams.close()


def _as_pcm(x):
    from . import _as_pcm as conv
    return conv(x)


def _q16(a) -> np.ndarray:
    """Q16 factors of a list given as Q16 integers or as floats"""
    a = np.ascontiguousarray(a)
    if a.ndim != 1 or a.dtype.kind not in "iuf":
        raise TypeError("a ladder is a 1-D list of Q16 integers (round(s * 65536)) or of floats")
    return (np.rint(a * 65536.0) if a.dtype.kind == "f" else a).astype(np.uint32)


def _ladder_of(speeds, warps):
    """("speed", s16, s16) or ("warp", t16, f16).  warps: a list of (tempo, pitch) pairs, or the tuple of two arrays
    (tempos, pitches) that recognize_warps takes."""
    if speeds is not None:
        s = _q16(speeds)
        return "speed", s, s
    if isinstance(warps, tuple) and len(warps) == 2 and all(isinstance(x, np.ndarray) and x.ndim == 1 for x in warps):
        t16, f16 = _q16(warps[0]), _q16(warps[1])   # (a tuple of two arrays: the two lists; anything else: pairs)
    else:
        w = np.asarray(warps)
        if w.ndim != 2 or w.shape[1] != 2:
            raise ValueError("warps is a list of (tempo, pitch) pairs, or the two lists (tempos, pitches)")
        t16, f16 = _q16(np.ascontiguousarray(w[:, 0])), _q16(np.ascontiguousarray(w[:, 1]))
    if len(t16) != len(f16):
        raise ValueError("warps=(tempos, pitches): two lists of one length")
    return "warp", t16, f16


def fingerprint_stream(chunks, Fs: int = RATE, fan_value: int = 5, amp_min=10, ctx=None):
    """Generator: yields list[(hex20, t1)] per chunk of `chunks` (any iterable of 1-D int16 arrays); the stream ends with
    the last chunk.  The concatenation of what it yields equals fingerprint(np.concatenate(chunks))."""
    fp = StreamFingerprinter(1, Fs, fan_value, amp_min, ctx)
    try:
        it = iter(chunks)
        try:
            cur = next(it)
        except StopIteration:
            return
        while True:
            try:
                nxt = next(it)
            except StopIteration:
                yield fp.push_hex([cur], end=[0])[0]
                return
            yield fp.push_hex([cur])[0]
            cur = nxt
    finally:
        fp.close()


class StreamRecognizer:
    """n_listeners live listeners against a HipFingerprintDB.  A listener is `channels` streams whose hashes are unioned
    (recognizer.py:377-382).  push(chunks_per_listener) returns per listener (results, w0): the reference-shaped result
    dicts of align_matches over the settled hashes with t1 >= w0 = max(0, H - window_frames), query offsets t1 - w0, for
    all listeners in ONE batched match -- `offset` means what it means for a clip recorded from frame w0.  H is the
    smallest settled horizon of the listener's channels; window_frames = int(window_seconds * 44100 / hop).  Listeners
    with no hashes in the window get [].  device=True keeps the windows on the GPU (shz_listeners_*): one library call per
    push, no hash crosses the bus, same return value.  fs_in: the listeners' audio is at fs_in and the table at 44.1 kHz; the
    chunks go through a StreamResampler first.

    speeds= / warps= (device=True only): listeners whose audio may play fast or slow.  speeds is a ladder as recognize_speeds
    takes it (Q16 integers, or floats), warps a list of (tempo, pitch) pairs or the two Q16 arrays as recognize_warps takes
    them.  The windows then hold settled PEAKS (shz_listeners_create_peaks); every push warps, pairs and matches every
    listener's window at every variant, and each result dict carries "speed", or "tempo" and "pitch", of the listener's
    best variant; `offset` is in the TABLE's frames.  last_best / last_profile hold the arrays of the last push;
    push(..., speeds=) / push(..., warps=) overrides the ladder for that push.  At a ladder of [65536] the results are those
    of the window's peaks paired among themselves, not bit for bit the plain listener's.

    delta_tol: the vote tolerance in offset bins of this recogniser's matches, held for its lifetime and set around every push
    (Context.tolerance); None: whatever the context holds at the push.

    songs= / exclude= (song ids; at most one of them): this recogniser's listeners are matched within / without these songs.
    The lists are held for its lifetime and every push runs inside Context.songs() -- host and device=True alike, a ladder
    included; both None: whatever filter the context holds at the push.  The unsharded table only.

    The key cap is taken from the context at the push: run push() inside `with ctx.key_cap(rows):` (Context.key_cap)."""

    def __init__(self, db, n_listeners: int, channels: int = 1, window_seconds: float = 5, topn: int = TOPN,
                 fan_value: int = 5, amp_min=10, device: bool = False, fs_in: int = None, speeds=None, warps=None,
                 delta_tol: int = None, songs=None, exclude=None):
        if speeds is not None and warps is not None:
            raise ValueError("speeds= and warps= exclude each other: a speed is the warp (s, s)")
        if (speeds is not None or warps is not None) and not device:
            raise ValueError("speeds= / warps= need device=True: the host recogniser keeps hashes, and a warp acts on peaks")
        self.ladder = None if speeds is None and warps is None else _ladder_of(speeds, warps)
        self.last_best = self.last_profile = None
        self.delta_tol = None if delta_tol is None else int(delta_tol)
        if songs is not None and exclude is not None:
            raise ValueError("songs= and exclude= exclude each other")
        if (songs is not None or exclude is not None) and not hasattr(db.table, "h"):
            raise NotImplementedError("songs= / exclude= take the unsharded table (shards=1)")
        self.songs = None if songs is None else _ffi._song_ids(songs)
        self.exclude = None if exclude is None else _ffi._song_ids(exclude)
        self.db, self.n, self.channels, self.topn = db, int(n_listeners), int(channels), int(topn)
        self.fp = StreamFingerprinter(self.n * self.channels, RATE, fan_value, amp_min, db.ctx, fs_in)
        self.window_frames = int(float(window_seconds) * RATE / self.fp.streams.hop)
        self._k = [np.zeros(0, np.uint32) for _ in range(self.n)]
        self._t = [np.zeros(0, np.uint32) for _ in range(self.n)]
        self.listeners = None
        if device:
            if not hasattr(db.table, "h"):
                raise NotImplementedError("device-resident listeners take the unsharded table (shards=1)")
            self.listeners = _ffi.Listeners(self.fp.streams, db.table, self.n, self.window_frames, peaks=self.ladder is not None)

    def _flat(self, per_listener):
        out = []
        for lc in per_listener:
            if self.channels == 1 and (lc is None or (isinstance(lc, np.ndarray) and lc.ndim == 1)):
                lc = [lc]
            if lc is None:
                lc = [None] * self.channels
            assert len(lc) == self.channels, "one chunk per channel"
            out.extend(lc)
        return out

    def horizon(self, listener: int) -> int:
        c = self.channels
        return min(self.fp.state(listener * c + j)["settled"] for j in range(c))

    def push(self, chunks_per_listener, end=None, speeds=None, warps=None):
        """chunks_per_listener[l]: list of `channels` 1-D int16 arrays (a bare array when channels == 1; None: nothing).
        end: listeners whose channels all end after this chunk.  Returns [(results, w0)] per listener.  speeds / warps:
        this push's ladder, for a recogniser created with one."""
        with self.db.ctx.tolerance(self.delta_tol), self.db.ctx.songs(only=self.songs, exclude=self.exclude):
            return self._push(chunks_per_listener, end, speeds, warps)

    def _push(self, chunks_per_listener, end, speeds, warps):
        assert len(chunks_per_listener) == self.n
        if speeds is not None and warps is not None:
            raise ValueError("speeds= and warps= exclude each other: a speed is the warp (s, s)")
        if (speeds is not None or warps is not None) and self.ladder is None:
            raise ValueError("a ladder for one push needs a recogniser created with speeds= or warps=")
        ends = None if end is None else [l * self.channels + j for l in (range(self.n) if end is True else end)
                                         for j in range(self.channels)]
        if self.ladder is not None:
            ladder = self.ladder if speeds is None and warps is None else _ladder_of(speeds, warps)
            return self._push_ladder(self._flat(chunks_per_listener), ends, ladder)
        if self.listeners is not None:
            return self._push_device(self._flat(chunks_per_listener), ends)
        k, t1, ho = self.fp.push(self._flat(chunks_per_listener), ends)
        keys, qoffs, qoff, w0s = [], [], [0], []
        for l in range(self.n):
            s0, s1 = int(ho[l * self.channels]), int(ho[(l + 1) * self.channels])
            H = self.horizon(l)
            w0 = max(0, H - self.window_frames)
            kk = np.concatenate([self._k[l], k[s0:s1]])
            tt = np.concatenate([self._t[l], t1[s0:s1]])
            keep = tt >= w0
            self._k[l], self._t[l] = kk[keep], tt[keep]
            keys.append(self._k[l])
            qoffs.append((self._t[l] - np.uint32(w0)).astype(np.uint32))
            qoff.append(qoff[-1] + len(self._k[l]))
            w0s.append(w0)
        results = [[] for _ in range(self.n)]
        live = [l for l in range(self.n) if qoff[l + 1] > qoff[l]]
        if live:
            from . import _result_dicts
            qo = np.zeros(len(live) + 1, np.uint64)
            qo[1:] = np.cumsum([qoff[l + 1] - qoff[l] for l in live])
            res = self.db.match(np.concatenate([keys[l] for l in live]), np.concatenate([qoffs[l] for l in live]), qo,
                                self.topn)
            for q, l in enumerate(live):
                results[l] = _result_dicts(self.db, res, q, int(res["nhash"][q]))
        return list(zip(results, w0s))

    def _push_device(self, chunks, ends):
        from . import _result_dicts
        self.db.finalize()
        res, w0 = self.listeners.push(self.fp._pcm(chunks, ends), ends, self.topn)
        nhash = res["nhash"].tolist()
        return [(_result_dicts(self.db, res, l, nhash[l]) if nhash[l] else [], int(w0[l])) for l in range(self.n)]

    def _push_ladder(self, chunks, ends, ladder):
        from . import _result_dicts
        self.db.finalize()
        kind, t16, f16 = ladder
        pcm = self.fp._pcm(chunks, ends)
        if kind == "speed":
            res, w0 = self.listeners.push_speeds(pcm, t16, ends, self.topn)
        else:
            res, w0 = self.listeners.push_warps(pcm, t16, f16, ends, self.topn)
        self.last_best, self.last_profile = res["best"], res["profile"]
        nhash, out = res["nhash"].tolist(), []
        for l in range(self.n):
            dicts = _result_dicts(self.db, res, l, nhash[l]) if nhash[l] else []
            b = int(res["best"][l])
            for d in dicts:
                if kind == "speed":
                    d["speed"] = float(t16[b]) / 65536
                else:
                    d["tempo"], d["pitch"] = float(t16[b]) / 65536, float(f16[b]) / 65536
            out.append((dicts, int(w0[l])))
        return out

    def window_hashes(self, listener: int) -> int:
        """Hashes in the listener's window after the last push (with a ladder: the hashes of its chosen variant)."""
        if self.listeners is not None:
            return self.listeners.state(listener)["window_hashes"]
        return len(self._k[listener])

    def reset(self, listeners=None):
        ls = range(self.n) if listeners is None else list(listeners)
        if self.listeners is not None:
            self.listeners.reset(ls)
            if self.fp.resampler is not None:
                self.fp.resampler.reset([l * self.channels + j for l in ls for j in range(self.channels)])
            return
        self.fp.reset([l * self.channels + j for l in ls for j in range(self.channels)])
        for l in ls:
            self._k[l] = np.zeros(0, np.uint32)
            self._t[l] = np.zeros(0, np.uint32)

    def close(self):
        if self.listeners is not None:
            self.listeners.close()
        self.fp.close()
