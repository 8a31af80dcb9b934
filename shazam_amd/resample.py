"""Sample-rate conversion on the GPU, so that audio at any rate meets a table built at another.

Hashes name spectrogram bins and frame distances, so the same music sampled at 48 kHz and at 44.1 kHz shares none
(DESIGN.md 3.8).  The reference has the same hole: read() hands a file's frame_rate through (__init__.py:70-113) and the
microphone is fixed at 44.1 kHz (recognizer.py:21-27).  Here the filter is designed on the host in fp64 (a Kaiser-windowed
sinc, one row of taps per phase, Q30) and applied by shz_resample_i16 (csrc/shz_resample.hip) in exact integer arithmetic:
the output is a function of the input and the taps alone, whatever the batch, the chunking or the device."""
from __future__ import annotations

import math

import numpy as np

from . import _ffi

RATE = 44100
MAX_TAPS = 4096            # SHZ_RESAMPLE_MAX_TAPS
MAX_RATIO = 1 << 24        # SHZ_RESAMPLE_MAX_RATIO
MAX_TABLE = 1 << 24        # SHZ_RESAMPLE_MAX_TABLE: L * T

_PLANS: dict = {}


def ratio(fs_in: int, fs_out: int):
    """(L, M): fs_out / fs_in = L / M in lowest terms."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in <= 0 or fs_out <= 0:
        raise ValueError("sample rates must be positive")
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def resample_plan(fs_in: int, fs_out: int, zero_crossings: int = 16, beta: float = 9.0):
    """(L, M, T, taps): taps int32 [L, T] in Q30, row p = phase p of a Kaiser-windowed sinc with cutoff 0.5 / max(L, M)
    of the rate fs_in * L, `zero_crossings` of the sinc on either side of the centre: T = 2 ceil(zero_crossings max(1, M / L))
    taps per phase.  taps[p][k] is the filter at p + (k - T / 2) L upsampled samples from its centre.  Every row is
    corrected on its largest tap to sum to exactly 2^30: a constant stays that constant.  Plans are cached."""
    L, M = ratio(fs_in, fs_out)
    key = (L, M, int(zero_crossings), float(beta))
    if key in _PLANS:
        return _PLANS[key]
    if zero_crossings < 1:
        raise ValueError("zero_crossings must be at least 1")
    T = 2 * (-(-int(zero_crossings) * max(L, M) // L))   # 2 ceil(zc max(1, M / L)), in integers
    if T > MAX_TAPS:
        raise NotImplementedError(f"{fs_in} -> {fs_out} Hz needs {T} taps per phase; the kernel takes at most {MAX_TAPS}")
    if L > MAX_RATIO or M > MAX_RATIO or L * T > MAX_TABLE:
        raise NotImplementedError(f"{fs_in} -> {fs_out} Hz needs L = {L}, M = {M} and a table of L * T = {L * T} taps; the kernel "
                                  f"takes L, M <= {MAX_RATIO} and L * T <= {MAX_TABLE}")
    D = max(L, M)
    t = (np.arange(L, dtype=np.float64)[:, None] + (np.arange(T, dtype=np.float64)[None, :] - T // 2) * L)   # [L, T]
    W = T * L / 2.0
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (t / W) ** 2, 0.0, 1.0))) / np.i0(beta)
    h = (L / D) * np.sinc(t / D) * win
    q = np.rint(h * float(1 << 30)).astype(np.int64)
    rows = np.arange(L)
    big = np.argmax(np.abs(q), axis=1)
    q[rows, big] += (1 << 30) - q.sum(axis=1)
    assert q.max() < 2 ** 31 and q.min() >= -2 ** 31
    plan = (L, M, T, np.ascontiguousarray(q.astype(np.int32)))
    plan[3].setflags(write=False)
    _PLANS[key] = plan
    return plan


def out_len(n: int, L: int, M: int) -> int:
    """ceil(n L / M): outputs of a clip of n samples."""
    return -(-int(n) * int(L) // int(M))


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from . import get_context
    return get_context()


def _pack(clips):
    from . import _as_pcm
    arrs = [_as_pcm(c) for c in clips]
    off = np.zeros(len(arrs) + 1, np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    pcm = np.concatenate(arrs) if off[-1] else np.zeros(1, np.int16)
    return pcm, off


def resample_batch(clips, fs_in: int, fs_out: int = RATE, ctx=None):
    """clips (1-D int16 arrays) at fs_in -> list of int16 arrays at fs_out.  Equal rates: copies, no filter."""
    if int(fs_in) == int(fs_out):
        from . import _as_pcm
        return [_as_pcm(c).copy() for c in clips]
    L, M, T, taps = resample_plan(fs_in, fs_out)
    pcm, off = _pack(clips)
    out, oo = _ctx(ctx).resample(pcm, off, L, M, T, taps)
    return [out[int(oo[i]):int(oo[i + 1])].copy() for i in range(len(off) - 1)]


def resample_to_device(clips, fs_in: int, fs_out: int, ctx):
    """(DevBuf, out_off) of the resampled clips: the result stays on the device for a call that takes SHZ_PCM_DEVICE.
    The caller frees the buffer."""
    L, M, T, taps = resample_plan(fs_in, fs_out)
    pcm, off = _pack(clips)
    return ctx.resample(pcm, off, L, M, T, taps, device_out=True)


class StreamResampler:
    """n_streams chunked inputs at fs_in -> fs_out.  push(chunks, end) returns one int16 array per stream: exactly the
    outputs whose newest input sample i0 has arrived (all the rest, against zeros, for streams in `end`).  Each stream
    keeps its last T input samples and its absolute position, so what a stream has emitted, concatenated, is
    resample_batch of everything it received, sample for sample, for any chunking."""

    def __init__(self, n_streams: int, fs_in: int, fs_out: int = RATE, ctx=None):
        self.ctx, self.n = _ctx(ctx), int(n_streams)
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.copy = self.fs_in == self.fs_out
        if not self.copy:
            self.L, self.M, self.T, self.taps = resample_plan(fs_in, fs_out)
        self.reset()

    def reset(self, which=None):
        if which is None:
            self.tail = [np.zeros(0, np.int16) for _ in range(self.n)]
            self.pos = [0] * self.n        # input samples received
            self.emitted = [0] * self.n    # outputs emitted
            self.ended = [False] * self.n
            return
        for i in which:
            self.tail[i], self.pos[i], self.emitted[i], self.ended[i] = np.zeros(0, np.int16), 0, 0, False

    def push(self, chunks, end=None):
        from . import _as_pcm
        assert len(chunks) == self.n
        ends = set(range(self.n) if end is True else ([] if end is None else [int(i) for i in end]))
        arrs = [np.zeros(0, np.int16) if c is None else _as_pcm(c) for c in chunks]
        for i, a in enumerate(arrs):
            if self.ended[i] and (len(a) or i in ends):
                raise ValueError(f"stream {i} has ended")
        if self.copy:
            for i in ends:
                self.ended[i] = True
            return [a.copy() for a in arrs]
        L, M, T = self.L, self.M, self.T
        bufs, base, first, last = [], [], [], []
        for i, a in enumerate(arrs):
            buf = np.concatenate([self.tail[i], a])
            pos = self.pos[i] + len(a)
            # output m is ready once sample i0 = (m M) div L + T / 2 is there: (m M) div L <= pos - 1 - T / 2
            ready = out_len(pos, L, M) if i in ends else (out_len(pos - T // 2, L, M) if pos > T // 2 else 0)
            ready = max(ready, self.emitted[i])
            bufs.append(buf)
            base.append(pos - len(buf))
            first.append(self.emitted[i])
            last.append(ready)
            self.pos[i], self.tail[i] = pos, buf[-T:].copy() if len(buf) > T else buf
        pcm, off = _pack(bufs)
        out, oo = self.ctx.resample(pcm, off, L, M, T, self.taps, in_base=base, m_first=first, m_end=last)
        for i in range(self.n):
            self.emitted[i] = last[i]
            if i in ends:
                self.ended[i] = True
        return [out[int(oo[i]):int(oo[i + 1])].copy() for i in range(self.n)]
