"""GPU: the CONTENT of the listeners' peak windows (window_count_kernel / window_write_kernel in csrc/shz_stream.hip), read
back through Listeners.peaks after every push and compared entry for entry and in order with the numpy twin
(tests/listen_speed_twin.py): the oracle's peaks of every channel's whole signal with w0 <= t < H_c.  The match cannot show
a compaction that duplicates one peak and drops another, or misplaces peaks at a wave or round border.

2 listeners x 2 channels over the streams of listen_speed_cases.  The sizes the kernels met per push and stream are taken
from the twin alone (old_n: its window before the push; new_n: the peaks the push settled; kept_old: old peaks with
t >= w0) and the last test asserts that the schedules together reached every class that matters to the kernels."""
import ctypes as C

import numpy as np
import pytest

import listen_speed_cases as CS
import listen_speed_twin as LT

pytestmark = pytest.mark.gpu

ROUND = 256
N, CH = 2, 2


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    ctx = S.get_context(0)
    sg = CS.songs()
    db, _ = CS.build_db(S, ctx, sg)
    sig = CS.streams(sg)
    lad = np.asarray([65536, int(CS.ladder()[-2])], np.uint32)      # the windows do not depend on the ladder: a short one
    yield {"S": S, "ctx": ctx, "db": db, "sig": sig, "peaks": [CS.oracle_peaks(x) for x in sig], "lad": lad, "sizes": [], "done": {}}
    db.close()


class _Run:
    """one Streams + peak-window Listeners and the twin's view of them"""

    def __init__(self, e, signals=None, peaks=None):
        from shazam_amd import _ffi
        self.e, self.ffi = e, _ffi
        self.sig = list(e["sig"] if signals is None else signals)
        self.peaks = list(e["peaks"] if peaks is None else peaks)
        self.feed = CS.Feed(self.sig)
        self.streams = _ffi.Streams(e["ctx"], N * CH)
        self.L = _ffi.Listeners(self.streams, e["db"].table, N, CS.WINDOW_FRAMES, peaks=True)
        self.win = [(np.zeros(0, np.uint16), np.zeros(0, np.uint32)) for _ in range(N * CH)]
        self.h_prev = [0] * (N * CH)

    def push(self, sizes, end=()):
        chunks, ends = self.feed.take(sizes, end)
        for i in ends or ():                       # a stream that ends early: the oracle's peaks of what it received
            if self.feed.pos[i] < len(self.sig[i]):
                self.peaks[i] = CS.oracle_peaks(self.sig[i][:self.feed.pos[i]])
        res, w0s = self.L.push_speeds(chunks, self.e["lad"], ends, CS.TOPN)
        hs = self.feed.horizons()
        for i in range(N * CH):
            assert self.streams.state(i)["settled"] == hs[i], ("settled", i)
        for l in range(N):
            h = hs[l * CH:(l + 1) * CH]
            w0, win = LT.window(self.peaks[l * CH:(l + 1) * CH], h, CS.WINDOW_FRAMES)
            assert int(w0s[l]) == w0 == self.ffi.listener_window(h, CS.WINDOW_FRAMES)[1], ("w0", l)
            assert self.L.state(l)["w0"] == w0
            assert self.L.state(l)["window_hashes"] == int(res["nhash"][l])
            for c in range(CH):
                i = l * CH + c
                f, t = self.L.peaks(l, c)
                assert f.dtype == np.uint16 and t.dtype == np.uint32
                assert len(f) == len(win[c][0]), ("window peaks", l, c, len(f), len(win[c][0]))
                assert np.array_equal(t, win[c][1]), ("t", l, c, int(np.flatnonzero(t != win[c][1])[0]))
                assert np.array_equal(f, win[c][0]), ("f", l, c, int(np.flatnonzero(f != win[c][0])[0]))
                pt = self.peaks[i][1]
                new_n = int(np.count_nonzero((pt >= self.h_prev[i]) & (pt < hs[i])))
                old_n, kept_old = len(self.win[i][1]), int(np.count_nonzero(self.win[i][1] >= w0))
                assert kept_old + (new_n if self.h_prev[i] >= w0 else 0) <= len(f) <= old_n + new_n
                self.e["sizes"].append((old_n, new_n, kept_old, w0))
                self.win[i], self.h_prev[i] = win[c], hs[i]
        return res

    def reset(self, listeners):
        self.L.reset(listeners)
        which = [l * CH + c for l in listeners for c in range(CH)]
        self.feed.reset(which)
        for i in which:
            self.win[i], self.h_prev[i] = (np.zeros(0, np.uint16), np.zeros(0, np.uint32)), 0
            self.peaks[i] = self.e["peaks"][i]

    def close(self):
        self.L.close()
        self.streams.close()


# ---- the schedules (each runs once per module: the tests below and the coverage test share them) ---------------------------

def _even(e):
    """8192 samples a push throughout; every stream ends with its last chunk and is matched once more"""
    r = _Run(e)
    n = len(r.sig[0])
    for a in range(0, n, CS.CHUNK):
        r.push([CS.CHUNK] * 4, end=range(4) if a + CS.CHUNK >= n else ())
    r.push([None] * 4)
    r.close()


def _irregular(e):
    """5000, 12345, 0, 30000, ... and one chunk longer than the window (250,000 samples: 122 frames), which keeps nothing old;
    the second listener's streams run through the same sizes three places on"""
    r = _Run(e)
    sizes = [5000, 12345, 0, 30000, 1, 4097, CS.CHUNK, 100, 3 * CS.CHUNK + 17, 2048, 250000, 4095, 60000, 7]
    for p in range(2 * len(sizes)):
        a, b = sizes[p % len(sizes)], sizes[(p + 3) % len(sizes)]
        r.push([a, a, b, b])
    r.close()


def _one_channel_ahead(e):
    """channel 0 of listener 0 is fed four chunks before channel 1 starts and stays ahead: it keeps its peaks beyond H"""
    r = _Run(e)
    for p in range(40):
        r.push([CS.CHUNK, CS.CHUNK if p >= 4 else None, CS.CHUNK, None if p % 3 == 0 else CS.CHUNK])
    ahead = r.feed.horizons()
    assert ahead[0] - ahead[1] >= 3 * CS.CHUNK // 2048
    f, t = r.L.peaks(0, 0)
    assert len(t) and int(t.max()) >= min(ahead[:2])                  # peaks at and beyond H = the slower channel's horizon
    r.close()


def _early_end(e):
    """listener 1 ends after 21 chunks (its last window holds the stream's true right edge); it keeps its window and is
    matched again while listener 0 goes on and its own window moves"""
    r = _Run(e)
    for p in range(34):
        res = r.push([CS.CHUNK] * 4, end=(2, 3) if p == 20 else ())
        if p == 20:
            kept = [r.L.peaks(1, c) for c in range(CH)]
            top = (int(res["sid"][1, 0]), int(res["delta"][1, 0]), int(res["aligned"][1, 0]))
        if p > 20:
            for c in range(CH):
                f, t = r.L.peaks(1, c)
                assert np.array_equal(f, kept[c][0]) and np.array_equal(t, kept[c][1])
            assert (int(res["sid"][1, 0]), int(res["delta"][1, 0]), int(res["aligned"][1, 0])) == top
    r.close()


def _reset_in_the_middle(e):
    """listener 0 starts afresh after 30 pushes: its windows are empty, listener 1's are untouched, and it fills again"""
    r = _Run(e)
    for p in range(44):
        r.push([CS.CHUNK] * 4)
        if p == 30:
            before = [r.L.peaks(1, c) for c in range(CH)]
            r.reset([0])
            for c in range(CH):
                f, t = r.L.peaks(0, c)
                assert len(f) == len(t) == 0
                f, t = r.L.peaks(1, c)
                assert np.array_equal(f, before[c][0]) and np.array_equal(t, before[c][1])
            assert r.L.state(0) == {"window_hashes": 0, "w0": 0}
    r.close()


def _dense(e):
    """a click per hop (synth-free, far more peaks a frame than music) beside a synth_clip: totals of many 256-entry rounds"""
    from oracle import synth
    dense = np.zeros(2048 * 60, np.int16)
    dense[1024::2048] = 20000
    tone = synth.synth_clip(11, 2, len(dense), 4000, 1500)
    sig = [dense, tone, tone, dense]
    r = _Run(e, sig, [CS.oracle_peaks(x) for x in sig])
    for a in range(0, len(dense), CS.CHUNK):
        r.push([CS.CHUNK] * 4, end=range(4) if a + CS.CHUNK >= len(dense) else ())
    r.close()


SCHEDULES = {"even": _even, "irregular": _irregular, "ahead": _one_channel_ahead, "end": _early_end, "reset": _reset_in_the_middle,
             "dense": _dense}


def _ensure(e, name):
    """run a schedule once; a failure is kept and raised again for whoever asks next"""
    done = e["done"]
    if name not in done:
        try:
            SCHEDULES[name](e)
            done[name] = None
        except BaseException as err:
            done[name] = err
            raise
    elif done[name] is not None:
        raise done[name]


@pytest.mark.parametrize("name", ["even", "irregular", "ahead", "end", "reset", "dense"])
def test_windows_equal_the_twin_after_every_push(env, name):
    _ensure(env, name)


def test_the_entry_refuses_what_it_documents(env):
    from shazam_amd import _ffi
    r = _Run(env)
    for _ in range(16):
        r.push([CS.CHUNK] * 4)
    L, cnt = _ffi.lib(), C.c_uint64(0)
    assert L.shz_listeners_peaks(r.L.h, N, 0, None, None, 0, C.byref(cnt)) == _ffi.E_INVALID
    assert L.shz_listeners_peaks(r.L.h, 0, CH, None, None, 0, C.byref(cnt)) == _ffi.E_INVALID
    assert L.shz_listeners_peaks(r.L.h, 0, 0, None, None, 0, None) == _ffi.E_INVALID
    f, t = r.L.peaks(1, 1)
    assert len(f) > 1
    bf, bt = np.full(len(f), 0xABCD, np.uint16), np.full(len(f), 0xABCDEF01, np.uint32)
    assert L.shz_listeners_peaks(r.L.h, 1, 1, _ffi.ptr(bf), _ffi.ptr(bt), len(f) - 1, C.byref(cnt)) == _ffi.E_CAPACITY
    assert cnt.value == len(f) and (bf == 0xABCD).all() and (bt == 0xABCDEF01).all()      # nothing was copied
    r.push([None] * 4)                                                                    # and no state changed
    r.close()


def test_the_schedules_reached_every_class_of_sizes(env):
    """from the twin's sizes alone"""
    for name in SCHEDULES:
        _ensure(env, name)
    sizes = env["sizes"]
    n_in = [o + n for o, n, _, _ in sizes]
    print("pushes x streams:", len(sizes), "| largest total:", max(n_in),
          "| nothing old kept:", sum(1 for o, n, ko, _ in sizes if o > 0 and ko == 0 and n > 0),
          "| everything kept:", sum(1 for o, n, ko, w in sizes if o > 0 and ko == o and w == 0 and n > 0),
          "| old ends inside a wave:", sum(1 for o, n, _, _ in sizes if o % 64 and n),
          "| totals <= 256 / > 256 / > 64 rounds:", sum(1 for x in n_in if 0 < x <= ROUND), sum(1 for x in n_in if x > ROUND),
          sum(1 for x in n_in if x > 64 * ROUND))
    # a push that keeps nothing old (one chunk longer than the window) while new peaks arrive
    assert any(o > 0 and ko == 0 and n > 0 for o, n, ko, _ in sizes)
    # one that keeps everything: w0 = 0
    assert any(o > 0 and ko == o and w == 0 and n > 0 for o, n, ko, w in sizes)
    # the usual case: part of the old peaks expires
    assert any(0 < ko < o for o, _, ko, _ in sizes)
    # the old part ends inside a wave and new peaks follow it in the same wave
    assert any(o % 64 != 0 and n > 0 for o, n, _, _ in sizes)
    # totals on both sides of the 256-entry round: within one wave, one round, two rounds, many
    assert any(0 < x < 64 for x in n_in) and any(64 < x <= ROUND for x in n_in)
    assert any(ROUND < x <= 2 * ROUND for x in n_in) and any(x > 2 * ROUND for x in n_in)
    # nothing old, nothing new, neither
    assert any(o == 0 and n > 0 for o, n, _, _ in sizes) and any(o > 0 and n == 0 for o, n, _, _ in sizes)
    assert any(o == 0 and n == 0 for o, n, _, _ in sizes)
