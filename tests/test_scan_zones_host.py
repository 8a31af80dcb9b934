"""CPU: shz_scan_zones -- the three zones (whole, head, tail) of every timeline segment, host only -- against the plain-Python
definition (tests/scan_extent_twin.py) on built segment lists: the clamps at 0 and at the recording's end, margins of 0 and
beyond the recording, one window, windows behind the end (empty zones), the clamp against segments of the same identity on
both sides, other songs between them, two recordings, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from scan_extent_twin import zones

E_INVALID = -1


@pytest.fixture(scope="module")
def F():
    from shazam_amd import _ffi
    _ffi.lib()
    return _ffi


def _seg(rows):
    """[(rec, sid, shift, first, last)] -> the dict of scan_timeline"""
    a = np.asarray(rows, np.int64).reshape(-1, 5)
    return {"rec": a[:, 0].astype(np.uint32), "sid": a[:, 1].astype(np.uint32), "shift": a[:, 2].astype(np.int64),
            "first": a[:, 3].astype(np.uint32), "last": a[:, 4].astype(np.uint32)}


def _check(F, rows, frames, W, S, M):
    rc, lo, hi = F.scan_zones_raw(_seg(rows), frames, W, S, M)
    assert rc == 0, (rows, frames, W, S, M)
    want = zones(rows, frames, W, S, M)
    got = list(zip(lo.reshape(-1).tolist(), hi.reshape(-1).tolist()))
    assert got == want, (rows, frames, W, S, M, got, want)
    return want


def test_clamps_at_zero_and_at_the_end(F):
    # one segment over the whole 343-frame recording: windows 0 .. 11 of 108 frames, step 22 (242 + 108 = 350 > 343)
    z = _check(F, [(0, 2, -43, 0, 11)], [343], 108, 22, 50)
    assert z == [(0, 343), (0, 108), (242, 343)]
    # inside: nothing is clamped
    z = _check(F, [(0, 2, -43, 3, 5)], [343], 108, 22, 20)
    assert z == [(46, 238), (46, 174), (110, 238)]


def test_margin_zero_and_beyond_the_recording(F):
    z = _check(F, [(0, 7, 5, 2, 4)], [343], 108, 22, 0)
    assert z == [(44, 196), (44, 152), (88, 196)]
    z = _check(F, [(0, 7, 5, 2, 4)], [343], 108, 22, 1000)
    assert z == [(0, 343), (0, 152), (88, 343)]
    _check(F, [(0, 7, 5, 2, 4)], [343], 108, 22, 0xFFFFFFFF)


def test_one_window(F):
    # W >= F: the one window is the whole recording
    z = _check(F, [(0, 1, 0, 0, 0)], [90], 108, 22, 30)
    assert z == [(0, 90), (0, 90), (0, 90)]
    _check(F, [(0, 1, 0, 0, 0)], [108], 108, 22, 0)


def test_windows_behind_the_end_are_empty(F):
    # S > W: frames 100, window 10, step 30 -> 4 windows at 0, 30, 60, 90; and a window number beyond them starts behind the end
    assert F.scan_window_count(100, 10, 30) == 4
    z = _check(F, [(0, 1, 0, 3, 3)], [100], 10, 30, 0)
    assert z == [(90, 100), (90, 100), (90, 100)]
    z = _check(F, [(0, 1, 0, 2, 5)], [100], 10, 30, 0)
    assert z == [(60, 100), (60, 70), (100, 100)]      # the tail starts at 150 > F: empty, written as hi = lo = F
    z = _check(F, [(0, 1, 0, 4, 5)], [100], 10, 30, 5)
    assert z == [(100, 100), (100, 100), (100, 100)]
    z = _check(F, [(0, 1, 0, 0, 0)], [0], 10, 30, 5)   # a recording without frames
    assert z == [(0, 0)] * 3


def test_same_identity_clamps_both_sides(F):
    W, S = 43, 11
    # two segments of (song 2, shift -43): windows 0..3 and 9..12.  The first ends at 33 + 43 = 76, the second starts at 99
    two = [(0, 2, -43, 0, 3), (0, 2, -43, 9, 12)]
    z = _check(F, two, [400], W, S, 10)        # gap 23 > M: nothing is clamped
    assert z[0] == (0, 86) and z[3] == (89, 185)
    z = _check(F, two, [400], W, S, 40)        # gap 23 < M: hi of the first stops at R = 99, lo of the second at L = 76
    assert z[0] == (0, 99) and z[2] == (33, 99) and z[3] == (76, 215) and z[4] == (76, 142)
    # segments whose windows overlap (step < window, max_gap 0): L > aS and R < bS + W -- no zone loses its own windows
    lap = [(0, 2, -43, 0, 3), (0, 2, -43, 5, 6)]
    z = _check(F, lap, [400], W, S, 40)
    assert z[0] == (0, 76) and z[3] == (55, 149)
    # three of one identity: the middle one is clamped on both sides, by its nearest neighbours
    three = [(0, 2, -43, 0, 1), (0, 2, -43, 8, 9), (0, 2, -43, 20, 22)]
    z = _check(F, three, [400], W, S, 60)
    assert z[3] == (54, 202) and z[0] == (0, 88) and z[6] == (160, 345)
    z = _check(F, three, [400], W, S, 5)
    assert z[3] == (83, 147)


def test_other_songs_and_shifts_do_not_clamp(F):
    W, S = 43, 11
    rows = [(0, 2, -43, 0, 3), (0, 5, 7, 5, 7), (0, 2, -44, 8, 8), (0, 2, -43, 9, 12), (0, 5, 7, 14, 15)]
    z = _check(F, rows, [400], W, S, 40)
    assert z[3] == (15, 154)          # song 5's first play: no neighbour in front, its second play starts at 154 < 160
    assert z[6] == (48, 171)          # shift -44 is another identity than -43: unclamped
    assert z[0] == (0, 99) and z[9] == (76, 215) and z[12] == (120, 248)


def test_two_recordings(F):
    W, S = 43, 11
    rows = [(0, 2, -43, 0, 3), (0, 2, -43, 9, 12), (2, 2, -43, 1, 2), (2, 3, 9, 4, 30)]
    z = _check(F, rows, [400, 0, 200], W, S, 40)
    assert z[6] == (0, 105)           # recording 2's segment of the same (song, shift) is not clamped by recording 0's
    assert z[9] == (4, 200) and z[11] == (200, 200)


def test_built_lists_against_the_twin(F):
    rng = np.random.default_rng(5)
    for _ in range(200):
        W, S, M = int(rng.integers(1, 60)), int(rng.integers(1, 70)), int(rng.choice([0, 1, 7, 50, 500]))
        frames = rng.integers(0, 600, 3).tolist()
        rows = []
        for r in range(3):
            w = 0
            for _ in range(int(rng.integers(0, 7))):
                a = w + int(rng.integers(0, 4))
                b = a + int(rng.integers(0, 5))
                rows.append((r, int(rng.integers(1, 3)), int(rng.integers(-2, 0)), a, b))
                w = b + 1
        _check(F, rows, frames, W, S, M)


def test_refusals(F):
    L = F.lib().shz_scan_zones
    seg = _seg([(0, 2, -43, 0, 3), (0, 2, -43, 9, 12)])
    frames = np.array([400], np.uint64)
    lo, hi = np.full(6, 77, np.uint32), np.full(6, 77, np.uint32)
    good = [seg["rec"], seg["sid"], seg["shift"], seg["first"], seg["last"], 2, frames, 1, 43, 11, 5, lo, hi]

    def call(args):
        return L(*[F.ptr(a) if isinstance(a, np.ndarray) or a is None else a for a in args])
    assert call(good) == 0 and lo[0] == 0 and hi[0] == 81
    lo[:], hi[:] = 77, 77
    for i in (0, 1, 2, 3, 4, 6, 11, 12):                       # every array NULL in turn
        assert call(good[:i] + [None] + good[i + 1:]) == E_INVALID, i
    assert call(good[:8] + [0] + good[9:]) == E_INVALID        # W = 0
    assert call(good[:9] + [0] + good[10:]) == E_INVALID       # S = 0
    assert call(good[:7] + [0] + good[8:]) == E_INVALID        # rec >= n_recs
    bad = lambda rows: call([*(_seg(rows)[k] for k in ("rec", "sid", "shift", "first", "last")), len(rows),   # noqa: E731
                             np.array([400, 400], np.uint64), 2, 43, 11, 5, lo, hi])
    assert bad([(0, 2, -43, 4, 3)]) == E_INVALID               # first > last
    assert bad([(2, 2, -43, 0, 3)]) == E_INVALID               # rec >= n_recs
    assert bad([(1, 2, -43, 0, 3), (0, 2, -43, 0, 3)]) == E_INVALID    # recordings descend
    assert bad([(0, 2, -43, 5, 6), (0, 3, 1, 0, 3)]) == E_INVALID      # windows descend inside a recording
    assert bad([(0, 2, -43, 0, 3), (0, 3, 1, 3, 4)]) == E_INVALID      # ... or share a window
    assert bad([(0, 2, -43, 0, 3), (1, 3, 1, 0, 4)]) == 0              # a new recording starts over
    lo[:], hi[:] = 77, 77
    assert call(good[:6] + [np.array([1 << 32], np.uint64)] + good[7:]) == E_INVALID   # frames beyond 32 bits
    assert (lo == 77).all() and (hi == 77).all(), "a refused call writes nothing"
    # no segment: nothing to refuse about the segment arrays
    assert L(None, None, None, None, None, C.c_uint64(0), F.ptr(frames), 1, 43, 11, 5, None, None) == 0
