"""CPU: shz_scan_play_zones (no GPU, no ctx) against the plain-Python definition (tests/scan_play_twin.py): every clamp, two
segments of one song in one recording, one-window segments, empty zones, negative and int32-edge candidates, the unity
identity against shz_scan_zones, seeded random timelines, and every refusal with the outputs untouched."""
import numpy as np
import pytest

import scan_play_twin as PT
from shazam_amd import _ffi

FIELDS = ("lo", "hi", "wlo", "whi", "d_lo", "d_hi", "cand_n")
FILL = 77


def _seg(segs):
    names = ("rec", "sid", "first", "last", "pos_first", "pos_last", "t16")
    return {k: np.asarray([s[i] for s in segs], np.int64) for i, k in enumerate(names)}


def _check(segs, frames, window, step, margin, w, what=""):
    rc, z = _ffi.scan_play_zones_raw(_seg(segs), frames, window, step, margin, w, fill=FILL)
    assert rc == _ffi.OK, (what, rc)
    want = PT.play_zones([s + (s[6],) for s in segs], frames, window, step, margin, w)
    assert PT.refusal([s + (s[6],) for s in segs], frames, window, step, margin, w) is None, what
    got = [{k: int(z[k].reshape(-1)[i]) for k in FIELDS} for i in range(3 * len(segs))]
    assert got == want, (what, [(g, t) for g, t in zip(got, want) if g != t][:3])
    return z


def test_clamps_neighbours_and_one_window_segments():
    # song 2 twice in recording 0 with a gap below the margin, at DIFFERENT positions: a warped play has no constant shift, so
    # the two clamp each other all the same; another song between them; a one-window segment; a second recording
    segs = [(0, 2, 0, 3, -43, -8, 68289), (0, 5, 5, 7, 7, 30, 32768), (0, 2, 9, 12, 300, 340, 76548), (2, 2, 1, 1, 5, 5, 131072)]
    z = _check(segs, [400, 0, 60], 43, 11, 40, 3, "neighbours")
    assert z["lo"].tolist() == [[0, 0, 33], [15, 15, 77], [76, 76, 132], [0, 0, 11]]
    assert z["hi"].tolist() == [[99, 43, 99], [160, 98, 160], [215, 142, 215], [60, 54, 60]]
    # margins clamped at 0 and at F, margin 0, a margin far above the recording
    for margin in (0, 1, 43, 1 << 19, 0xFFFFFFFF):
        _check(segs, [400, 0, 60], 43, 11, margin, 0, ("margin", margin))
    # a one-window segment: c_a == c_b, the three candidates have one width
    z = _check([(0, 1, 4, 4, 90, 90, 60030)], [300], 108, 22, 20, 2, "one window")
    assert (z["d_hi"] - z["d_lo"]).tolist() == [[4, 4, 4]]


def test_empty_zones_and_windows_behind_the_end():
    # step > window: the last window starts behind the recording's end; zones there are empty and written as hi = lo
    segs = [(0, 1, 2, 5, 10, 100, 70000), (0, 1, 0xFFFFFFF0, 0xFFFFFFFF, 0, 0, 65536)]
    z = _check(segs, [100], 10, 30, 7, 1, "behind the end")
    assert z["lo"][1].tolist() == [100, 100, 100] and z["hi"][1].tolist() == [100, 100, 100]
    assert z["cand_n"][1].tolist() == [0, 0, 0]          # c = p - W(a S) + W(lo) lies below int32 there: no candidate
    assert z["lo"][0, 2] == 100 and z["hi"][0, 2] == 100 and z["cand_n"][0, 2] == 1   # empty, and still a candidate
    _check([(0, 1, 0, 0, 0, 0, 32768)], [0], 10, 30, 7, 0, "no frames")


def test_negative_and_int32_edge_candidates():
    top, bot = (1 << 31) - 1, -(1 << 31)
    for t16 in (32768, 65536, 131072):
        _check([(0, 1, 3, 9, -500, -100, t16)], [400], 20, 10, 15, 4, ("negative", t16))
        # the range straddles the top / the bottom of int32: clamped; wholly outside: no candidate
        z = _check([(0, 1, 0, 2, top, top - 5, t16)], [400], 20, 10, 0, 7, ("top", t16))
        assert z["cand_n"].tolist() == [[1, 1, 1]] and z["d_hi"][0, 0] == top and z["d_hi"][0, 1] == top
        # (a zone starts at or in front of its window, so c <= p: a range never lies above int32, only below)
        # with a margin the whole and the head zone start 30 frames in front of window a: c_a + w < -2^31, no candidate; the
        # tail zone starts at window b: c_b = p_b, clamped at the bottom
        z = _check([(0, 1, 5, 6, bot, bot, t16)], [400], 20, 10, 30, 7, ("bottom", t16))
        assert z["cand_n"].tolist() == [[0, 0, 1]] and z["d_lo"].tolist() == [[0, 0, bot]] and z["d_hi"].tolist() == [[0, 0, bot + 7]]
        z = _check([(0, 1, 0, 0, bot, bot, t16)], [400], 20, 10, 0, 7, ("bottom edge", t16))
        assert z["cand_n"].tolist() == [[1, 1, 1]] and z["d_lo"][0, 0] == bot and z["d_hi"][0, 0] == bot + 7
    # a drift line of exactly the largest width: 4,095 bins pass, 4,096 are refused (below)
    z = _check([(0, 1, 0, 4, 0, 40 + 4095 - 2 * 3, 65536)], [400], 20, 10, 0, 3, "width 4095")
    assert int(z["d_hi"][0, 0]) - int(z["d_lo"][0, 0]) == 4095


def test_unity_identity_against_scan_zones():
    """t16 = 65536, p_a = shift + a S, p_b = shift + b S, w = tol: the zones are shz_scan_zones' (no song has segments at two
    shifts in one recording) and every candidate is shz_scan_extents': (sid, shift + lo - tol, shift + lo + tol)."""
    W_, S_, M_, tol = 43, 11, 40, 2
    plain = [(0, 2, -43, 0, 3), (0, 5, 7, 5, 7), (0, 2, -43, 9, 12), (2, 2, 1000, 1, 2)]
    seg = {k: np.asarray([s[i] for s in plain], np.int64) for i, k in enumerate(("rec", "sid", "shift", "first", "last"))}
    lo, hi = _ffi.scan_zones(seg, [400, 0, 60], W_, S_, M_)
    z = _check([(r, sid, a, b, h + a * S_, h + b * S_, 65536) for r, sid, h, a, b in plain], [400, 0, 60], W_, S_, M_, tol, "unity")
    assert np.array_equal(z["lo"], lo) and np.array_equal(z["hi"], hi)
    assert np.array_equal(z["wlo"], lo.astype(np.uint64)) and np.array_equal(z["whi"], hi.astype(np.uint64))
    shift = np.asarray([s[2] for s in plain], np.int64)[:, None]
    assert np.array_equal(z["d_lo"], shift + lo - tol) and np.array_equal(z["d_hi"], shift + lo + tol)
    assert (z["cand_n"] == 1).all()


def test_random_timelines_against_the_twin():
    rng = np.random.default_rng(20)
    seen = {"ok": 0, "refused": 0}
    for case in range(300):
        n_recs = int(rng.integers(1, 4))
        frames = [int(rng.integers(0, 3000)) for _ in range(n_recs)]
        window, step = int(rng.integers(1, 200)), int(rng.integers(1, 120))
        segs = []
        for r in range(n_recs):
            w0 = 0
            for _ in range(int(rng.integers(0, 5))):
                a = w0 + int(rng.integers(0, 6))
                b = a + int(rng.integers(0, 8))
                w0 = b + 1
                segs.append((r, int(rng.integers(1, 3)), a, b, int(rng.integers(-3000, 3000)), int(rng.integers(-3000, 3000)),
                             int(rng.integers(32768, 131073))))
        margin, w = int(rng.integers(0, 300)), int(rng.integers(0, 40))
        if PT.refusal([x + (x[6],) for x in segs], frames, window, step, margin, w) is None:
            _check(segs, frames, window, step, margin, w, ("random", case))
            seen["ok"] += 1
        else:                                                # (a drift line of 4,096 bins or more: positions are random)
            _refused(_ffi.E_UNSUPPORTED, segs, frames, window, step, margin, w, ("random", case))
            seen["refused"] += 1
    assert seen["ok"] >= 100 and seen["refused"] >= 10, seen


def _refused(code, segs, frames, window, step, margin, w, what):
    rc, z = _ffi.scan_play_zones_raw(_seg(segs), frames, window, step, margin, w, fill=FILL)
    assert rc == code, (what, rc)
    for k in FIELDS:
        assert (z[k] == FILL).all(), (what, k)


def test_refusals_leave_the_outputs_untouched():
    ok = [(0, 1, 0, 3, 0, 33, 65536), (0, 2, 5, 6, 10, 20, 70000)]
    _check(ok, [400], 20, 10, 5, 2, "accepted")
    # what shz_scan_zones refuses
    _refused(_ffi.E_INVALID, ok, [400], 0, 10, 5, 2, "window 0")
    _refused(_ffi.E_INVALID, ok, [400], 20, 0, 5, 2, "step 0")
    _refused(_ffi.E_INVALID, ok, [1 << 32], 20, 10, 5, 2, "frames 2^32")
    _refused(_ffi.E_INVALID, [(1, 1, 0, 3, 0, 33, 65536)], [400], 20, 10, 5, 2, "rec >= n_recs")
    _refused(_ffi.E_INVALID, [(0, 1, 4, 3, 0, 33, 65536)], [400], 20, 10, 5, 2, "first > last")
    _refused(_ffi.E_INVALID, [ok[0], (0, 2, 3, 6, 10, 20, 70000)], [400], 20, 10, 5, 2, "windows not ascending")
    # a time factor outside [32768, 131072]
    for bad in (0, 32767, 131073, 0xFFFFFFFF):
        _refused(_ffi.E_INVALID, [ok[0], (0, 2, 5, 6, 10, 20, bad)], [400], 20, 10, 5, 2, ("factor", bad))
        assert PT.refusal([ok[0] + (65536,), (0, 2, 5, 6, 10, 20, bad, bad)], [400], 20, 10, 5, 2) == "invalid"
    # a zone of 2^20 warped frames: 524,288 own frames at factor 2 (one frame less passes)
    long_ = [(0, 1, 0, 0, 0, 0, 131072)]
    assert PT.refusal([long_[0] + (131072,)], [1 << 19], 1 << 19, 1, 0, 0) == "unsupported"
    _refused(_ffi.E_UNSUPPORTED, long_, [1 << 19], 1 << 19, 1, 0, 0, "zone length")
    _check(long_, [(1 << 19) - 1], 1 << 19, 1, 0, 0, "zone length below the limit")
    # a used candidate 4,096 bins wide: by the tolerance alone, and by the drift line
    flat = [(0, 1, 0, 3, 0, 30, 65536)]                  # no drift: every candidate is 2 w wide
    _refused(_ffi.E_UNSUPPORTED, flat, [400], 20, 10, 5, 2048, "w 2048")
    _check(flat, [400], 20, 10, 5, 2047, "w 2047")
    _refused(_ffi.E_UNSUPPORTED, [(0, 1, 0, 4, 0, 40 + 4096 - 2 * 3, 65536)], [400], 20, 10, 0, 3, "width 4096")
    assert PT.refusal([(0, 1, 0, 4, 0, 40 + 4096 - 2 * 3, 65536, 65536)], [400], 20, 10, 0, 3) == "unsupported"
    # an unused candidate may be as wide as it likes
    z = _check([(0, 1, 100, 200, -(1 << 31), -(1 << 31), 131072)], [400], 20, 50, 30, 0, "unused and wide")
    assert z["cand_n"].tolist() == [[0, 0, 0]]               # c_a = -2^31 - 9200, c_b = -2^31 - 19200


def test_null_arrays_and_no_segments():
    L = _ffi.lib()
    fr = np.asarray([100], np.uint64)
    assert L.shz_scan_play_zones(None, None, None, None, None, None, None, 0, _ffi.ptr(fr), 1, 10, 5, 0, 0, None, None, None, None,
                                 None, None, None) == _ffi.OK
    a = np.zeros(1, np.uint32)
    p = np.zeros(1, np.int32)
    t = np.full(1, 65536, np.uint32)
    o = [np.full(3, FILL, d) for d in (np.uint32, np.uint32, np.uint64, np.uint64, np.int32, np.int32, np.uint32)]
    args = [a, a, a, a, p, p, t]
    for miss in range(7):
        got = [None if i == miss else _ffi.ptr(x) for i, x in enumerate(args)]
        assert L.shz_scan_play_zones(*got, 1, _ffi.ptr(fr), 1, 10, 5, 0, 0, *[_ffi.ptr(x) for x in o]) == _ffi.E_INVALID, miss
    for miss in range(7):
        outs = [None if i == miss else _ffi.ptr(x) for i, x in enumerate(o)]
        assert L.shz_scan_play_zones(*[_ffi.ptr(x) for x in args], 1, _ffi.ptr(fr), 1, 10, 5, 0, 0, *outs) == _ffi.E_INVALID, miss
    assert all((x == FILL).all() for x in o)
    assert L.shz_scan_play_zones(*[_ffi.ptr(x) for x in args], 1, _ffi.ptr(fr), 1, 10, 5, 0, 0, *[_ffi.ptr(x) for x in o]) == _ffi.OK
    assert o[0].tolist() == [0, 0, 0] and o[1].tolist() == [10, 10, 10]


@pytest.mark.parametrize("t16", [32768, 54524, 65536, 76548, 131072])
def test_warped_borders_are_the_window_cut_of_the_scan(t16):
    """W(lo), W(hi) with the segment's own time factor, as shz_scan_warps cuts its windows"""
    z = _check([(0, 1, 2, 4, 0, 0, t16)], [1000], 108, 22, 30, 0, t16)
    assert z["wlo"][0].tolist() == [PT.W(14, t16), PT.W(14, t16), PT.W(88, t16)]
    assert z["whi"][0].tolist() == [PT.W(226, t16), PT.W(152, t16), PT.W(226, t16)]
