"""GPU: shz_warp_pair_hash_tf equals the numpy statement of the two-factor warp (tests/warp_twin.py) bit for bit -- keys,
anchor times and the CSR, in the order query, warp, clip.  The warps are every pair of {32768, 62259, 65536, 68813, 131072}:
all four quadrants, both extremes of each axis, the diagonal.  The peak lists are built for what the second factor adds to
the order argument: bins that fold into one f' inside a frame and ACROSS two frames that share a t' (the
tie rule "earlier index first" in the quadrant t16 < 65536 < f16, with neighbouring bins in one f' at 131072), three consecutive
frames of which two merge, bins at and around 2048 that leave only for f16 < 65536, a clip that loses all its peaks, empty
and one-peak clips, a two-channel query between one-channel queries, and ~1,500 real peaks of a note clip.  Also 1 and
1,024 warps a call, device lists in and out, and the diagonal against shz_warp_pair_hash itself."""
import itertools

import numpy as np
import pytest

import warp_twin as W

pytestmark = pytest.mark.gpu

AXIS = [32768, 62259, 65536, 68813, 131072]
TEMPO = [t for t, _ in itertools.product(AXIS, AXIS)]      # 25 warps, tempo-major; pair 6 k is the diagonal
PITCH = [f for _, f in itertools.product(AXIS, AXIS)]
FANS = [1, 2, 5, 64]


@pytest.fixture(scope="module")
def ctx():
    import shazam_amd
    return shazam_amd.get_context(0)


def _frames(spec):
    """[(frame, [bins])] -> (f, t) in (t asc, f asc) order"""
    f, t = [], []
    for fr, bins in spec:
        f.extend(sorted(bins))
        t.extend([fr] * len(bins))
    return f, t


def _clips():
    """(name, f, t) of every built clip.  Frames 1, 2 share t' = 1 at 32768 and frames 9, 10 share t' = 9 at 62259."""
    out = [("empty", [], []), ("one peak", [700], [3])]
    out.append(("adjacent",) + _frames([(0, [100, 101, 102, 103, 500, 501]), (4, [7, 8, 9, 1000, 1001, 1002, 1003]), (5, [64, 65])]))
    out.append(("two frames",) + _frames([(1, [100, 101, 300, 302, 303]), (2, [100, 101, 102, 301, 302]),
                                          (9, [400, 401, 900]), (10, [399, 400, 401, 402, 901]), (40, [5])]))
    out.append(("three frames",) + _frames([(1, [200, 201, 600]), (2, [200, 201, 202, 601]), (3, [199, 200, 201, 600]),
                                            (8, [50, 51]), (9, [50, 51]), (10, [50, 51]), (11, [49, 52])]))
    out.append(("edge",) + _frames([(2, [5, 1023, 1024, 1025, 1945, 1946, 1947, 2046, 2047, 2048]), (3, [1024, 1946, 2048]),
                                    (4, [1025, 1947, 2047])]))
    out.append(("all leave",) + _frames([(1, [2000, 2040, 2048]), (2, [1947, 1999]), (7, [2048])]))
    return out


def _pack(clips):
    pf = np.asarray([x for _, f, _ in clips for x in f], np.uint16)
    pt = np.asarray([x for _, _, t in clips for x in t], np.uint32)
    po = np.zeros(len(clips) + 1, np.uint64)
    po[1:] = np.cumsum([len(f) for _, f, _ in clips])
    return pf, pt, po


@pytest.fixture(scope="module")
def packed():
    return _pack(_clips())


@pytest.fixture(scope="module")
def real_peaks():
    """The peaks of 20 s of a note clip, as the oracle picks them"""
    from oracle import cpu_ref as O
    _, _, f, t = O.fingerprint_keys(W.notes_clip(7, 0, 20))
    assert 1000 < len(f) < 3000
    return np.asarray(f, np.uint16), np.asarray(t, np.uint32), np.asarray([0, len(f)], np.uint64)


def _assert_equal(got, want, what=""):
    (k, t1, ho), (ek, et, eho) = got, want
    assert np.array_equal(ho, eho), what
    assert np.array_equal(k, ek) and np.array_equal(t1, et), what


def test_built_cases_do_what_they_were_built_for():
    """The twin on the built clips: the cases exist in the data the GPU tests compare."""
    clips = {n: (np.asarray(f, np.int64), np.asarray(t, np.int64)) for n, f, t in _clips()}
    wf, wt = W.warp_peaks_tf(*clips["two frames"], 32768, 131072)
    # frames 1 and 2 in one t'; f' = (f + 1) >> 1 at 131072: bin 100 of BOTH frames in 50, bin 101 of both and 102 of the
    # second in 51 -- ties across the frames, by index
    assert wt[:10].tolist() == [1] * 10 and wf[:10].tolist() == [50, 50, 51, 51, 51, 150, 151, 151, 151, 152]
    wf, wt = W.warp_peaks_tf(*clips["two frames"], 62259, 68813)
    assert wt.tolist().count(9) == 8                                    # frames 9 and 10 share t' = 9
    wf, wt = W.warp_peaks_tf(*clips["three frames"], 32768, 65536)
    assert wt[:11].tolist() == [1] * 7 + [2] * 4                        # of three consecutive frames two merge
    wf, _ = W.warp_peaks_tf(*clips["edge"], 65536, 62259)
    assert wf.tolist().count(2048) == 2 and len(wf) == 9                # 1945, 1946 -> 2047, 2048 stay; 1947 and above leave
    wf, _ = W.warp_peaks_tf(*clips["edge"], 131072, 32768)
    assert wf.tolist() == [10, 2046, 2048, 2048]                        # 1023, 1024 stay, 1025 leaves
    wf, _ = W.warp_peaks_tf(*clips["edge"], 65536, 131072)
    assert len(wf) == 16 and wf.max() == 1024                           # nothing leaves above unity
    for f16 in (32768, 62259):
        assert len(W.warp_peaks_tf(*clips["all leave"], 65536, f16)[0]) == 0
    assert len(W.warp_peaks_tf(*clips["all leave"], 65536, 65536)[0]) == 6


@pytest.mark.parametrize("fan", FANS)
def test_every_clip_and_warp_equals_the_twin(ctx, packed, fan):
    pf, pt, po = packed
    nc = len(po) - 1
    got = ctx.warp_pair_hash_tf(pf, pt, po, TEMPO, PITCH, None, fan)
    _assert_equal(got, W.warp_pair_batch_tf(pf, pt, po, np.arange(nc + 1), TEMPO, PITCH, fan))
    assert len(got[2]) == nc * len(TEMPO) + 1
    if fan > 1:
        assert len(got[0]) > 0


@pytest.mark.parametrize("fan", [2, 5])
def test_a_two_channel_query_between_one_channel_queries(ctx, packed, fan):
    pf, pt, po = _pack([c for c in _clips() if c[0] in ("adjacent", "two frames", "three frames", "edge", "all leave")])
    for qc in ([0, 1, 3, 4, 5], [0, 2, 4, 5], [0, 0, 1, 5, 5], [0, 5]):
        got = ctx.warp_pair_hash_tf(pf, pt, po, TEMPO, PITCH, qc, fan)
        _assert_equal(got, W.warp_pair_batch_tf(pf, pt, po, qc, TEMPO, PITCH, fan), qc)


@pytest.mark.parametrize("fan", [2, 5, 64])
def test_real_peaks_equal_the_twin(ctx, real_peaks, fan):
    pf, pt, po = real_peaks
    got = ctx.warp_pair_hash_tf(pf, pt, po, TEMPO, PITCH, None, fan)
    _assert_equal(got, W.warp_pair_batch_tf(pf, pt, po, [0, 1], TEMPO, PITCH, fan))
    assert len(got[0]) >= len(pf)


def test_one_warp_and_1024_warps(ctx, packed):
    pf, pt, po = _pack([c for c in _clips() if c[0] in ("two frames", "three frames", "edge")])
    for t16, f16 in ((32768, 131072), (131072, 32768), (65536, 65536), (62259, 68813)):
        _assert_equal(ctx.warp_pair_hash_tf(pf, pt, po, [t16], [f16], None, 5),
                      W.warp_pair_batch_tf(pf, pt, po, [0, 1, 2, 3], [t16], [f16], 5), (t16, f16))
    rng = np.random.default_rng(1024)
    t16 = rng.integers(32768, 131073, 1024)
    f16 = rng.integers(32768, 131073, 1024)
    t16[:4], f16[:4] = [32768, 32768, 131072, 131072], [32768, 131072, 32768, 131072]
    got = ctx.warp_pair_hash_tf(pf, pt, po, t16, f16, [0, 2, 3], 3)
    _assert_equal(got, W.warp_pair_batch_tf(pf, pt, po, [0, 2, 3], t16, f16, 3))
    assert len(got[2]) == 3 * 1024 + 1


def test_the_diagonal_is_warp_pair_hash(ctx, packed, real_peaks):
    for pf, pt, po in (packed, real_peaks):
        for fan in (2, 5):
            _assert_equal(ctx.warp_pair_hash_tf(pf, pt, po, AXIS, AXIS, None, fan), ctx.warp_pair_hash(pf, pt, po, AXIS, None, fan))
    pf, pt, po = packed
    k, t1, ho = ctx.warp_pair_hash_tf(pf, pt, po, [65536], [65536], None, 5)
    _assert_equal((k, t1, ho), ctx.pair_hash(pf, pt, po, 5))


def test_device_in_device_out_equals_host(ctx, packed):
    from shazam_amd import _ffi
    pf, pt, po = packed
    k, t1, ho = ctx.warp_pair_hash_tf(pf, pt, po, TEMPO, PITCH, None, 5)
    n = len(k)
    d_f, d_t = ctx.alloc(pf.nbytes), ctx.alloc(pt.nbytes)
    d_k, d_o = ctx.alloc(n * 4), ctx.alloc(n * 4)
    try:
        d_f.upload(pf)
        d_t.upload(pt)
        # device in, host out; host in, device out; both
        rc, hk, ht, dho, cnt = ctx.warp_pair_hash_tf_raw(d_f, d_t, po, TEMPO, PITCH, None, 5, cap=n, device_in=True)
        assert rc == _ffi.OK and cnt == n and np.array_equal(dho, ho) and np.array_equal(hk, k) and np.array_equal(ht, t1)
        for dev_in in (False, True):
            d_k.upload(np.zeros(n, np.uint32))
            d_o.upload(np.zeros(n, np.uint32))
            src = (d_f, d_t) if dev_in else (pf, pt)
            rc, _, _, dho, cnt = ctx.warp_pair_hash_tf_raw(*src, po, TEMPO, PITCH, None, 5, cap=n, device_in=dev_in, out_key=d_k,
                                                           out_t1=d_o)
            assert rc == _ffi.OK and cnt == n and np.array_equal(dho, ho)
            assert np.array_equal(d_k.download(np.uint32, n), k) and np.array_equal(d_o.download(np.uint32, n), t1)
        # a capacity that is too small names the exact count and writes the CSR
        rc, _, _, cho, cnt = ctx.warp_pair_hash_tf_raw(pf, pt, po, TEMPO, PITCH, None, 5, cap=n - 1)
        assert rc == _ffi.E_CAPACITY and cnt == n and np.array_equal(cho, ho)
    finally:
        for b in (d_f, d_t, d_k, d_o):
            b.free()
