"""GPU: shz_warp_pair_hash equals the numpy statement of the warp (tests/speed_twin.py) bit for bit -- keys, anchor times and
the CSR, in the order query, speed, clip -- on built peak sets: empty and one-peak clips, a tail with too few successors,
frames that merge below unity with interleaving f', peaks that leave above the last bin, a gap that passes 200 frames only
after the warp; every ladder edge and fan value; device lists equal host lists; the 65536 column is shz_pair_hash; a
capacity that is too small names the exact count; single clips whose (peak, speed) item counts sit on the route edges of the
device scan (shz_prims.hip: 2048 | 2049 items, 8192 | 8193 items) and inside its flat route."""
import functools

import numpy as np
import pytest

import speed_twin as T

pytestmark = pytest.mark.gpu

SPEEDS = [32768, 40000, 65535, 65536, 65537, 70000, 131072]
FANS = [1, 2, 5, 64]


@pytest.fixture(scope="module")
def ctx():
    import shazam_amd
    return shazam_amd.get_context(0)


def _clips():
    """(name, f, t) of every built clip."""
    rng = np.random.default_rng(42)
    out = [("empty", [], []), ("one peak", [700], [3])]
    # the last peaks have fewer than fan - 1 successors (every fan above 1: the list is short)
    out.append(("short tail", [10, 900, 40, 41, 2000], [0, 0, 1, 5, 5]))
    # adjacent frames 1, 2 -> t' = 1 at 40000 with interleaving f', equal f' across the two frames, and frame 3 alone
    out.append(("merge", [100, 300, 500, 200, 300, 400, 600, 50], [1, 1, 1, 2, 2, 2, 2, 3]))
    # 32768: f = 2048 -> 4096 leaves, 1500 -> 3000 leaves, 1024 -> 2048 stays, 1025 -> 2050 leaves; dropped peaks between kept ones
    out.append(("drop", [5, 1024, 1025, 1500, 2048, 7, 1000, 2048], [2, 2, 2, 2, 2, 3, 3, 3]))
    # dt = 150 <= 200 before the warp, 300 > 200 at 131072; and 250 -> 125 at 32768 the other way
    out.append(("gap", [11, 12, 13, 14], [0, 150, 400, 401]))
    # random material over more than one workgroup of (peak, speed) items, with frame gaps
    f, t, fr = [], [], 0
    for _ in range(160):
        fr += int(rng.choice([1, 1, 1, 2, 3]))
        n = int(rng.integers(0, 7))
        f.extend(sorted(rng.choice(2049, n, replace=False).tolist()))
        t.extend([fr] * n)
    out.append(("random", f, t))
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


@pytest.mark.parametrize("fan", FANS)
def test_every_clip_and_speed_equals_the_twin(ctx, packed, fan):
    pf, pt, po = packed
    nc = len(po) - 1
    k, t1, ho = ctx.warp_pair_hash(pf, pt, po, SPEEDS, None, fan)
    ek, et, eho = T.warp_pair_batch(pf, pt, po, np.arange(nc + 1), SPEEDS, fan)
    assert np.array_equal(ho, eho)
    assert np.array_equal(k, ek) and np.array_equal(t1, et)
    assert len(ho) == nc * len(SPEEDS) + 1
    if fan > 1:
        assert len(k) > 0


def test_built_cases_do_what_they_were_built_for():
    """The twin on the built clips: the cases exist in the data the GPU test compares."""
    clips = {n: (np.asarray(f, np.int64), np.asarray(t, np.int64)) for n, f, t in _clips()}
    wf, wt = T.warp_peaks(*clips["merge"], 40000)
    assert wt.tolist() == [1] * 7 + [2] and wf[:7].tolist() == sorted(wf[:7].tolist()) and len(set(wf[:7].tolist())) == 6
    wf, _ = T.warp_peaks(*clips["drop"], 32768)
    assert wf.tolist() == [10, 2048, 14, 2000]
    k, _ = T.warp_pair(*clips["gap"], 65536, 2)
    k2, _ = T.warp_pair(*clips["gap"], 131072, 2)
    k3, _ = T.warp_pair(*clips["gap"], 32768, 2)
    assert (len(k), len(k2), len(k3)) == (2, 1, 3)


@pytest.mark.parametrize("fan", [2, 5])
def test_three_clips_in_two_queries(ctx, packed, fan):
    pf, pt, po = _pack([c for c in _clips() if c[0] in ("merge", "drop", "random")])
    for qc in ([0, 1, 3], [0, 2, 3], [0, 0, 3, 3], [0, 3]):
        k, t1, ho = ctx.warp_pair_hash(pf, pt, po, SPEEDS, qc, fan)
        ek, et, eho = T.warp_pair_batch(pf, pt, po, qc, SPEEDS, fan)
        assert np.array_equal(ho, eho), qc
        assert np.array_equal(k, ek) and np.array_equal(t1, et), qc


def test_unity_column_is_pair_hash(ctx, packed):
    pf, pt, po = packed
    nc, K = len(po) - 1, len(SPEEDS)
    v = SPEEDS.index(65536)
    for fan in FANS:
        k, t1, ho = ctx.warp_pair_hash(pf, pt, po, SPEEDS, None, fan)
        pk, pt1, pho = ctx.pair_hash(pf, pt, po, fan)
        for c in range(nc):
            a, b = int(ho[c * K + v]), int(ho[c * K + v + 1])
            pa, pb = int(pho[c]), int(pho[c + 1])
            assert np.array_equal(k[a:b], pk[pa:pb]) and np.array_equal(t1[a:b], pt1[pa:pb]), (fan, c)
        k1, t11, ho1 = ctx.warp_pair_hash(pf, pt, po, [65536], None, fan)
        assert np.array_equal(k1, pk) and np.array_equal(t11, pt1) and np.array_equal(ho1, pho)


def test_device_in_device_out_equals_host(ctx, packed):
    from shazam_amd import _ffi
    pf, pt, po = packed
    k, t1, ho = ctx.warp_pair_hash(pf, pt, po, SPEEDS, None, 5)
    n = len(k)
    d_f, d_t = ctx.alloc(pf.nbytes), ctx.alloc(pt.nbytes)
    d_k, d_o = ctx.alloc(n * 4), ctx.alloc(n * 4)
    try:
        d_f.upload(pf)
        d_t.upload(pt)
        rc, _, _, dho, cnt = ctx.warp_pair_hash_raw(d_f, d_t, po, SPEEDS, None, 5, cap=n, device_in=True, out_key=d_k, out_t1=d_o)
        assert rc == _ffi.OK and cnt == n
        assert np.array_equal(dho, ho)
        assert np.array_equal(d_k.download(np.uint32, n), k) and np.array_equal(d_o.download(np.uint32, n), t1)
    finally:
        for b in (d_f, d_t, d_k, d_o):
            b.free()


def test_small_capacity_names_the_exact_count(ctx, packed):
    from shazam_amd import _ffi
    pf, pt, po = packed
    k, t1, ho = ctx.warp_pair_hash(pf, pt, po, SPEEDS, None, 5)
    n = len(k)
    for cap in (0, 1, n - 1):
        rc, _, _, cho, cnt = ctx.warp_pair_hash_raw(pf, pt, po, SPEEDS, None, 5, cap=cap)
        assert rc == _ffi.E_CAPACITY and cnt == n
        assert np.array_equal(cho, ho)
    rc, kk, tt, _, cnt = ctx.warp_pair_hash_raw(pf, pt, po, SPEEDS, None, 5, cap=n)
    assert rc == _ffi.OK and cnt == n and np.array_equal(kk, k) and np.array_equal(tt, t1)
    # the context is usable after the refusals
    k2, _, _ = ctx.warp_pair_hash(pf, pt, po, SPEEDS, None, 5)
    assert np.array_equal(k2, k)


@functools.lru_cache(maxsize=None)
def _long_clip(P):
    """One clip of exactly P peaks in (t asc, f asc) order: 1 to 3 frames from one occupied frame to the next, 0 to 6 distinct
    bins a frame, the last frame cut where the count reaches P."""
    rng = np.random.default_rng(20240 + P)
    f, t, fr = [], [], 0
    while len(f) < P:
        fr += int(rng.integers(1, 4))
        n = int(rng.integers(0, 7))
        f.extend(sorted(rng.choice(2049, n, replace=False).tolist()))
        t.extend([fr] * n)
    pf, pt = np.asarray(f[:P], np.uint16), np.asarray(t[:P], np.uint32)
    for a in (pf, pt):
        a.setflags(write=False)
    return pf, pt, np.asarray([0, P], np.uint64)


@pytest.mark.parametrize("fan", [2, 5])
@pytest.mark.parametrize("ladder", [[40000], [65536], [40000, 65536, 70000]], ids=["below", "unity", "three"])
@pytest.mark.parametrize("P", [2048, 2049, 8192, 8193])
def test_item_counts_on_the_scan_route_edges(ctx, P, ladder, fan):
    """sp_count scans P x len(ladder) items twice (keep flags, partner counts).  One rung: P items, on the edges between the
    scan's single tile, its one-workgroup loop and its flat route; three rungs of 8192 / 8193 peaks: well inside the flat
    route.  [40000] is below unity: frames merge and the peaks are re-ranked."""
    pf, pt, po = _long_clip(P)
    assert len(pf) == P and np.all(np.diff(pt.astype(np.int64) * 4096 + pf) > 0)
    k, t1, ho = ctx.warp_pair_hash(pf, pt, po, ladder, None, fan)
    ek, et, eho = T.warp_pair_batch(pf, pt, po, [0, 1], ladder, fan)
    assert np.array_equal(ho, eho)
    assert np.array_equal(k, ek) and np.array_equal(t1, et)
    assert len(ho) == len(ladder) + 1 and len(k) >= P // 2
