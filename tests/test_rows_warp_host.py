"""CPU: the row warp's arithmetic (shz_warp_row_host -- the inline map the kernels of shz_warp_rows call, run over host
arrays) against its numpy statement tests/rows_warp_twin.py, bit for bit, and the relation of the row warp to the peak-level
warp of shz_warp_pair_hash_tf (tests/warp_twin.py) on fingerprints of the oracle.  No GPU.

A row (key32 = f1 << 20 | f2 << 8 | dt, off = t1) is the two peaks (f1, t1) and (f2, t1 + dt); the warp moves both and
forms the key again.  The edge rows below are built from the definition: the first f with f' = 2048 / 2049 at a factor,
and an (off, dt) whose dt' is exactly 200 / 201."""
import numpy as np
import pytest

import rows_warp_twin as RT
import warp_twin as WT
from oracle import cpu_ref as O, synth
from shazam_amd import _ffi

FACTORS = (32768, 40000, 60000, 65535, 65536, 65537, 67502, 70000, 100000, 131072)


def _key(f1, f2, dt):
    return (np.asarray(f1, np.int64) << 20) | (np.asarray(f2, np.int64) << 8) | np.asarray(dt, np.int64)


def _check(key32, off, t16, f16):
    """library == twin on these rows: the mask, and the kept rows' images in order; dropped rows come back as 0"""
    gk, go, gkeep = _ffi.warp_row_host(key32, off, t16, f16)
    wk, wo, wkeep = RT.warp_rows(key32, off, t16, f16)
    assert gkeep.dtype == bool and np.array_equal(gkeep, wkeep), (t16, f16)
    assert np.array_equal(gk[gkeep], wk) and np.array_equal(go[gkeep], wo), (t16, f16)
    assert not gk[~gkeep].any() and not go[~gkeep].any()
    return wk, wo, wkeep


@pytest.mark.parametrize("t16", FACTORS)
def test_random_rows_equal_the_twin(t16):
    rng = np.random.default_rng(t16)
    n = 20000
    key = _key(rng.integers(0, 2049, n), rng.integers(0, 2049, n), rng.integers(0, 201, n))
    off = rng.integers(0, 1 << 19, n)
    kept = 0
    for f16 in FACTORS:
        kept += int(_check(key, off, t16, f16)[2].sum())
    assert 0 < kept < n * len(FACTORS)                     # some rows leave, some stay


def test_identity_returns_the_input():
    rng = np.random.default_rng(5)
    n = 5000
    key = _key(rng.integers(0, 2049, n), rng.integers(0, 2049, n), rng.integers(0, 201, n))
    off = rng.integers(0, 1 << 19, n)
    gk, go, keep = _ffi.warp_row_host(key, off, 65536, 65536)
    assert keep.all() and np.array_equal(gk, key) and np.array_equal(go, off)
    assert gk.dtype == np.uint32 and go.dtype == np.uint32
    e = _ffi.warp_row_host(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 65536, 65536)
    assert all(len(x) == 0 for x in e)


@pytest.mark.parametrize("f16", (32768, 40000, 60000, 65000, 65535))
def test_frequency_edge_2048_stays_and_2049_leaves(f16):
    fp = lambda f: (2 * 65536 * f + f16) // (2 * f16)
    at = {fp(f): f for f in range(2048, -1, -1)}           # the first f of every f'
    assert 2048 in at and fp(at[2048]) == 2048
    over = min(f for f in range(4096) if fp(f) > 2048)     # (a key holds 12 bits of f)
    rows = [(at[2048], 7, 3, True), (7, at[2048], 3, True), (at[2048], at[2048], 0, True),
            (over, 7, 3, False), (7, over, 3, False)]
    if f16 >= 60000:                                       # (below, f' steps by two: 2049 is no image)
        assert fp(over) == 2049
    key = _key([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    off = np.arange(100, 100 + len(rows))
    wk, wo, keep = _check(key, off, 65536, f16)
    assert keep.tolist() == [r[3] for r in rows]
    assert (wk[0] >> 20) == 2048 and ((wk[1] >> 8) & 0xFFF) == 2048 and wk[2] == (2048 << 20 | 2048 << 8)


@pytest.mark.parametrize("t16", (65537, 70000, 100000, 131072))
def test_time_edge_dt_200_stays_and_201_leaves(t16):
    tp = lambda t: (t * t16 + 32768) >> 16
    found = {}
    for off in range(0, 400):
        for dt in range(0, 256):                           # (a key holds 8 bits of dt)
            d = tp(off + dt) - tp(off)
            if d in (200, 201, 202) and d not in found:
                found[d] = (off, dt)
    assert 200 in found and (201 in found or t16 == 131072 and 202 in found)      # (2x: dt' is even)
    rows = [(found[d], d <= 200) for d in sorted(found)]
    key = _key([5] * len(rows), [9] * len(rows), [r[0][1] for r in rows])
    off = np.asarray([r[0][0] for r in rows])
    wk, wo, keep = _check(key, off, t16, 65536)
    assert keep.tolist() == [r[1] for r in rows]
    assert (wk[0] & 0xFF) == 200 and wo[0] == tp(found[200][0])


def test_dt_zero_and_the_extreme_factors():
    rng = np.random.default_rng(11)
    n = 3000
    key = _key(rng.integers(0, 2049, n), rng.integers(0, 2049, n), 0)
    off = rng.integers(0, 1 << 19, n)
    for t16 in (32768, 65536, 131072):
        for f16 in (32768, 65536, 131072):
            wk, wo, keep = _check(key, off, t16, f16)
            assert not (wk & 0xFF).any()                   # both peaks share a frame, before and after
            if f16 >= 65536:
                assert keep.all()                          # frequencies only fall: no row leaves
    # 0.5x in time halves dt (two frames may merge), 2x doubles it: dt <= 100 stays, dt > 100 leaves
    key = _key(100, 200, np.arange(0, 201))
    off = np.full(201, 1000)
    _, _, keep = _check(key, off, 131072, 65536)
    assert keep.tolist() == [d <= 100 for d in range(201)]
    wk, wo, keep = _check(key, off, 32768, 65536)
    assert keep.all() and np.array_equal(wk & 0xFF, (np.arange(1000, 1201) * 32768 + 32768 >> 16) - 500) and (wo == 500).all()
    # factors outside [32768, 131072] are refused
    for bad in ((32767, 65536), (65536, 131073), (0, 65536)):
        with pytest.raises(_ffi.ShzError) as e:
            _ffi.warp_row_host(key, off, *bad)
        assert e.value.code == _ffi.E_INVALID


def test_batch_twin_order_and_csr():
    rng = np.random.default_rng(3)
    counts = [0, 5, 1, 40]
    ro = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(ro[-1])
    key = _key(rng.integers(0, 2049, n), rng.integers(0, 2049, n), rng.integers(0, 201, n))
    off = rng.integers(0, 5000, n)
    tempos, pitches = [65536, 131072, 32768], [65536, 32768, 131072]
    k, o, oro = RT.warp_rows_batch(key, off, ro, tempos, pitches)
    assert len(oro) == len(counts) * 3 + 1 and oro[-1] == len(k) == len(o)
    for q in range(len(counts)):
        a, b = int(ro[q]), int(ro[q + 1])
        for v in range(3):
            wk, wo, _ = RT.warp_rows(key[a:b], off[a:b], tempos[v], pitches[v])
            s = slice(int(oro[q * 3 + v]), int(oro[q * 3 + v + 1]))
            assert np.array_equal(k[s], wk) and np.array_equal(o[s], wo)
        assert oro[q * 3 + 1] - oro[q * 3] == counts[q]    # the identity keeps every row


@pytest.fixture(scope="module")
def songs():
    """(key32, t1, peak_f, peak_t) of two 10 s music-like clips, from the oracle"""
    return [O.fingerprint_keys(synth.music_clip(77, c, 10 * 44100)) for c in range(2)]


@pytest.mark.parametrize("t16,f16", [(65536, 65536), (67502, 67502), (65536, 68813), (70000, 65536), (66000, 72000), (131072, 131072)])
def test_at_or_above_unity_the_row_warp_is_the_peak_warp(songs, t16, f16):
    """t16 >= 65536 keeps the order of the peaks and lets no two frames merge, f16 >= 65536 lets no peak leave, and
    dt' >= dt: a pair within 200 frames after the warp was within 200 before it, at the same rank among its peak's partners.
    So warping the hashes equals hashing the warped peaks, entry for entry"""
    for k, t1, pf, pt in songs:
        assert len(k) > 2000
        rk, ro, _ = RT.warp_rows(k, t1, t16, f16)
        pk, po = WT.warp_pair_tf(pf, pt, t16, f16)
        assert np.array_equal(rk, pk) and np.array_equal(ro, po)
        gk, go, keep = _ffi.warp_row_host(k, t1, t16, f16)
        assert np.array_equal(gk[keep], pk) and np.array_equal(go[keep], po)


def test_below_unity_the_two_differ_by_a_few_per_cent(songs):
    """(by design: the peak-level warp pairs again after frames merge and peaks leave)"""
    k, t1, pf, pt = songs[0]
    s16 = RT.q16(0.97)
    rk, ro, _ = RT.warp_rows(k, t1, s16, s16)
    pk, po = WT.warp_pair_tf(pf, pt, s16, s16)
    rows, peaks = set(zip(rk.tolist(), ro.tolist())), set(zip(pk.tolist(), po.tolist()))
    common = len(rows & peaks)
    assert rows != peaks and common >= 0.9 * max(len(rows), len(peaks))
