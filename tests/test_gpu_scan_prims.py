"""GPU: the three device exclusive scans of shz_prims.hip (shz_scan_u32, shz_scan_popc64, shz_scan_u64) called directly
through shz_scan_host, against numpy's cumsum in uint64: every output element and the total are compared for equality.

scan_impl picks one of four routes by the number of tiles (tile = SCAN_TILE = 256 threads x 8 items; thread t of a
workgroup holds the elements 8t .. 8t + 7 of its tile):

  route                elements n                                     smallest n that reaches it   what runs
  single tile          1 .. TILE                                      1                            scan_apply_kernel, no block offsets
  one-workgroup loop   TILE + 1 .. LOOP_TILES * TILE                  2049                         scan_loop_kernel, carry from tile to tile
  flat                 LOOP_TILES * TILE + 1 .. FLAT_TILES * TILE     8193                         scan_sums_kernel + scan_apply_flat_kernel
  recursive            from FLAT_TILES * TILE + 1                     4,194,305                    sums, scan_impl in place on the sums, scan_apply_kernel

The inner scan of the recursive route takes the routes again by ITS tile count: 4,194,305 elements give 2,049 sums (loop
route), LOOP_TILES * TILE * TILE + 1 = 16,777,217 elements give 8,193 sums (flat route, with the tail of the temporary as
its scratch).  An inner scan that recurses itself needs more than FLAT_TILES * TILE * TILE = 8.5 x 10^9 elements: out of
scope here.  The sizes below are derived from the three constants, which mirror the defines of shz_prims.hip."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048          # SCAN_TILE = SCAN_THREADS * SCAN_ITEMS
LOOP_TILES = 4       # SCAN_LOOP_TILES
FLAT_TILES = 2048    # SCAN_FLAT_TILES

LOOP_MAX, FLAT_MAX = LOOP_TILES * TILE, FLAT_TILES * TILE
# lane, wave and workgroup item edges | single tile -> loop | loop -> flat
SMALL = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513,
         TILE - 1, TILE, TILE + 1,
         2 * TILE, 2 * TILE + 1, LOOP_MAX - 1, LOOP_MAX, LOOP_MAX + 1]
# flat -> recursive (the inner scan of 2,049 sums loops) | one more tile | 8,193 sums: the inner scan is flat
LARGE = [TILE * (FLAT_TILES - 1) + 5, FLAT_MAX - 1, FLAT_MAX, FLAT_MAX + 1,
         FLAT_MAX + TILE + 1,
         LOOP_MAX * TILE + 1]
VARIANT_SIZES = [1, TILE, TILE + 1, LOOP_MAX, LOOP_MAX + 1, FLAT_MAX + 1]
U32_MAX = (1 << 32) - 1

assert SMALL[-1] == 8193 and LARGE == [2048 * 2047 + 5, 4194303, 4194304, 4194305, 4194304 + 2049, 16777217]

U32, POPC64, U64 = 0, 1, 2
KINDS = {"u32": U32, "popc64": POPC64, "u64": U64}
ONES64 = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    import shazam_amd
    return shazam_amd.get_context(0)


def _impulse_positions(n):
    """(j, position) of the impulses that exist in an array of n elements"""
    return [(j, p) for j, p in enumerate([0, 7, 8, 511, 512, TILE - 1, TILE, TILE + 1, LOOP_MAX - 1, LOOP_MAX, n - 1]) if 0 <= p < n]


def _popcount(x):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.uint64)
    table = np.array([bin(i).count("1") for i in range(256)], np.uint64)
    return table[x.view(np.uint8).reshape(-1, 8)].sum(axis=1)


def _rng(kind, pattern, n):
    return np.random.default_rng([KINDS[kind], sum(map(ord, pattern)), n])


def _input(kind, pattern, n):
    rng = _rng(kind, pattern, n)
    if kind == "u32":
        if pattern == "random":
            return rng.integers(0, 16, n, dtype=np.uint32)
        if pattern == "ones":
            return np.ones(n, np.uint32)
        if pattern == "impulses":
            x = np.zeros(n, np.uint32)
            for j, p in _impulse_positions(n):
                x[p] += np.uint32(1 << j)
            return x
        if pattern == "limit":      # the values sum to exactly 2^32 - 1
            x = np.full(n, U32_MAX // n, np.uint32)
            x[-1] += np.uint32(U32_MAX - (U32_MAX // n) * n)
            return x
    if kind == "popc64":
        if pattern == "random":     # random words with runs of 0 and of all-ones words
            x = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
            for k in range(6):
                a = int(rng.integers(0, n)) if n else 0
                b = min(n, a + int(rng.integers(1, max(2, n // 5 + 2))))
                x[a:b] = ONES64 if k % 2 else np.uint64(0)
            return x
        if pattern == "sparse":     # about 4 bits a word
            w = [rng.integers(0, 1 << 63, n, dtype=np.uint64) for _ in range(4)]
            return w[0] & w[1] & w[2] & w[3]
        if pattern == "impulses":
            x = np.zeros(n, np.uint64)
            for _, p in _impulse_positions(n):
                x[p] = ONES64
            return x
    if kind == "u64":
        if pattern == "random":     # prefixes pass 2^32 inside a wave, inside a tile and between tiles
            return rng.integers(0, 1 << 40, n, dtype=np.uint64)
        if pattern == "impulses":
            x = np.zeros(n, np.uint64)
            for j, p in _impulse_positions(n):
                x[p] += np.uint64(1 << (32 + j))
            return x
        if pattern == "high bit":   # 2^63, then ones
            x = np.ones(n, np.uint64)
            x[0] = np.uint64(1 << 63)
            return x
    raise AssertionError((kind, pattern))


def _reference(kind, x):
    """(exclusive prefix sums as uint64, total as int) of the scanned values, with the no-overflow facts asserted on the host"""
    v = _popcount(x) if kind == "popc64" else x.astype(np.uint64)
    if len(v) == 0:
        return np.zeros(0, np.uint64), 0
    # uint64 addition cannot have wrapped: the top parts alone bound the sum below 2^63 + 2^62
    assert int((v >> np.uint64(32)).sum(dtype=np.uint64)) + len(v) < 3 << 30
    inc = np.cumsum(v, dtype=np.uint64)
    total = int(inc[-1])
    if kind != "u64":
        assert total <= U32_MAX      # the contract of the 32-bit scans
    return np.concatenate([np.zeros(1, np.uint64), inc[:-1]]), total


def _check(ctx, kind, x, **kw):
    want, total = _reference(kind, x)
    got, gtot = ctx.scan_prim(KINDS[kind], x, **kw)
    assert got.dtype == (np.uint64 if kind == "u64" else np.uint32) and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (kind, len(x), kw, "first wrong element", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    if kw.get("want_total", True):
        assert gtot == total, (kind, len(x), kw, gtot, total)
    else:
        assert gtot is None
    return got


SMALL_PATTERNS = {"u32": ["random", "ones", "impulses", "limit"], "popc64": ["random", "impulses"],
                  "u64": ["random", "impulses", "high bit"]}
LARGE_PATTERNS = {"u32": ["random", "impulses"], "popc64": ["random", "impulses"], "u64": ["random", "impulses"]}


def _cases():
    out = []
    for kind in KINDS:
        for n in SMALL:
            out += [(kind, p, n) for p in SMALL_PATTERNS[kind] if n > 0 or p not in ("limit", "high bit")]
        for n in LARGE:
            for p in LARGE_PATTERNS[kind]:
                if kind == "popc64" and p == "random" and n == LARGE[-1]:
                    p = "sparse"
                out.append((kind, p, n))
    out.append(("u64", "high bit", FLAT_MAX + 1))     # ... and through the block offsets of the recursive route
    return out


@pytest.mark.parametrize("kind,pattern,n", _cases())
def test_scan_equals_cumsum(ctx, kind, pattern, n):
    x = _input(kind, pattern, n)
    if pattern == "limit":
        assert int(x.sum(dtype=np.uint64)) == U32_MAX == 4294967295
    _check(ctx, kind, x)


@pytest.mark.parametrize("n", VARIANT_SIZES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_variants_equal_the_plain_call(ctx, kind, n):
    """The output on the input (what the sort does with its digit tables), no total pointer, and a call that follows a
    larger one whose block sums are still in the temporary."""
    x = _input(kind, "random", n)
    plain = _check(ctx, kind, x)
    if kind != "popc64":
        assert np.array_equal(_check(ctx, kind, x, in_place=True), plain)
        assert np.array_equal(_check(ctx, kind, x, in_place=True, want_total=False), plain)
    assert np.array_equal(_check(ctx, kind, x, want_total=False), plain)
    big = _input(kind, "random", n + 3 * LOOP_MAX + 17)     # flat or recursive: leaves its sums behind
    _check(ctx, kind, big)
    assert np.array_equal(_check(ctx, kind, x), plain)


def test_u32_limit_total_reads_4294967295(ctx):
    """The total itself, spelled out: a u32 scan whose values sum to 2^32 - 1, on every route below the recursive one."""
    for n in (1, TILE, TILE + 1, LOOP_MAX + 1):
        x = _input("u32", "limit", n)
        out, total = ctx.scan_prim(U32, x)
        assert total == 4294967295
        assert int(out[-1]) + int(x[-1]) == 4294967295


def test_refusals_leave_the_context_usable(ctx):
    from shazam_amd import _ffi
    L = _ffi.lib()
    x32, x64 = np.arange(100, dtype=np.uint32), np.arange(100, dtype=np.uint64)
    o32, o64 = np.zeros(100, np.uint32), np.zeros(100, np.uint64)
    tot = C.c_uint64(77)
    p = _ffi.ptr
    assert L.shz_scan_host(ctx.h, 3, p(x32), p(o32), 100, 0, C.byref(tot)) == _ffi.E_INVALID          # unknown kind
    assert L.shz_scan_host(ctx.h, 0xFFFFFFFF, p(x32), p(o32), 100, 0, C.byref(tot)) == _ffi.E_INVALID
    assert L.shz_scan_host(ctx.h, POPC64, p(x64), p(o32), 100, 1, C.byref(tot)) == _ffi.E_INVALID    # in place with popc64
    for kind, x, o in ((U32, x32, o32), (POPC64, x64, o32), (U64, x64, o64)):                        # null buffers, n > 0
        assert L.shz_scan_host(ctx.h, kind, None, p(o), 100, 0, C.byref(tot)) == _ffi.E_INVALID
        assert L.shz_scan_host(ctx.h, kind, p(x), None, 100, 0, C.byref(tot)) == _ffi.E_INVALID
        assert L.shz_scan_host(ctx.h, kind, None, None, 100, 1 if kind != POPC64 else 0, None) == _ffi.E_INVALID
    with pytest.raises(_ffi.ShzError):
        ctx.scan_prim(POPC64, x64, in_place=True)
    assert tot.value == 77 and not o32.any() and not o64.any()       # a refused call writes nothing
    # null buffers with n = 0 are no error: the total is set to 0 by a kernel of its own
    assert L.shz_scan_host(ctx.h, U64, None, None, 0, 0, C.byref(tot)) == _ffi.OK and tot.value == 0
    assert L.shz_scan_host(ctx.h, U32, None, None, 0, 0, None) == _ffi.OK
    for kind in KINDS:
        _check(ctx, kind, _input(kind, "random", LOOP_MAX + 1))
