"""GPU: shz_table_song_hashes -- the rows of listed songs gathered on the device -- against numpy on Table.export(): a
boolean mask and a lexsort per listed id.  Every comparison is exact.

The gather walks a segment's song-id column in blocks of 1,024 rows, one wave a block, 64 rows a load, four blocks a
workgroup; the row totals below sit on and beside every wave, block and workgroup border (and 3 x 4,096 + 17 spans
several workgroups).  Tables are row-level numpy tables, one segment or three frozen ones plus the active; the lists are
unsorted, hold one id, ids without rows inside and above the table's range, the table's largest id alone (the bitmap's
last word) and ids on both sides of a 32-bit bitmap word."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 17)
SEG_SIZES = (257, 4097, 3 * 4096 + 17)
HOLE = 7            # an id inside the range that never gets a row
ONE_SEG, ALL_SEG = 34, 35   # segmented tables: a song with rows in one segment only / in every segment


def make_rows(seed, n, n_songs=None, max_off=3000):
    """n distinct rows (key32, sid, off) as int64, in random order: songs 1 .. n_songs without HOLE (31, 32, 33 and the
    largest id, 96, are there whenever n allows), keys from a small pool so that a song holds a key at several offsets"""
    rng = np.random.default_rng(seed)
    if n_songs is None:
        n_songs = 96 if n >= 1023 else max(1, min(40, n // 4))
    ids = np.array([s for s in range(1, n_songs + 1) if s != HOLE or n_songs == HOLE], np.int64)
    pool = rng.integers(0, 1 << 32, max(1, n // 3), dtype=np.int64)
    k = pool[rng.integers(0, len(pool), 3 * n + 8)]
    s = ids[rng.integers(0, len(ids), 3 * n + 8)]
    o = rng.integers(0, max_off + 1, 3 * n + 8, dtype=np.int64)
    if n >= len(ids):
        s[:len(ids)] = ids                                   # every song has a row
    rows = np.stack([k, s, o], 1)
    _, first = np.unique(rows, axis=0, return_index=True)
    rows = rows[np.sort(first)][:n]
    assert len(rows) == n
    return rows[:, 0], rows[:, 1], rows[:, 2]


def build(ctx, tk, ts, to, segmented=False):
    import shazam_amd as S
    t = S.Table(ctx)
    u = [np.ascontiguousarray(x, np.uint32) for x in (tk, ts, to)]
    if segmented:
        t.set_segment_rows(max(16, (len(tk) + 3) // 4))           # a quarter fits a segment: three frozen ones and the active
        for part in np.array_split(np.arange(len(tk)), 4):
            t.insert(u[0][part], u[1][part], u[2][part])
            t.finalize()
    else:
        t.insert(*u)
        t.finalize()
    return t


def expected(ek, es, eo, sids):
    """(row_off, key32, off) from the exported rows"""
    ro, ks, os_ = [0], [], []
    for s in sids:
        m = es == s
        order = np.lexsort((eo[m], ek[m]))
        ks.append(ek[m][order])
        os_.append(eo[m][order])
        ro.append(ro[-1] + int(m.sum()))
    return (np.array(ro, np.uint64), np.concatenate(ks).astype(np.uint32) if ks else np.zeros(0, np.uint32),
            np.concatenate(os_).astype(np.uint32) if os_ else np.zeros(0, np.uint32))


def check(t, exported, sids, label):
    sids = np.asarray(sids, np.uint32)
    want = expected(*exported, sids)
    got = t.song_hashes(sids)
    for name, g, w in zip(("row_off", "key32", "off"), got, want):
        assert np.array_equal(g, w), f"{label}: {name} differs (list {sids[:8].tolist()}...)"
    counts, k, o = t.song_hashes(sids, counts_only=True)
    assert np.array_equal(counts, want[0]) and len(k) == 0 and len(o) == 0, f"{label}: counts-only"
    return got


def lists_for(ts, rng):
    """the id list shapes of the issue, from the ids the table holds"""
    ids = np.unique(ts)
    top = int(ids.max())
    shuffled = rng.permutation(ids)
    out = {
        "all_unsorted_plus_absent": np.concatenate([shuffled[: len(ids) // 2], [top + 5, HOLE if HOLE not in ids else top + 9],
                                                    shuffled[len(ids) // 2:]]),
        "one_id": ids[:1],
        "largest_alone": np.array([top]),
        "above_largest_alone": np.array([top + 1]),
        "hole_alone": np.array([HOLE if HOLE not in ids else top + 2]),
        "none": np.zeros(0, np.int64),
    }
    if {31, 32, 33} <= set(ids.tolist()):
        out["word_border"] = np.array([33, 31, 32])
        out["word_border_31"] = np.array([31])
        out["word_border_32"] = np.array([32])
    if len(ids) > 20:
        out["one_in_a_hundred"] = ids[len(ids) // 2: len(ids) // 2 + 1]
    return out


@pytest.mark.parametrize("n", SIZES)
def test_gather_equals_numpy_on_the_export(n):
    import shazam_amd as S
    ctx = S.get_context(0)
    tk, ts, to = make_rows(100 + n, n)
    t = build(ctx, tk, ts, to)
    ex = t.export()
    assert len(ex[0]) == n
    rng = np.random.default_rng(n)
    for name, sids in lists_for(ts, rng).items():
        got = check(t, ex, sids, f"n={n} {name}")
        if name == "all_unsorted_plus_absent":
            assert int(got[0][-1]) == n                                          # every row hits
            assert np.array_equal(np.diff(got[0].astype(np.int64)),
                                  np.bincount(ts, minlength=int(np.max(sids)) + 1)[np.asarray(sids, np.int64)])
        if name in ("above_largest_alone", "hole_alone", "none"):
            assert int(got[0][-1]) == 0                                          # no row hits
    t.close()


@pytest.mark.parametrize("n", SEG_SIZES)
def test_gather_over_three_frozen_segments_and_the_active(n):
    """song ONE_SEG has rows in one segment only, song ALL_SEG in every one (read off the export: keys rise inside a segment)"""
    import shazam_amd as S
    ctx = S.get_context(0)
    tk, ts, to = make_rows(200 + n, n, n_songs=33)
    quarter = n // 4
    extra_k = np.arange(1, 13, dtype=np.int64) * 0x01010101
    # ALL_SEG: three rows into every quarter; ONE_SEG: five rows into the first quarter
    pos = np.concatenate([q * quarter + np.arange(3) for q in range(4)])
    ts[pos], tk[pos], to[pos] = ALL_SEG, extra_k, np.arange(12) * 7
    ts[10:15], tk[10:15], to[10:15] = ONE_SEG, extra_k[:5] + 1, np.arange(5)
    t = build(ctx, tk, ts, to, segmented=True)
    assert t.segments() == 4
    ex = t.export()
    seg = np.concatenate([[0], np.cumsum(np.diff(ex[0].astype(np.int64)) < 0)])
    assert seg[-1] == 3, "the export does not show four rising key runs"
    assert len(np.unique(seg[ex[1] == ONE_SEG])) == 1 and (ex[1] == ONE_SEG).sum() == 5
    assert len(np.unique(seg[ex[1] == ALL_SEG])) == 4
    rng = np.random.default_rng(n)
    for name, sids in lists_for(ts, rng).items():
        check(t, ex, sids, f"segmented n={n} {name}")
    check(t, ex, [ALL_SEG, 2, ONE_SEG], f"segmented n={n} planted")
    check(t, ex, [ONE_SEG], f"segmented n={n} one segment")
    t.close()


@pytest.mark.parametrize("segmented", (False, True))
def test_wide_offsets_and_many_ids_take_the_two_sort_path(segmented):
    """slot, key32 and offset fit one 64-bit word while bits(slots) + 32 + bits(largest offset) <= 64; a table offset of 2^31 - 1
    with three listed songs or more does not: the hits are sorted twice.  Two listed songs still fit (1 + 32 + 31)."""
    import shazam_amd as S
    ctx = S.get_context(0)
    tk, ts, to = make_rows(31, 2000, n_songs=40, max_off=2 ** 31 - 1)
    to[0] = 2 ** 31 - 1
    t = build(ctx, tk, ts, to, segmented=segmented)
    ex = t.export()
    ids = np.unique(ts)
    rng = np.random.default_rng(5)
    check(t, ex, rng.permutation(ids), "wide: all")
    check(t, ex, [int(ts[0]), 3, 9], "wide: three")
    check(t, ex, [int(ts[0]), 3], "wide: two")
    check(t, ex, [int(ts[0])], "wide: one")
    t.close()


def test_capacity_duplicates_staged_rows_and_repeatability():
    import shazam_amd as S
    from shazam_amd import _ffi
    ctx = S.get_context(0)
    L = _ffi.lib()
    n = 3 * 4096 + 17
    tk, ts, to = make_rows(77, n)
    t = build(ctx, tk, ts, to, segmented=True)
    ex = t.export()
    sids = np.array([40, 2, 96, HOLE, 33, 1000], np.uint32)
    want = expected(*ex, sids)
    total = int(want[0][-1])
    assert total > 100
    # one row short: SHZ_E_CAPACITY, row_off filled all the same
    ro = np.zeros(len(sids) + 1, np.uint64)
    k, o = np.full(total, 0xAAAAAAAA, np.uint32), np.full(total, 0xAAAAAAAA, np.uint32)
    rc = L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), _ffi.ptr(k), _ffi.ptr(o), total - 1, 0)
    assert rc == _ffi.E_CAPACITY and np.array_equal(ro, want[0])
    assert (k == 0xAAAAAAAA).all() and (o == 0xAAAAAAAA).all()
    # exactly enough: the rows; twice: the same arrays
    for _ in range(2):
        ro[:] = 0
        rc = L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), _ffi.ptr(k), _ffi.ptr(o), total, 0)
        assert rc == _ffi.OK
        assert np.array_equal(ro, want[0]) and np.array_equal(k, want[1]) and np.array_equal(o, want[2])
    a, b = t.song_hashes(np.unique(ts)), t.song_hashes(np.unique(ts))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # device output
    dk, do = ctx.alloc(total * 4), ctx.alloc(total * 4)
    ro[:] = 0
    rc = L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), _ffi.ptr(dk), _ffi.ptr(do), total,
                                 _ffi.SONGS_DEVICE_OUT)
    assert rc == _ffi.OK and np.array_equal(ro, want[0])
    assert np.array_equal(dk.download(np.uint32, total), want[1]) and np.array_equal(do.download(np.uint32, total), want[2])
    dk.free()
    do.free()
    # refusals: one column alone, an unknown flag, no row_off, an id twice -- before anything is launched
    ro[:] = 5
    assert L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), _ffi.ptr(k), None, total, 0) == _ffi.E_INVALID
    assert L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), None, _ffi.ptr(o), total, 0) == _ffi.E_INVALID
    assert L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), ro.ctypes.data_as(_ffi.u64p), None, None, 0, 1) == _ffi.E_INVALID
    assert L.shz_table_song_hashes(t.h, _ffi.ptr(sids), len(sids), None, None, None, 0, 0) == _ffi.E_INVALID
    twice = np.array([40, 2, 96, 2], np.uint32)
    assert L.shz_table_song_hashes(t.h, _ffi.ptr(twice), 4, ro.ctypes.data_as(_ffi.u64p), None, None, 0, 0) == _ffi.E_INVALID
    assert (ro == 5).all()
    with pytest.raises(S.ShzError) as e:
        t.song_hashes([3, 3])
    assert e.value.code == _ffi.E_INVALID and "twice" in str(e.value)
    # no ids: SHZ_OK, row_off[0] = 0
    one = np.full(1, 9, np.uint64)
    assert L.shz_table_song_hashes(t.h, None, 0, one.ctypes.data_as(_ffi.u64p), None, None, 0, 0) == _ffi.OK and one[0] == 0
    # staged rows: SHZ_E_STATE, as shz_table_song_rows
    t.insert(np.array([1], np.uint32), np.array([2], np.uint32), np.array([3], np.uint32))
    with pytest.raises(S.ShzError) as e:
        t.song_hashes([2])
    assert e.value.code == _ffi.E_STATE
    with pytest.raises(S.ShzError) as e:
        t.song_rows(2)
    assert e.value.code == _ffi.E_STATE
    t.finalize()
    ex = t.export()
    check(t, ex, [2, 40], "after the staged row")
    assert t.song_rows(2) == int(t.song_hashes([2], counts_only=True)[0][1])
    t.close()


def test_empty_table_and_counts_for_every_id():
    import shazam_amd as S
    ctx = S.get_context(0)
    t = S.Table(ctx)
    t.finalize()
    ro, k, o = t.song_hashes([3, 1])
    assert ro.tolist() == [0, 0, 0] and len(k) == 0 and len(o) == 0
    tk, ts, to = make_rows(9, 5000)
    t.insert(*[np.ascontiguousarray(x, np.uint32) for x in (tk, ts, to)])
    t.finalize()
    every = np.arange(0, 130, dtype=np.uint32)                                      # 0 and ids past the largest included
    ro, _, _ = t.song_hashes(every, counts_only=True)
    assert np.array_equal(np.diff(ro.astype(np.int64)), np.bincount(ts, minlength=130))
    t.close()
