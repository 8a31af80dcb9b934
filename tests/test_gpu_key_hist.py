"""GPU: the key-size histogram of a table (Table.key_hist, shz_table_key_hist) against numpy on the exported rows:
np.unique(export()[0], return_counts=True) put through floor.bucket_of.  Bucket edges, runs across a workgroup's chunk of
rows, keys at the borders of the bucket directory, keys spread over segments (counted once, with all their rows), key-range
segments, deleted songs and the sharded table.  Every comparison is exact."""
import numpy as np
import pytest

from shazam_amd import floor
from test_gpu_key_cap import _segmented

pytestmark = pytest.mark.gpu

CHUNK = 4096          # rows of one workgroup of key_hist_kernel (KH_CHUNK)


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _want(tk):
    keys, rows = np.zeros(32, np.uint64), np.zeros(32, np.uint64)
    uniq, counts = np.unique(tk, return_counts=True)
    for n in counts.tolist():
        keys[floor.bucket_of(n)] += np.uint64(1)
        rows[floor.bucket_of(n)] += np.uint64(n)
    return {"keys": keys, "rows": rows, "max_rows": int(counts.max()) if len(counts) else 0, "n_keys": len(uniq)}


def _check(t, what=""):
    """key_hist() of a Table or ShardedTable against numpy on its export; returns the histogram"""
    h = t.key_hist()
    w = _want(t.export()[0])
    assert h["keys"].dtype == np.uint64 and h["rows"].dtype == np.uint64 and h["keys"].shape == h["rows"].shape == (32,), what
    assert h["keys"].tolist() == w["keys"].tolist(), (what, "keys")
    assert h["rows"].tolist() == w["rows"].tolist(), (what, "rows")
    assert (h["max_rows"], h["n_keys"]) == (w["max_rows"], w["n_keys"]), what
    assert int(h["rows"].sum()) == t.rows()[0] and int(h["keys"].sum()) == h["n_keys"], what
    return h


def _sized(S, ctx, sizes, keys=None):
    """a table whose key keys[i] (default 7 i + 3) holds sizes[i] rows"""
    keys = [7 * i + 3 for i in range(len(sizes))] if keys is None else keys
    tk = np.concatenate([np.full(n, k) for k, n in zip(keys, sizes)]).astype(np.uint32)
    r = np.concatenate([np.arange(n) for n in sizes])
    t = S.Table(ctx)
    t.insert(tk, (1 + r % 9).astype(np.uint32), (r // 9).astype(np.uint32))
    t.finalize()
    return t


def test_an_empty_table_and_one_row(S, ctx):
    t = S.Table(ctx)
    try:
        h = t.key_hist()
        assert not h["keys"].any() and not h["rows"].any() and (h["max_rows"], h["n_keys"]) == (0, 0)
        t.finalize()
        h = _check(t, "empty, finalized")
        assert h["n_keys"] == 0
        t.insert(np.array([77], np.uint32), 3, np.array([5], np.uint32))
        with pytest.raises(S.ShzError):                    # staged rows: finalize first, as export() asks
            t.key_hist()
        t.finalize()
        h = _check(t, "one row")
        assert h["keys"][0] == 1 and h["rows"][0] == 1 and (h["max_rows"], h["n_keys"]) == (1, 1)
        t.clear()
        assert _check(t, "cleared")["n_keys"] == 0
    finally:
        t.close()


def test_bucket_edges(S, ctx):
    sizes = [1, 16, 17, 32, 33, 64, 65, 4095, 4096, 4097]
    t = _sized(S, ctx, sizes)
    try:
        h = _check(t, "edges")
        assert h["max_rows"] == 4097 and h["n_keys"] == len(sizes)
        for b, n in ((0, 1), (15, 1), (16, 1), (17, 2), (18, 2), (23, 1), (24, 2)):
            assert int(h["keys"][b]) == n, b
        assert int(h["rows"][24]) == 4096 + 4097 and int(h["rows"][17]) == 32 + 33
    finally:
        t.close()


@pytest.mark.parametrize("first", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK - 100, 3 * CHUNK - 7])
def test_a_run_across_a_chunk_of_rows(S, ctx, first):
    """the rows before the run fill `first` places: the run of 200 rows then starts just before, at and just behind a
    workgroup's border, or lies across it; a run of 2 CHUNK + 5 rows covers whole chunks without a head"""
    small = [1, 2, 3] * 40
    small = small[:max(0, min(len(small), first // 2))]
    pad = first - sum(small)
    sizes = small + ([pad] if pad > 0 else []) + [200, 2 * CHUNK + 5, 1]
    t = _sized(S, ctx, sizes)
    try:
        k = t.export()[0]
        assert int(np.flatnonzero(np.diff(k.astype(np.int64)) != 0)[len(sizes) - 4]) + 1 == first
        _check(t, ("chunk", first))
    finally:
        t.close()


def test_keys_at_the_borders_of_the_bucket_directory(S, ctx):
    keys = [0x00, 0x01, 0xFF, 0x100, 0x1FF, 0x200, 0x2FE, 0x2FF, 0x300, 0xFFFF, 0x10000, 0x100FF, 0xABCDFF, 0xABCE00, 0xFFFFFFFF]
    sizes = [3, 1, 17, 2, 40, 1, 5, 16, 33, 1, 2, 64, 7, 9, 18]
    t = _sized(S, ctx, sizes, keys)
    try:
        h = _check(t, "directory borders")
        assert h["n_keys"] == len(keys) and h["max_rows"] == 64
    finally:
        t.close()


@pytest.mark.parametrize("n_batches", [1, 3, 5])
def test_keys_spread_over_segments_count_once(S, ctx, n_batches):
    c = 3 * n_batches - 1
    t = _segmented(S, ctx, n_batches, c, 200 + n_batches)
    try:
        assert t.segments() >= min(n_batches, 4)
        h = _check(t, ("segments", n_batches))
        assert int(h["keys"][floor.bucket_of(c + 1)]) >= 1 and int(h["keys"][floor.bucket_of(c)]) >= 1     # keys 500 and 600
    finally:
        t.close()


def test_key_range_segments_and_deleted_songs(S, ctx):
    rng = np.random.default_rng(23)
    t = S.Table(ctx)
    t.set_segment_rows(256)
    for run in range(2):
        k = (rng.integers(0, 90, 800) ** 2 % 97).astype(np.uint32) * np.uint32(0x55)       # uneven key sizes
        t.insert(k, rng.integers(1 + 50 * run, 51 + 50 * run, 800).astype(np.uint32), rng.integers(0, 4000, 800).astype(np.uint32))
        if run == 0:
            t.seal_run()
    t.finalize()
    try:
        assert t.segments() >= 4
        before = _check(t, "key ranges")
        assert t.delete_songs(np.arange(1, 30, dtype=np.uint32)) > 0
        after = _check(t, "after delete_songs")
        assert int(after["rows"].sum()) < int(before["rows"].sum())
        t.delete_songs(np.arange(0, 200, dtype=np.uint32))
        assert _check(t, "all songs deleted")["n_keys"] == 0
    finally:
        t.close()


@pytest.mark.parametrize("nshards", [2, 3])
def test_sharded_table(S, ctx, nshards):
    from shazam_amd.shard import ShardedTable
    rng = np.random.default_rng(nshards)
    sizes = np.concatenate([rng.integers(1, 20, 60), [100, 500, 4100]])
    keys = rng.choice(1 << 20, len(sizes), replace=False)
    tk = np.repeat(keys, sizes).astype(np.uint32)
    r = np.concatenate([np.arange(n) for n in sizes])
    st, t = ShardedTable(ctx, nshards=nshards), S.Table(ctx)
    try:
        for x in (st, t):
            x.insert(tk, (1 + r % 5).astype(np.uint32), (r // 5).astype(np.uint32))
            x.finalize()
        hs, h = _check(st, ("sharded", nshards)), _check(t, "unsharded")
        assert hs["keys"].tolist() == h["keys"].tolist() and hs["rows"].tolist() == h["rows"].tolist()
        assert (hs["max_rows"], hs["n_keys"]) == (h["max_rows"], h["n_keys"]) == (4100, len(sizes))
        db = S.get_database("hip")(ctx=ctx)
        assert set(db.key_hist()) == {"keys", "rows", "max_rows", "n_keys"} and db.key_hist()["n_keys"] == 0
    finally:
        st.close()
        t.close()
