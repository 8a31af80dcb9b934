"""GPU: the table's life cycle as operation sequences against a set model (tests/table_life_twin.py).

The table is the one stateful object of the library: staged columns, sealed runs in an arena, an active segment, frozen
segments with their bucket indexes and id ranges, and the cached maxima that size the vote key and the run packing.  Every
sequence here drives insert / insert_clips / seal_run / finalize / delete_songs / clear / set_segment_rows / set_run_rows
in a seeded order (tests/test_table_life_host.py asserts what each sequence reaches) and compares, at every checkpoint --
after a finalize, after a clear, after a delete that leaves nothing pending, the last without a finalize -- rows, segments,
export, song_rows, song_hashes, lookup and match with the model, exactly.

Directed cases beside them, one per defect the sequences or the reading for them found:
  * delete_songs of id 2^32 - 1 (the bitmap up to the largest listed id wrapped to no bits: a host heap overwrite);
  * the top-up of a segment that already holds more rows than a lowered limit (the room wrapped: 63/64 of the batch went in);
  * a table whose frozen segments were all deleted, and a cleared one, answered "table not finalized";
  * ids and offsets that outgrow the run packing while runs wait: refused, nothing lost, clear() recovers (pinned as is)."""
import numpy as np
import pytest

import table_life_twin as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    from shazam_amd import _ffi
    return _ffi, S.get_context(0)


@pytest.fixture(scope="module")
def small_runs():
    from shazam_amd import _ffi
    ctx = _ffi.Context(0)   # a context of its own: the switch holds for every table of the context
    ctx.set_debug(_ffi.DEBUG_RUN_LIMIT_SMALL)
    yield _ffi, ctx
    ctx.close()


def _run(F, ctx, ops, seed, what):
    t = F.Table(ctx)
    try:
        return T.drive([t], ops, seed, what)
    finally:
        t.close()


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("profile", T.PROFILES)
def test_random_sequence(env, profile, seed):
    F, ctx = env
    _run(F, ctx, T.sequence(seed, profile), seed, (profile, seed))


@pytest.mark.parametrize("seed", range(2))
@pytest.mark.parametrize("profile", T.PROFILES)
def test_random_sequence_small_run_limit(small_runs, profile, seed):
    F, ctx = small_runs
    _run(F, ctx, T.sequence(seed, profile), seed, (profile, seed, "run limit 65,536"))


def _unique_rows(n, first=0, sids=40):
    """n distinct rows, deterministic: row i = (a key of 997, song 1 + i % sids, offset i // sids)"""
    i = np.arange(first, first + n, dtype=np.int64)
    return ((i * 7919) % 997 * 1031 + 5).astype(np.uint32), (1 + i % sids).astype(np.uint32), (i // sids).astype(np.uint32)


def _checkpoint(t, model, seed, **ctx):
    T.check(t, model, np.random.default_rng(seed), dict({"what": ("directed", seed), "U": None}, **ctx))


def test_delete_songs_of_the_largest_ids(env):
    """Ids 1, 2^31 - 1, 2^32 - 2 and 2^32 - 1 (the column path: such ids do not pack).  Nothing in delete_songs is sized by
    the value of an id.  song_hashes is asked for song 1 and the absent id only: its scratch is, by its contract in
    shz_catalog.hip, 8 bytes per id up to the largest one listed that the table may hold."""
    F, ctx = env
    wide = np.array([1, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    k, _, o = _unique_rows(1200)
    s = wide[np.arange(1200) % 4]
    t, m = F.Table(ctx), T.Model()
    try:
        for x in (t, m):
            x.insert(k, s, o)
            x.finalize()
        _checkpoint(t, m, 1, hash_sid_max=40)
        deleted = set()
        for n, ids in enumerate(([0xFFFFFFFF], [0xFFFFFFFE, 5])):
            deleted |= {r for r in m.visible if r[1] in ids}
            nv, _ = m.delete_songs(ids)
            assert t.delete_songs(ids) == nv == 300
            _checkpoint(t, m, 2 + n, hash_sid_max=40, deleted=deleted, gone_sid=ids[0], checkpoint=3)
        assert t.delete_songs([0xFFFFFFFF]) == 0           # no such row any more
        _checkpoint(t, m, 4, hash_sid_max=40, deleted=deleted, gone_sid=0xFFFFFFFF)
    finally:
        t.close()
    # ... and a table that never held the id: narrow ids in packed runs
    t, m = F.Table(ctx), T.Model()
    try:
        k, s, o = _unique_rows(1000)
        for x in (t, m):
            x.insert(k, s, o)
            x.finalize()
        assert t.delete_songs([0xFFFFFFFF]) == 0
        assert t.delete_songs([0xFFFFFFFF, 3]) == m.delete_songs([0xFFFFFFFF, 3])[0] == 25
        _checkpoint(t, m, 5, gone_sid=3)
    finally:
        t.close()


def test_lowered_limit_starts_new_segments(env):
    """3,500 rows in the active segment under a limit of 4,000; the limit drops to 500; 1,500 new rows arrive.  The active
    segment has no room: it is frozen as it is and the batch starts segments of its own, 1 + ceil(1500 / 500) at least."""
    F, ctx = env
    t, m = F.Table(ctx), T.Model()
    try:
        t.set_segment_rows(4000)
        for x in (t, m):
            x.insert(*_unique_rows(3500))
            x.finalize()
        assert t.segments() == 1
        t.set_segment_rows(500)
        for x in (t, m):
            x.insert(*_unique_rows(1500, first=3500))
            x.finalize()
        assert t.segments() >= 1 + -(-1500 // 500), t.segments()
        assert t.rows() == (5000, 0)
        _checkpoint(t, m, 6)
    finally:
        t.close()


def test_table_of_frozen_segments_deleted_to_empty_answers(env):
    """tiny segments, and a last batch that only repeats rows the table holds: the active segment is topped up, frozen, and
    nothing is left to start a new one.  Every id is deleted: no segment remains and no row waits for a finalize, so the
    table answers -- with nothing -- without one.  Then it is used again.  The same for clear()."""
    F, ctx = env
    t, m = F.Table(ctx), T.Model()
    try:
        t.set_segment_rows(256)
        k, s, o = _unique_rows(600)
        for x in (t, m):
            x.insert(k, s, o)
            x.finalize()
        assert t.segments() >= 3
        for x in (t, m):
            x.insert(k, s, o)
            x.finalize()
        _checkpoint(t, m, 7)
        deleted = set(m.visible)
        ids = np.arange(0, 64, dtype=np.uint32)
        assert t.delete_songs(ids) == m.delete_songs(ids)[0] == 600
        assert t.segments() == 0 and t.rows() == (0, 0)
        _checkpoint(t, m, 8, deleted=deleted, gone_sid=7, checkpoint=3)
        lk, ls, lo = t.lookup(k[:50])
        assert len(lk) == len(ls) == len(lo) == 0
        res = t.match(k[:100], o[:100], np.array([0, 100], np.uint64), 3)
        assert not any(res[name].any() for name in ("sid", "delta", "aligned", "dedup", "nres", "npairs"))
        for x in (t, m):
            x.insert(k[:1], s[:1], o[:1])
            x.finalize()
        _checkpoint(t, m, 9, deleted=deleted - m.visible)
        # clear() from the same state: frozen segments only
        for x in (t, m):
            x.clear()
            x.insert(k, s, o)
            x.finalize()
            x.insert(k, s, o)
            x.finalize()
            x.clear()
        assert t.segments() == 0
        _checkpoint(t, m, 10)
    finally:
        t.close()


def test_fresh_table_still_refuses(env):
    """what the empty-table state must not loosen: a table nobody finalized does not answer, deleted from or cleared"""
    F, ctx = env
    t = F.Table(ctx)
    try:
        for step in (lambda: None, lambda: t.delete_songs([1]), t.clear):
            step()
            with pytest.raises(F.ShzError) as e:
                t.lookup(np.array([1], np.uint32))
            assert e.value.code == F.E_STATE
    finally:
        t.close()


def test_ids_outgrow_the_packing_while_runs_wait(env):
    """A sealed run of narrow rows waits; the next rows need 21 + 21 bits.  Today's promise: finalize refuses
    (SHZ_E_UNSUPPORTED), no row is lost or made visible, clear() brings the table back."""
    F, ctx = env
    t, m = F.Table(ctx), T.Model()
    try:
        k, s, o = _unique_rows(800)
        t.insert(k, s, o)
        t.seal_run()
        t.insert(k[:10], np.full(10, 1 << 20, np.uint32), np.full(10, 1 << 20, np.uint32))
        before = t.rows()
        assert before == (0, 810)
        with pytest.raises(F.ShzError) as e:
            t.finalize()
        assert e.value.code == F.E_UNSUPPORTED
        assert t.rows() == before
        t.clear()
        assert t.rows() == (0, 0)
        for x in (t, m):
            x.insert(k, s, o)
            x.seal_run()
            x.insert(*_unique_rows(300, first=500))
            x.finalize()
        _checkpoint(t, m, 11)
    finally:
        t.close()


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("profile", ("tiny_segments", "runs"))
def test_sharded_table_walks_the_same_states(env, profile, seed):
    """ShardedTable(nshards=3) and a plain Table take the same operations and meet the same model at every checkpoint
    (rows, export as a set, song_rows, lookup, match; the plain table also segments and song_hashes)."""
    F, ctx = env
    from shazam_amd.shard import ShardedTable
    t, st = F.Table(ctx), ShardedTable(ctx, nshards=3)
    try:
        T.drive([t, st], T.sequence(seed, profile), seed, ("sharded", profile, seed), full=(True, False))
    finally:
        t.close()
        st.close()


@pytest.mark.parametrize("profile", ("runs", "tiny_segments"))
def test_a_life_leaves_no_memory_behind(env, profile):
    """one sequence three times, each on a fresh table that is closed: the first warms the workspace, the third must leave
    what the second left (the margin of test_gpu_bulk_build.py)"""
    F, ctx = env
    ops = T.sequence(1, profile)
    free = []
    for rep in range(3):
        _run(F, ctx, ops, 1, (profile, "repetition", rep))
        ctx.sync()
        free.append(ctx.mem_info()[0])
    assert abs(free[2] - free[1]) < (8 << 20), free
