"""GPU: the k-way run merge of the bulk build (shz_build.hip: the plan kernels kw_sample / kw_bounds / kw_tile_rows /
kw_cuts, the five modes and two tile sizes of kw_tile_kernel, the seal in front of them and kway_merge / collapse_runs /
flush_runs around them) on BUILT runs -- skewed, comb-shaped, tied, at the run counts and run lengths where the code
switches -- against numpy: the table is np.unique over the packed rows of all runs (kway_cases.expected), exactly.

Runs are blocks of finalize_runs (block r = run r, empty blocks make no run) or seal_run calls where a case says so.
Where ONE merge builds the table the exported columns equal the expected rows in order, across segments too; where
several flushes build it the rows are compared as a set, each row once, sorted inside every stretch a flush wrote.
The guards (numpy model of the plan, kway_cases.plan_model) only assert that a case reaches the path it was built for;
test_kway_plan_model.py asserts the same guards without a GPU, and that the older tests' random runs do not meet them.

What the tie cases can and cannot see.  Tied rows are equal 64-bit values, so HOW a tie is broken leaves no trace in a
table as long as it is broken alike for every run: `<` for `<=` in the diagonal search of kw_tile_kernel still starts
every thread on a valid point of the merge path (the serial merge then emits the same values), and `<=` for `<` in
kw_bounds_kernel moves the copies of a splitter's value to the tile before, all of them.  Both were built and run: all
tests here pass under either.  What the tie cases do catch is copies of one value parted between tiles (kw_bounds
breaking the tie by the run's parity): 31 tests here fail, among them every same-rows, one-key/shared-sid and
clustered-duplicates case."""
import numpy as np
import pytest

import kway_cases as K

pytestmark = pytest.mark.gpu

RUN_COUNTS = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 40, 65]
DEDUP = pytest.mark.parametrize("dedup", [False, True], ids=["own_sids", "shared_sids"])


@pytest.fixture(scope="module")
def env():
    from shazam_amd import _ffi
    return _ffi, _ffi.Context(0)


def _plan(runs, piece_rows=K.SEG_ROWS_DEFAULT):
    return K.plan_model([K.sealed(r) for r in runs], piece_rows)


def _exact(t, want):
    """one merge built the table: the exported columns ARE the expected rows, in order"""
    got = t.export()
    assert t.rows() == (len(want[0]), 0)
    for name, g, w in zip(("key", "sid", "off"), got, want):
        assert g.dtype == w.dtype and len(g) == len(w), name
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (name, len(bad), int(bad[0]), g[bad[0]:bad[0] + 4], w[bad[0]:bad[0] + 4])
    return got


def _build(env, runs, seg_rows=None):
    """the runs as blocks of one finalize_runs; -> (table, expected columns)"""
    F, ctx = env
    assert K.holds_layout(runs)
    k, s, o, sizes = K.staged(runs)
    t = F.Table(ctx)
    if seg_rows:
        t.set_segment_rows(seg_rows)
    t.insert(k, s, o)
    t.finalize_runs(sizes)
    return t, K.expected(runs)


def _check_one_merge(env, runs, seg_rows=None):
    t, want = _build(env, runs, seg_rows)
    try:
        _exact(t, want)
        if not seg_rows:
            assert t.segments() == 1
        return t.segments(), len(want[0])
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------- run counts
@DEDUP
@pytest.mark.parametrize("k", RUN_COUNTS)
def test_run_counts_with_unequal_lengths(env, k, dedup):
    """every count around the switches: 16 / 17 (tile size), 32 / 33 (KW_MAXK: beyond it the smallest runs are merged
    first, packed, modes 3 / 4), 65 (two collapses).  Disjoint song ids: modes 0 / 3; shared ones with repeated rows: 1 / 2 / 4."""
    runs = K.random_runs(100 + k, K.run_sizes(k, k), dedup)
    if dedup and k > 1:
        assert len(K.expected(runs)[0]) < sum(len(K.sealed(r)) for r in runs)      # rows do repeat across runs
    _check_one_merge(env, runs)


def test_empty_blocks_make_no_run(env):
    sizes = K.run_sizes(7, 40)
    for r in (0, 5, 6, 20, 39):
        sizes[r] = 0
    _check_one_merge(env, K.random_runs(7, sizes, True))


# ---------------------------------------------------------------------------------------------------------- skew / comb
@DEDUP
@pytest.mark.parametrize("big_pos", [0, 15, 31])
def test_skewed_runs(env, big_pos, dedup):
    """60,000 rows beside 31 runs of 96: a thread's outputs cross several merge regions and step over empty ones"""
    runs = K.skewed_runs(big_pos, big_pos, dedup)
    p = _plan(runs)
    assert p.k == 32 and K.thread_regions(p).max() >= 3
    _check_one_merge(env, runs)


@DEDUP
@pytest.mark.parametrize("k", [8, 16, 32])
def test_comb_fills_tiles(env, k, dedup):
    """tiles of 1.87 / 1.92 / 1.95 x TILE rows (4,001 rows, 16 outputs a thread at k = 32)"""
    runs = K.comb_runs(k, dedup)
    p = _plan(runs)
    assert K.fill(p) >= 1.8 and p.tile_rows.max() == K.comb_full_tile_rows(k)
    _check_one_merge(env, runs)


@DEDUP
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "run0_largest"])
@pytest.mark.parametrize("k", [5, 32])
def test_disjoint_value_ranges(env, k, descending, dedup):
    """run r holds only keys of range r: in a tile most shares are empty, and the merged table is the runs laid end to end"""
    runs = K.disjoint_runs(200 + k, k, descending, dedup)
    ends = [(int(v[0]), int(v[-1])) for v in (K.sealed(r) for r in runs)]
    if descending:
        ends = ends[::-1]
    assert all(a[1] < b[0] for a, b in zip(ends, ends[1:]))
    _check_one_merge(env, runs)


# ---------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("k", [2, 16, 17, 32])
def test_every_run_holds_the_same_rows(env, k):
    runs = K.same_rows_runs(k, k)
    p = _plan(runs)
    ties = K.splitter_ties(p)
    assert len(ties) >= 1 and (ties == k).all()             # all k samples tie at every splitter
    t, want = _build(env, runs)
    try:
        assert len(want[0]) == len(runs[0][0])              # the table is one copy
        _exact(t, want)
    finally:
        t.close()


@pytest.mark.parametrize("k", [2, 16, 17, 32])
def test_every_run_holds_the_same_pairs_under_its_own_sid(env, k):
    runs = K.same_pairs_runs(300 + k, k)
    t, want = _build(env, runs)
    try:
        assert len(want[0]) == k * len(runs[0][0])          # nothing is dropped
        got = _exact(t, want)
        assert (got[1].reshape(-1, k) == np.arange(1, k + 1)).all()   # groups of k neighbours differ in the sid only
    finally:
        t.close()


@DEDUP
@pytest.mark.parametrize("k", [3, 16, 32])
def test_one_key_for_all_rows(env, k, dedup):
    runs = K.one_key_runs(400 + k, k, dedup)
    assert len(np.unique(np.concatenate([r[0] for r in runs]))) == 1
    _check_one_merge(env, runs)


# ---------------------------------------------------------------------------------------------------------- stride edges
@DEDUP
@pytest.mark.parametrize("M, more", [(128, 0), (64, 13)], ids=["k7_M128", "k20_M64"])
def test_run_lengths_around_the_sample_stride(env, M, more, dedup):
    """runs of 1, M - 1, M, M + 1, 2 M, 2 M + 1 rows beside one of 5,000"""
    runs, lens = K.stride_runs(M, M, dedup, more)
    p = _plan(runs)
    assert p.M == M and [len(K.sealed(r)) for r in runs] == lens
    _check_one_merge(env, runs)


@DEDUP
@pytest.mark.parametrize("singles, big", [(32, 0), (31, 5000)])
def test_runs_of_one_row(env, singles, big, dedup):
    runs = K.single_row_runs(500 + singles, singles, big, dedup)
    assert len(runs) == 32 and sorted(len(r[0]) for r in runs)[:31] == [1] * 31
    _check_one_merge(env, runs)


def test_both_ends_of_the_packed_range(env):
    """row (0, 0, 0) and the row whose packed value is 2^64 - 1, in different runs and together in one"""
    runs = K.range_end_runs(600)
    t, want = _build(env, runs)
    try:
        assert (want[0][0], want[1][0], want[2][0]) == (0, 0, 0)
        assert (want[0][-1], want[1][-1], want[2][-1]) == (0xFFFFFFFF, (1 << (32 - K.OB)) - 1, (1 << K.OB) - 1)
        _exact(t, want)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------- segments
@pytest.mark.parametrize("dups", [False, True], ids=["no_dups", "clustered_dups"])
@pytest.mark.parametrize("k", [3, 32])
@pytest.mark.parametrize("L", [16, 256, 1000])
def test_segments_of_one_merge_follow_each_other_in_order(env, L, k, dups):
    """pieces of at most L rows cut from ONE merge: the export is globally ordered, across the segments.  Pieces are
    whole tiles taken greedily; for L >= 8 kp2 a tile stays below 3 L / 8 rows, so no piece outgrows L and every piece
    but the last holds more than L - 3 (L / 8) rows: both bound segments().  (About 8 L rows: even at L = 16 and k = 3,
    where a tile may hold up to 11 rows and a piece as few as 5, the table stays within its 32 segments.)"""
    rng = np.random.default_rng(L + k)
    total = 8 * L
    w = rng.integers(1, 8, k).astype(np.float64)
    sizes = np.maximum(1, (w / w.sum() * total).astype(int)).tolist()
    runs = K.random_runs(700 + L + k, sizes, False)
    if dups:   # every run also holds one block of rows, all inside a narrow key range: the duplicates sit in one piece
        block = K.draw(rng, max(L // 4, 4), 200, 240, keys=(np.uint64(1 << 15) << np.uint64(8)) | np.arange(4, dtype=np.uint64))
        runs = [tuple(np.concatenate([a, b]) for a, b in zip(r, K.rows_of(rng.permutation(block)))) for r in runs]
    t, want = _build(env, runs, seg_rows=L)
    try:
        _exact(t, want)
        n, segs = len(want[0]), t.segments()
        assert -(-n // L) <= segs <= K.MAX_SEGS
        p = _plan(runs, L)
        if L >= 8 * p.kp2:
            assert p.nominal == L // 8 and p.tile_rows.max() < 3 * p.nominal
            assert segs <= 1 + (n - 1) // (L - 3 * p.nominal + 1)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------- flushes
def _check_flushed(t, runs, max_restarts):
    """several flushes built the table: every row once, and sorted inside every stretch one flush wrote"""
    want = K.pack(*K.expected(runs))
    got = K.pack(*t.export())
    assert t.rows() == (len(want), 0) and len(got) == len(want)
    assert np.array_equal(np.sort(got), want)
    restarts = np.flatnonzero(got[1:] <= got[:-1])
    assert len(restarts) <= max_restarts, restarts
    return restarts


@pytest.mark.parametrize("case", ["skewed", "skewed_many_runs", "tied_own_sids", "tied_shared_sids"])
def test_leftover_of_a_flush_that_is_not_final(env, case):
    """three seal_run calls under a segment limit the second one crosses: full segments are cut there and the leftover
    goes back to the arena as ONE packed run (modes 3 / 4), which finalize merges with the third run"""
    F, ctx = env
    rng = np.random.default_rng(len(case))
    if case.startswith("skewed"):     # 5,000 rows, then 96 (a third of them rows of the first seal in the shared-sid case)
        L = 5040
        a, b, c = K.random_runs(800, [5000, 96, 700], case == "skewed_many_runs")
    elif case == "tied_own_sids":     # the same (key, offset) pairs under three song ids: nothing repeats
        L = 2048
        a, b, c = K.same_pairs_runs(801, 3, n=1500)
    else:                              # rows of the first seal again in the second and third, beside new ones
        L = 2048
        va = K.draw(rng, 2000, 1, 40, top=True)
        vb = K.mixed(rng, 2800, va, 1, 40, share=0.1)
        vc = K.mixed(rng, 900, np.unique(np.r_[va, vb]), 1, 40, share=0.5)
        a, b, c = (K.rows_of(v) for v in (va, vb, vc))
    assert K.holds_layout([a]) and len(a[0]) < L <= len(K.expected([a, b])[0]) - 8    # the second seal crosses L, rows are left
    t = F.Table(ctx)
    try:
        t.set_segment_rows(L)
        if case == "skewed_many_runs":
            t.set_run_rows(128)        # every seal cuts runs of 128 rows: beyond KW_MAXK runs the smallest are merged first
        t.insert(*a)
        t.seal_run()
        assert t.rows() == (0, len(a[0]))
        t.insert(*b)
        t.seal_run()
        visible, waiting = t.rows()
        assert L - 3 * (L // 8) < visible <= t.segments() * L                       # segments were cut ...
        assert waiting > 0 and visible + waiting == len(K.expected([a, b])[0])      # ... and the leftover waits, each row once
        t.insert(*c)
        t.seal_run()
        t.finalize()
        _check_flushed(t, [a, b, c], max_restarts=2)                                # a flush at the 2nd seal, the 3rd, finalize
        assert t.segments() >= -(-t.rows()[0] // L)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------- seal
@pytest.mark.parametrize("at", [0, 255, -2], ids=["rows_0_1", "rows_255_256", "last_two_rows"])
def test_seal_of_ordered_rows_with_one_inversion(env, at):
    """run_pack_kernel must see the one row that sorts before its predecessor: the pair shares its key, so the short sort
    on the key bits alone would leave it in arrival order"""
    F, ctx = env
    n = 1000
    cols = K.inverted_rows(900 + at, n, at % n)
    t = F.Table(ctx)
    try:
        t.insert(*cols)
        t.finalize()
        _exact(t, K.expected([cols]))
    finally:
        t.close()


def test_seal_of_ordered_rows_with_equal_sid_off_under_descending_keys(env):
    F, ctx = env
    cols = K.descending_key_rows(950, 1000)
    t = F.Table(ctx)
    try:
        t.insert(*cols)
        t.finalize()
        _exact(t, K.expected([cols]))
    finally:
        t.close()
