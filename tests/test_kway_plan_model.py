"""No GPU: the built inputs of test_gpu_kway_built.py reach the paths of the k-way merge they were built for, and the
uniformly random equal runs of the older tests do not -- measured on the numpy model of the merge's plan
(kway_cases.plan_model: sample stride, sorted samples, lower-bound shares per tile and run; kway_cases.thread_regions: the
merge regions one thread's outputs touch in the first round of kw_tile_kernel).  The model's constants are copied from
shz_build.hip in one place (kway_cases.KW_*): when the plan changes, these guards fail and name what to revisit."""
import numpy as np
import pytest

import kway_cases as K


def _plan(runs, piece_rows=K.SEG_ROWS_DEFAULT):
    return K.plan_model([K.sealed(r) for r in runs], piece_rows)


def test_pack_and_rows_of_are_inverse_and_expected_is_unique_of_packed():
    rng = np.random.default_rng(0)
    for ob in (1, 12, 20, 31):
        k = rng.integers(0, 1 << 32, 500).astype(np.uint32)
        s = rng.integers(0, 1 << (32 - ob), 500).astype(np.uint32)
        o = rng.integers(0, 1 << ob, 500).astype(np.uint32)
        v = K.pack(k, s, o, ob)
        assert v.dtype == np.uint64 and all(np.array_equal(a, b) for a, b in zip(K.rows_of(v, ob), (k, s, o)))
        # numeric order of the packed rows = lexicographic order of (key, sid, off)
        idx = np.lexsort((o, s, k))
        assert np.array_equal(np.sort(v), v[idx])
    a = (np.array([5, 1, 5], np.uint32), np.array([2, 3, 2], np.uint32), np.array([4095, 0, 4095], np.uint32))
    b = (np.array([1, 0], np.uint32), np.array([3, 9], np.uint32), np.array([0, 7], np.uint32))
    ek, es, eo = K.expected([a, b, (a[0][:0],) * 3])
    assert ek.tolist() == [0, 1, 5] and es.tolist() == [9, 3, 2] and eo.tolist() == [7, 0, 4095]


def test_model_constants_match_the_source():
    """the constants the model copies are the ones shz_build.hip defines"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shazam_amd", "csrc", "shz_build.hip")).read()
    for name in ("KW_MAXK", "KW_THREADS", "KW_TILE_SMALL", "KW_TILE_LARGE"):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == getattr(K, name), name
    assert "kp2 <= %d ? KW_TILE_SMALL : KW_TILE_LARGE" % K.KW_SMALL_MAX_KP2 in src
    assert "piece_rows / %d" % K.KW_PIECE_DIV in src
    assert "TMAX = %d * TILE" % K.KW_BUF_TILES in src


def test_plan_of_a_small_example_by_hand():
    """3 runs under a piece of 64 rows: kp2 = 4, nominal = 8, M = 2, c = 4"""
    runs = [np.arange(0, 20, 2, dtype=np.uint64), np.array([3, 4, 4 + 1], np.uint64), np.array([100], np.uint64)]
    p = K.plan_model(runs, 64)
    assert (p.k, p.kp2, p.tile, p.nominal, p.M, p.c) == (3, 4, K.KW_TILE_SMALL, 8, 2, 4)
    assert p.samples.tolist() == [0, 3, 4, 5, 8, 12, 16, 100] and p.ntiles == 2 and p.split.tolist() == [8]
    assert p.bounds.tolist() == [[0, 0, 0], [4, 3, 0], [10, 3, 1]]
    assert p.tile_rows.tolist() == [7, 7]
    assert K.thread_regions(p).tolist() == [1, 1]          # one row a thread


@pytest.mark.parametrize("k", [16, 32])
def test_random_equal_runs_reach_neither_several_regions_nor_full_tiles(k):
    p = _plan(K.old_random_runs(k, k))
    assert K.thread_regions(p).max() <= 2
    assert K.fill(p) < 1.5 and -(-int(p.tile_rows.max()) // K.KW_THREADS) <= 11
    assert len(p.split) and K.splitter_ties(p).max() == 1


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("big_pos", [0, 15, 31])
def test_skewed_runs_make_a_thread_cross_several_regions(big_pos, dedup):
    runs = K.skewed_runs(big_pos, big_pos, dedup)
    p = _plan(runs)
    assert p.k == 32 and K.holds_layout(runs)
    assert K.thread_regions(p).max() >= 3
    assert p.tile_rows.max() <= p.buf_rows


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("k", [8, 16, 32])
def test_comb_fills_a_tile(k, dedup):
    runs = K.comb_runs(k, dedup)
    p = _plan(runs)
    assert p.k == p.c == k and p.M == p.tile // k and K.holds_layout(runs)
    assert K.fill(p) >= 1.8
    assert p.tile_rows.max() == K.comb_full_tile_rows(k) <= p.buf_rows
    if k == 32:
        assert -(-int(p.tile_rows.max()) // K.KW_THREADS) == 16       # outputs a thread (the random runs reach 11)


@pytest.mark.parametrize("k", [2, 16, 17, 32])
def test_same_rows_in_every_run_tie_all_samples_at_every_splitter(k):
    runs = K.same_rows_runs(k, k)
    p = _plan(runs)
    ties = K.splitter_ties(p)
    assert p.k == k and len(ties) >= 1 and (ties == k).all() and K.holds_layout(runs)
    assert p.tile_rows.max() <= p.buf_rows


@pytest.mark.parametrize("M, more", [(128, 0), (64, 13)])
def test_stride_runs_have_the_lengths_around_the_stride(M, more):
    for dedup in (False, True):
        runs, lens = K.stride_runs(M, M, dedup, more)
        p = _plan(runs)
        assert p.M == M and [len(K.sealed(r)) for r in runs] == lens and K.holds_layout(runs)
        assert {1, M - 1, M, M + 1, 2 * M, 2 * M + 1, 5000} <= set(lens)


def test_every_other_built_case_holds_the_layout_and_stays_inside_the_buffer():
    cases = [K.random_runs(3, K.run_sizes(3, 32), True), K.random_runs(4, K.run_sizes(4, 17), False),
             K.disjoint_runs(5, 32, True, False), K.disjoint_runs(6, 5, False, True), K.same_pairs_runs(7, 17),
             K.one_key_runs(8, 32, True), K.one_key_runs(9, 16, False), K.single_row_runs(10, 32, 0, True),
             K.single_row_runs(11, 31, 5000, False), K.range_end_runs(12)]
    for runs in cases:
        p = _plan(runs)
        assert K.holds_layout(runs) and p.tile_rows.max() < p.buf_rows and p.tile_rows.sum() == sum(len(K.sealed(r)) for r in runs)
    lo_hi = K.sealed(K.range_end_runs(12)[2])
    assert lo_hi[0] == 0 and lo_hi[-1] == np.uint64(0xFFFFFFFFFFFFFFFF)


def test_inverted_rows_hold_one_inversion_under_one_key():
    n = 1000
    for at in (0, 255, n - 2):
        k, s, o = K.inverted_rows(at, n, at)
        lo = (s.astype(np.uint64) << np.uint64(K.OB)) | o
        assert np.flatnonzero(lo[1:] < lo[:-1]).tolist() == [at] and k[at] == k[at + 1]
        assert K.holds_layout([(k, s, o)]) and len(K.sealed((k, s, o))) == n
        # a stable sort on the key alone leaves the pair in the wrong order
        assert not np.array_equal(K.pack(k, s, o)[np.argsort(k, kind="stable")], K.sealed((k, s, o)))
    k, s, o = K.descending_key_rows(1, n)
    lo = (s.astype(np.uint64) << np.uint64(K.OB)) | o
    assert not (lo[1:] < lo[:-1]).any() and (k[1::2] < k[::2]).all() and (lo[1::2] == lo[::2]).all()
    assert np.array_equal(K.pack(k, s, o)[np.argsort(k, kind="stable")], K.sealed((k, s, o)))
