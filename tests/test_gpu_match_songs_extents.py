"""GPU: Table.match_songs_extents (shz_match_songs_extents), the catalogue form -- the listed songs' own rows, gathered on the
device, are the queries -- against the plain-Python definition (tests/extent_twin.py) on the songs read back with
Table.song_hashes and the table's export.  With and without SHZ_DEBUG_EXTENT_SMALL_TILES; every comparison is exact."""
import numpy as np
import pytest

from extent_twin import SCALARS, assert_extents, expected_extents

pytestmark = pytest.mark.gpu

A_ROWS, DELTA, LO, HI = 400, 37, 120, 219        # song 2 holds song 1's rows of the frames LO .. HI, shifted by DELTA


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def planted(S, ctx):
    """song 1: A_ROWS rows at the frames 0 .. 299; song 2: the rows of song 1 inside LO .. HI at off + DELTA, and 250 rows of its
    own on keys song 1 partly shares; song 3: unrelated rows; song 5: no rows"""
    rng = np.random.default_rng(9)
    ka = rng.integers(0, 5000, A_ROWS).astype(np.uint32)
    oa = rng.integers(0, 300, A_ROWS).astype(np.uint32)
    oa[:4] = (LO, HI, LO - 1, HI + 1)            # both ends of the stretch are occupied, and their neighbours outside it
    ins = (oa >= LO) & (oa <= HI)
    kb = np.concatenate([ka[ins], rng.integers(0, 5000, 250).astype(np.uint32)])
    ob = np.concatenate([oa[ins] + DELTA, rng.integers(0, 600, 250).astype(np.uint32)])
    kc, oc = rng.integers(0, 5000, 300).astype(np.uint32), rng.integers(0, 300, 300).astype(np.uint32)
    t = S.Table(ctx)
    t.insert(ka, 1, oa)
    t.insert(kb, 2, ob)
    t.insert(kc, 3, oc)
    t.finalize()
    yield t, int(ins.sum())
    t.close()


def _check(ctx, t, sids, cs, lo, hi, cn, what):
    from shazam_amd import _ffi
    tk, ts, to = t.export()
    ro, qk, qo = t.song_hashes(sids)
    cs, lo, hi = np.asarray(cs, np.uint32), np.asarray(lo, np.int32), np.asarray(hi, np.int32)
    want = expected_extents(tk, ts, to, qk, qo, ro, cs.tolist(), lo.tolist(), hi.tolist(), cn)
    out = None
    for flag in (0, _ffi.DEBUG_EXTENT_SMALL_TILES):
        ctx.set_debug(flag)
        try:
            res = t.match_songs_extents(sids, cs, lo, hi, cand_n=cn)
            bare = t.match_songs_extents(sids, cs, lo, hi, cand_n=cn, hist=False)
        finally:
            ctx.set_debug(0)
        assert_extents(res, want, (what, flag))
        for k in SCALARS + ("shift",):
            assert np.array_equal(bare[k], res[k]), (what, flag, k)
        out = res
    return out


def test_the_song_itself_at_delta_0_counts_its_own_rows(ctx, planted):
    t, _ = planted
    sids = [1, 2, 3, 5]
    ro, _, _ = t.song_hashes(sids, counts_only=True)
    rows = np.diff(ro.astype(np.int64))
    assert rows[3] == 0 and rows[:3].min() > 200
    r = _check(ctx, t, sids, [[s] for s in sids], [[0]] * 4, [[0]] * 4, None, "itself")
    assert r["count"][:, 0].tolist() == rows.tolist()
    _, k1, o1 = t.song_hashes([1])
    assert (int(r["q_first"][0, 0]), int(r["q_last"][0, 0])) == (int(o1.min()), int(o1.max())) == (int(r["t_first"][0, 0]), int(r["t_last"][0, 0]))


def test_a_planted_excerpt_gives_its_stretch_in_both_songs(ctx, planted):
    t, n_in = planted
    # listed in an order that is not the id order; song 1 asks for song 2 at DELTA, song 2 for song 1 at -DELTA
    r = _check(ctx, t, [2, 1], [[1, 3, 2], [2, 3, 1]], [[-DELTA, -300, 0], [DELTA, -300, 0]], [[-DELTA, 600, 0], [DELTA, 600, 0]],
               [3, 2], "excerpt")
    assert int(r["count"][1, 0]) >= n_in                                    # (chance pairs at DELTA can only add)
    assert (int(r["q_first"][1, 0]), int(r["q_last"][1, 0])) == (LO, HI)
    assert (int(r["t_first"][1, 0]), int(r["t_last"][1, 0])) == (LO + DELTA, HI + DELTA)
    assert int(r["count"][0, 0]) == int(r["count"][1, 0])                   # the same pairs seen from song 2
    assert (int(r["q_first"][0, 0]), int(r["q_last"][0, 0])) == (LO + DELTA, HI + DELTA)
    assert (int(r["t_first"][0, 0]), int(r["t_last"][0, 0])) == (LO, HI)
    assert not any(int(r[k][1, 2]) for k in SCALARS)                        # the slot past cand_n: zero, though it would match


def test_refusals(S, ctx, planted):
    from shazam_amd import _ffi
    t, _ = planted

    def code(*a, **k):
        with pytest.raises(_ffi.ShzError) as e:
            t.match_songs_extents(*a, **k)
        return e.value.code

    assert code([1, 2, 1], [[2], [1], [2]], [[0]] * 3, [[0]] * 3) == _ffi.E_INVALID          # a song id listed twice
    assert code([1, 2], [[2], [1]], [[1], [0]], [[0], [0]]) == _ffi.E_INVALID                # d_lo > d_hi
    assert code([1, 2], [[2], [1]], [[0], [0]], [[0], [0]], cand_n=[1, 2]) == _ffi.E_INVALID # cand_n above ncand
    assert code([1], np.zeros((1, 65), np.uint32), np.zeros((1, 65), np.int32), np.zeros((1, 65), np.int32)) == _ffi.E_INVALID
    L, p = _ffi.lib(), _ffi.ptr
    a = np.asarray([1], np.uint32)
    o = np.full(64, 0xABABABAB, np.uint32)
    z = np.zeros(1, np.int32)
    one = np.ones(1, np.uint32)
    assert L.shz_match_songs_extents(ctx.h, t.h, None, 1, 1, p(a), p(z), p(z), p(one), p(o), p(o), p(o), p(o), p(o), p(o), p(o)) == _ffi.E_INVALID
    assert L.shz_match_songs_extents(ctx.h, t.h, p(a), 1, 1, p(a), p(z), p(z), None, p(o), p(o), p(o), p(o), p(o), p(o), p(o)) == _ffi.E_INVALID
    assert L.shz_match_songs_extents(ctx.h, t.h, p(a), 1, 1, p(a), p(z), p(z), p(one), p(o), p(o), None, p(o), p(o), p(o), p(o)) == _ffi.E_INVALID
    assert L.shz_match_songs_extents(ctx.h, None, p(a), 1, 1, p(a), p(z), p(z), p(one), p(o), p(o), p(o), p(o), p(o), p(o), p(o)) == _ffi.E_INVALID
    assert L.shz_match_songs_extents(ctx.h, t.h, p(a), 0, 1, p(a), p(z), p(z), p(one), p(o), p(o), p(o), p(o), p(o), p(o), p(o)) == _ffi.OK
    assert (o == 0xABABABAB).all()
    # the state of the table; a listed song with an offset >= 2^20 (a query offset here); a table offset >= 2^31
    u = S.Table(ctx)
    u.insert(np.asarray([1, 2], np.uint32), 1, np.asarray([5, 1 << 20], np.uint32))
    u.insert(np.asarray([1], np.uint32), 2, np.asarray([9], np.uint32))

    def ucode(*a, **k):
        with pytest.raises(_ffi.ShzError) as e:
            u.match_songs_extents(*a, **k)
        return e.value.code

    assert ucode([2], [[1]], [[0]], [[0]]) == _ffi.E_STATE
    u.finalize()
    assert ucode([1], [[2]], [[0]], [[9]]) == _ffi.E_UNSUPPORTED
    r = u.match_songs_extents([2], [[1]], [[-4]], [[-4]])                   # (song 2 itself is fine as a query)
    assert (int(r["count"][0, 0]), int(r["q_first"][0, 0]), int(r["t_first"][0, 0])) == (1, 9, 5)
    u.insert(np.asarray([3], np.uint32), 3, np.asarray([1 << 31], np.uint32))
    u.finalize()
    assert ucode([2], [[1]], [[0]], [[0]]) == _ffi.E_UNSUPPORTED
    u.close()
