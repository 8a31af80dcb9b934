"""CPU: the song filter's definition (tests/song_filter_twin.py) against the unfiltered ranking, what the three C entries
refuse on a NULL context, and what Context.songs() refuses -- nothing here touches a device."""
import ctypes as C

import numpy as np
import pytest

from song_filter_twin import allowed_rows, expected_floor_sets, expected_match_sets
from vote_floor_twin import expected_floor
from vote_tol_twin import expected_match


def _random_votes(seed, n_songs=12, nq=4):
    """a table of few keys and small offsets, so that every (query, song) has several bins with several votes"""
    rng = np.random.default_rng(seed)
    keys = rng.choice(1 << 31, 24, replace=False).astype(np.uint32)
    n_rows = 400
    tk = keys[rng.integers(0, 24, n_rows)]
    ts = rng.integers(0, n_songs, n_rows).astype(np.uint32)
    to = rng.integers(0, 24, n_rows).astype(np.uint32)
    qk = keys[rng.integers(0, 24, 60 * nq)]
    qo = rng.integers(0, 24, 60 * nq).astype(np.uint32)
    return tk, ts, to, qk, qo, (np.arange(nq + 1) * 60).astype(np.uint64)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("tol", [0, 2])
def test_filtered_ranking_is_the_unfiltered_one_with_the_barred_songs_struck_out(seed, exclude, tol):
    n_songs, nq = 12, 4
    tk, ts, to, qk, qo, qoff = _random_votes(500 + seed, n_songs, nq)
    rng = np.random.default_rng(900 + seed)
    sets = [sorted(rng.choice(n_songs + 3, size=int(rng.integers(0, n_songs)), replace=False).tolist()) for _ in range(3)]
    set_of = [0, 2, 1, 2]
    full = expected_match(tk, ts, to, qk, qo, qoff, tol, n_songs)
    got = expected_match_sets(tk, ts, to, qk, qo, qoff, tol, n_songs, sets, set_of, exclude)
    rows = list(zip(tk.tolist(), ts.tolist(), to.tolist()))
    for q in range(nq):
        passes = lambda s: (s in sets[set_of[q]]) != exclude   # noqa: E731
        ranked, npairs, nhash = full[q]
        want = [r for r in ranked if passes(r[0])]
        assert got[q][0] == want, (q, got[q][0], want)
        assert got[q][2] == nhash                                        # the query's alone
        a, b = int(qoff[q]), int(qoff[q + 1])
        hs = set(zip(qk[a:b].tolist(), qo[a:b].tolist()))
        kept = sum(1 for k, s, o in set(rows) for hk, _ in hs if hk == k and passes(s))
        assert got[q][1] == kept <= npairs
    # with a smaller topn the filtered ranking is the head of that list, not a filtered head
    two = expected_match_sets(tk, ts, to, qk, qo, qoff, tol, 2, sets, set_of, exclude)
    assert all(two[q][0] == got[q][0][:2] for q in range(nq))


def test_twin_edges_and_floor():
    tk, ts, to, qk, qo, qoff = _random_votes(77)
    every = list(range(12))
    assert expected_match_sets(tk, ts, to, qk, qo, qoff, 1, 5, [every]) == expected_match(tk, ts, to, qk, qo, qoff, 1, 5)
    assert expected_match_sets(tk, ts, to, qk, qo, qoff, 1, 5, [[]], exclude=True) == expected_match(tk, ts, to, qk, qo, qoff, 1, 5)
    none = expected_match_sets(tk, ts, to, qk, qo, qoff, 0, 5, [[]])
    plain = expected_match(tk, ts, to, qk, qo, qoff, 0, 5)
    assert [(r, n) for r, n, _ in none] == [([], 0)] * 4 and [h for *_, h in none] == [h for *_, h in plain]
    assert allowed_rows(ts, [3, 3, 99], False).sum() == (ts == 3).sum()
    sh, bh = expected_floor_sets(tk, ts, to, qk, qo, qoff, 0, [every])
    sh0, bh0 = expected_floor(tk, ts, to, qk, qo, qoff, 0)
    assert np.array_equal(sh, sh0) and np.array_equal(bh, bh0)
    sh, bh = expected_floor_sets(tk, ts, to, qk, qo, qoff, 0, [[2], every], [0, 1, 0, 1])
    assert np.array_equal(sh[1::2], sh0[1::2]) and np.array_equal(bh[1::2], bh0[1::2])
    assert (sh[0::2].sum(axis=1) <= 1).all()                             # one song left: one entry of the song histogram


def test_null_context_is_refused():
    from shazam_amd import _ffi
    L = _ffi.lib()
    ids, off = np.array([1, 2], np.uint32), np.array([0, 2], np.uint64)
    assert L.shz_set_song_filter(None, _ffi.ptr(ids), _ffi.ptr(off), 1, 0) == _ffi.E_INVALID
    assert L.shz_set_song_filter(None, None, None, 0, 0) == _ffi.E_INVALID
    n, f, k = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    assert L.shz_get_song_filter(None, C.byref(n), C.byref(f), C.byref(k)) == _ffi.E_INVALID
    assert (n.value, f.value, k.value) == (7, 7, 7)
    m = np.zeros(1, np.uint32)
    assert L.shz_match_batch_sets(None, None, None, None, None, 0, 2, 0, None, None, None, None, None, None, None,
                                  _ffi.ptr(m)) == _ffi.E_INVALID
    assert L.shz_match_device_host_sets(None, None, None, None, None, 0, 2, 0, -1, None, None, None, None, None, None, None,
                                        _ffi.ptr(m)) == _ffi.E_INVALID


def test_songs_refuses_only_and_exclude_together():
    from shazam_amd import _ffi
    ctx = _ffi.Context.__new__(_ffi.Context)      # no device: songs() refuses before it looks at the handle
    ctx.h = None
    with pytest.raises(ValueError):
        with ctx.songs(only=[1], exclude=[2]):
            pass
    with pytest.raises(ValueError):
        with ctx.songs(only=[1], sets=[[2]]):
            pass
    with ctx.songs():                              # all three None: the context stays as it is (no call is made)
        pass
    with ctx.songs(only=None, exclude=None, sets=None) as c:
        assert c is ctx
    assert [a.tolist() for a in _ffi._song_sets([3, 1, 3])] == [[3, 1, 3]]
    assert [a.tolist() for a in _ffi._song_sets([[3], (1, 2), range(2)])] == [[3], [1, 2], [0, 1]]
    assert [a.tolist() for a in _ffi._song_sets([])] == [[]]
    with pytest.raises(ValueError):
        _ffi._song_sets([-1])
