"""GPU: shz_scan_warps with a per-window selection -- every window tries a list of warps of its own, only the listed
(window, warp) pairs become queries of the match -- against the host recipe restricted to the selection (tests/
scan_warp_twin.py): a full selection is the dense call; random lists with empty ones at the front, in the middle and at the
end of a recording, a recording without a slot and a call without any; the same under small slices, where a 2-warp chunk
cuts through the lists; the two work counts; what is refused about a selection."""
import numpy as np
import pytest

import scan_warp_cases as SC
import scan_warp_twin as SW

pytestmark = pytest.mark.gpu

SR = SC.SR
T16 = np.asarray([62259, 68813, 65536, 68813, 62259, 65536, 40000], np.uint32)
F16 = np.asarray([62259, 62259, 65536, 68813, 68813, 67468, 65536], np.uint32)
K = len(T16)


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def songs():
    return SC.songs()


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    d, table = SC.make_db(S, ctx, songs)
    yield d, table
    d.close()


@pytest.fixture(scope="module")
def batch(songs):
    """Four recordings with windows (one of them stereo with channels of unequal length), one without clips between them."""
    a = songs[1][SR:SR + 4096 + 69 * 2048]              # 70 frames
    b = songs[2][2 * SR:2 * SR + 4096 + 49 * 2048]      # 50 frames
    return [a, [], [b, b[:40000]], songs[3][:4096 + 39 * 2048], songs[0][5 * SR:5 * SR + 4096 + 44 * 2048]]


WINDOW, STEP = 20, 8
COUNTS = [8, 0, 5, 4, 5]                                # windows per recording: 22 in all


def _csr(lists):
    so = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    sw = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if so[-1] else np.zeros(0, np.uint32)
    return so, sw.astype(np.uint32)


def _random_lists(seed):
    """Per window a random ascending sub-list; the first, a middle and the last window of recording 0 and the first window of
    recording 2 try nothing, recording 3 has no slot at all, and warp 5 is never tried."""
    def make(n_wins):
        assert n_wins == sum(COUNTS)
        rng = np.random.default_rng([0x5E1, seed])
        lists = [np.flatnonzero(rng.random(K) < 0.5) for _ in range(n_wins)]
        lists = [x[x != 5] for x in lists]
        for w in (0, 3, 4, 7, 8, 13, 14, 15, 16):
            lists[w] = np.zeros(0, np.int64)
        lists[1], lists[21] = np.asarray([0, 1, 2, 3, 4, 6]), np.asarray([6])
        return _csr(lists)
    return make


def test_a_full_selection_is_the_dense_call(S, ctx, db, batch):
    from shazam_amd import _ffi
    d, _ = db
    _, pcm, off, first = SC.flatten(S, batch)
    for debug in (0, _ffi.DEBUG_SCAN_SPEED_SMALL_SLICES):
        for topn in (1, 3):
            want, wo, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, topn=topn)
            n = int(wo[-1])
            assert np.diff(wo.astype(np.int64)).tolist() == COUNTS
            ctx.set_debug(debug)
            try:
                got, wo1, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, SW.full_selection(n, K), topn=topn)
            finally:
                ctx.set_debug(0)
            assert np.array_equal(wo, wo1) and got["profile"].shape == (n * K,)
            got["profile"] = got["profile"].reshape(n, K)
            SC.same(got, want, ("full selection", debug, topn))
            assert got["work"] == want["work"] and want["nres"].any()


@pytest.mark.parametrize("seed", range(3))
def test_random_selections_equal_the_restricted_recipe(S, ctx, db, batch, seed):
    from shazam_amd import _ffi
    d, _ = db
    for debug in (0, _ffi.DEBUG_SCAN_SPEED_SMALL_SLICES):     # small slices: 2-warp chunks cut through the lists
        ctx.set_debug(debug)
        try:
            got, win_off = SC.check(S, d, batch, WINDOW, STEP, T16, F16, _random_lists(seed), topns=(1, 2),
                                    full_sorts=(False, True) if seed == 0 else (False,), what=("random lists", seed, debug))
        finally:
            ctx.set_debug(0)
        assert np.diff(win_off.astype(np.int64)).tolist() == COUNTS
        so, _ = _random_lists(seed)(sum(COUNTS))
        empty = np.flatnonzero(np.diff(so.astype(np.int64)) == 0).tolist()
        assert set(empty) >= {0, 3, 4, 7, 8, 13, 14, 15, 16}
        assert (got["best"][empty] == _ffi.SCAN_NO_WARP).all() and not got["nres"][empty].any() and not got["aligned"][empty].any()
        assert (np.delete(got["best"], empty) != _ffi.SCAN_NO_WARP).all() and 5 not in got["best"].tolist()
        assert got["nres"].any()


def test_a_call_without_any_slot_extracts_nothing(S, ctx, db, batch):
    from shazam_amd import _ffi
    d, _ = db
    _, pcm, off, first = SC.flatten(S, batch)
    n = sum(COUNTS)
    before = (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats())
    got, wo, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, (np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32)))
    assert (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats()) == before
    assert np.diff(wo.astype(np.int64)).tolist() == COUNTS and got["work"] == (0, 0) and got["profile"].shape == (0,)
    assert (got["best"] == _ffi.SCAN_NO_WARP).all() and len(got["best"]) == n
    for name in SC.ARRAYS:
        assert not got[name].any(), name


def test_work_counts_what_a_selection_saves(S, ctx, db, batch):
    d, _ = db
    _, pcm, off, first = SC.flatten(S, batch)
    n = sum(COUNTS)
    dense, _, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16)
    single, _, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16[3:4], F16[3:4])
    sel = (np.arange(n + 1, dtype=np.uint64), np.full(n, 3, np.uint32))          # every window tries warp 3 alone
    got, _, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, sel)
    assert got["work"] == single["work"] and 0 < got["work"][0] < dense["work"][0] and 0 < got["work"][1] < dense["work"][1]
    assert (got["best"] == 3).all() and np.array_equal(got["profile"], single["profile"][:, 0])
    SC.same(got, single, "one warp for every window", SC.ARRAYS)
    # the twin's counts: hashes over the warps in use only, cut entries over the slots only (SC.check compares both)
    _, _ = SC.check(S, d, batch, WINDOW, STEP, T16, F16, lambda m: sel, what="warp 3 alone")


def test_selection_refusals_launch_nothing(S, ctx, db, batch):
    from shazam_amd import _ffi
    import ctypes as C
    d, _ = db
    _, pcm, off, first = SC.flatten(S, batch)
    n = sum(COUNTS)
    so, sw = _random_lists(1)(n)
    want, _, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, (so, sw))
    before = (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats(), d.table.rows(), ctx.mem_info()[0])

    def edit(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    first_slot = int(so[1])                                # window 1 lists 0 1 2 3 4 6
    for what, s_off, s_warp, says in (
            ("sel_off[0] != 0", edit(so, 0, 1), sw, "sel_off[0]"),
            ("a decreasing sel_off", edit(so, 5, int(so[4]) - 1), sw, "decreases"),
            ("a list that repeats a warp", so, edit(sw, first_slot + 1, int(sw[first_slot])), "ascending"),
            ("a list that descends", so, edit(sw, first_slot + 2, 0), "ascending"),
            ("an index of n_warps", so, edit(sw, first_slot + 5, K), f"warp {K}")):
        with pytest.raises(_ffi.ShzError) as e:
            ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, (s_off, s_warp))
        assert e.value.code == _ffi.E_INVALID and says in str(e.value), (what, str(e.value))
    # a sel_off for more or fewer windows than the call has: refused by the wrapper, which counts the windows first
    for s_off in (np.append(so, so[-1]), so[:-1]):
        with pytest.raises(ValueError, match=f"{len(s_off)} entries for {n} windows"):
            ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, (s_off, sw))
    with pytest.raises(ValueError, match=f"for {n} windows"):
        ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, (np.append(so, so[-1]), sw), cap_windows=n + 1)
    # exactly one of the two pointers NULL: through the raw ABI
    res = _ffi._match_result(n, 2)
    best, wo, cnt = np.zeros(n, np.uint32), np.zeros(len(first), np.uint64), C.c_uint64()
    for a, b in ((so.ctypes.data_as(_ffi.u64p), None), (None, sw.ctypes.data_as(_ffi.u32p))):
        rc = _ffi.lib().shz_scan_warps(ctx.h, d.table.h, _ffi.ptr(pcm), off.ctypes.data_as(_ffi.u64p), len(off) - 1,
                                       first.ctypes.data_as(_ffi.u32p), len(first) - 1, SR, 10.0, 5, WINDOW, STEP, 2,
                                       T16.ctypes.data_as(_ffi.u32p), F16.ctypes.data_as(_ffi.u32p), K, a, b, 0,
                                       wo.ctypes.data_as(_ffi.u64p), _ffi.ptr(best), _ffi.ptr(res["sid"]), _ffi.ptr(res["delta"]),
                                       _ffi.ptr(res["aligned"]), _ffi.ptr(res["dedup"]), _ffi.ptr(res["nres"]), None, None, None, None,
                                       n, C.byref(cnt), None, None, None, None)
        assert rc == _ffi.E_INVALID and b"go together" in (_ffi.lib().shz_last_error(ctx.h) or b"")
    assert (ctx.spec_stats(), ctx.extract_stats(), d.table.match_stats(), d.table.rows(), ctx.mem_info()[0]) == before
    got, _, _ = ctx.scan_warps(d.table, pcm, off, first, WINDOW, STEP, T16, F16, (so, sw))
    SC.same(got, want, "after the refusals")
