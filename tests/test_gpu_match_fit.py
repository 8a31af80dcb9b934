"""GPU: Table.match_extents(..., fit=True) (shz_match_extents_fit) -- the moments sum q, sum u, sum q^2, sum q u of every
candidate's pairs -- on tables and queries built by hand, against the plain-Python definition (tests/fit_twin.py); the other
outputs against shz_match_extents on the same inputs.  Every comparison is exact."""
from fractions import Fraction

import numpy as np
import pytest

from extent_twin import SCALARS
from fit_twin import SUMS, assert_moments, expected_moments

pytestmark = pytest.mark.gpu

QMAX = (1 << 20) - 1


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _table(S, ctx, rows):
    t = S.Table(ctx)
    tk, ts, to = (np.asarray([r[i] for r in rows], np.uint32) for i in range(3))
    t.insert(tk, ts, to)
    t.finalize()
    return t


def _query_arrays(queries):
    qk = np.asarray([h[0] for hs in queries for h in hs], np.uint32)
    qo = np.asarray([h[1] for hs in queries for h in hs], np.uint32)
    qoff = np.cumsum([0] + [len(hs) for hs in queries]).astype(np.uint64)
    return qk, qo, qoff


def _cand_arrays(cands, ncand=None):
    """per query a list of (sid, d_lo, d_hi) -> [n, ncand] arrays and cand_n; unused slots hold a candidate too wide for the
    sums, which is refused if it is read"""
    n = len(cands)
    ncand = ncand or max(1, max(len(c) for c in cands))
    cs, lo, hi = np.full((n, ncand), 1, np.uint32), np.full((n, ncand), -(1 << 30), np.int32), np.full((n, ncand), 1 << 30, np.int32)
    for q, c in enumerate(cands):
        for i, (s, a, b) in enumerate(c):
            cs[q, i], lo[q, i], hi[q, i] = s, a, b
    return cs, lo, hi, np.asarray([len(c) for c in cands], np.uint32)


def _check(ctx, t, queries, cands, what, ncand=None):
    """fit=True against the twin (sums) and against fit=False (everything else), at default and at small tiles"""
    from shazam_amd import _ffi
    tk, ts, to = t.export()
    qk, qo, qoff = _query_arrays(queries)
    cs, lo, hi, cn = _cand_arrays(cands, ncand)
    want = expected_moments(tk, ts, to, qk, qo, qoff, cs.tolist(), lo.tolist(), hi.tolist(), cn)
    out = None
    for flag in (0, _ffi.DEBUG_EXTENT_SMALL_TILES):
        ctx.set_debug(flag)
        try:
            res = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn, fit=True)
            plain = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn)
        finally:
            ctx.set_debug(0)
        assert_moments(res, want, (what, flag))
        assert not any(f in plain for f in SUMS)
        for k in SCALARS + ("hist", "shift"):
            assert np.array_equal(res[k], plain[k]), (what, flag, k)
        for f in SUMS:
            assert res[f].dtype == np.uint64 and not res[f][res["count"] == 0].any(), (what, flag, f)
        out = res
    return out


def test_an_exact_line(S, ctx):
    from shazam_amd.extent import line_fit, tempo_of
    rows = [(100 + i, 7, 1000 + 9 * i) for i in range(64)]
    rows += [(100 + i, 9, 1000 + 9 * i) for i in range(64)]                     # decoys: the same keys under song 9
    rows += [(100 + i, 7, 8 * i + 999 - i) for i in range(64)]                  # song 7 just below the range (d = 999 - i)
    rows += [(100 + i, 7, 8 * i + 1064 + i) for i in range(64)]                 # ... and just above it (d = 1064 + i)
    t = _table(S, ctx, rows)
    q = [(100 + i, 8 * i) for i in range(64)]
    r = _check(ctx, t, [q], [[(7, 1000, 1063)]], "line")
    assert int(r["count"][0, 0]) == 64
    line = line_fit(*(int(r[f][0, 0]) for f in ("count",) + SUMS), 1000)
    assert line == (Fraction(1, 8), Fraction(1000))
    assert tempo_of(65536, line[0]) == 1.125
    t.close()


def _segmented_table(S, ctx, rng):
    """4 batches, finalized one by one into segments of 1,000 rows: random rows under keys 0 .. 59, key 1000 with more than
    64 rows and key 2000 with more than 2,048, offsets 0 .. 5999"""
    t = S.Table(ctx)
    t.set_segment_rows(1000)
    for part in range(4):
        k = np.concatenate([rng.integers(0, 60, 500), np.full(18, 1000), np.full(540, 2000)]).astype(np.uint32)
        s = rng.integers(1, 7, len(k)).astype(np.uint32)
        o = rng.integers(0, 6000, len(k)).astype(np.uint32)
        t.insert(k, s, o)
        t.finalize()
    return t


def test_fuzz_against_the_twin(S, ctx):
    rng = np.random.default_rng(77)
    t = _segmented_table(S, ctx, rng)
    tk = t.export()[0]
    assert t.segments() >= 3 and (tk == 1000).sum() > 64 and (tk == 2000).sum() > 2048

    def hashes(n, big=0, mid=0):
        h = [(int(k), int(o)) for k, o in zip(rng.integers(0, 60, n), rng.integers(0, 41, n))]
        h += [(2000, int(o)) for o in rng.integers(0, 41, big)] + [(1000, int(o)) for o in rng.integers(0, 41, mid)]
        return h + h[:n // 10]                                                  # duplicates: a query is a set

    queries = [hashes(270, 2, 1), [], hashes(150, 1, 2), hashes(40, 1, 0), hashes(200, 0, 3),
               hashes(7), hashes(120, 2, 1), hashes(1), hashes(250, 1, 1)]       # 9 queries: more than the 4 of a chunk's LDS
    assert len(queries) == 9 and max(len(q) for q in queries) <= 300

    def some(n):
        out = []
        for _ in range(n):
            lo = int(rng.integers(-40, 5000))
            out.append((int(rng.integers(1, 7)), lo, lo + int(rng.integers(0, 600))))
        return out

    cands = [some(5), some(2), some(64),                                        # (query 2: all 64 candidates)
             [(3, -30, 4065), (3, 1000, 3000), (3, 2999, 2999), (4, -40, -40), (4, 17, 17)],   # one song twice; widths 4,096 and 1 bin
             some(7), some(3), [(1, -40, 4055), (2, 1905, 6000)], some(1), some(9)]
    assert max(hi - lo for c in cands for _, lo, hi in c) == 4095
    r = _check(ctx, t, queries, cands, "fuzz", ncand=64)
    assert int(r["count"][3, 0]) > int(r["count"][3, 1]) > 0                    # the overlap counts in both
    assert (r["count"] > 0).sum() > 40 and int(r["sum_qu"].max()) > 0
    t.close()


@pytest.mark.parametrize("place", [0, 4])
def test_64_bit_carries_through_the_lds_flush_and_the_global_path(S, ctx, place):
    """5,000 rows of one key and one song at offsets QMAX - 400 + j, the query's one hash at offset QMAX: d = j - 400, and the
    range [0, 4095] holds 4,096 of them.  sum_qq = 4096 QMAX^2 (about 2^52), sum_qu = QMAX * 4095 * 4096 / 2 (about 2^43).
    place 0: the query is the first of every chunk (LDS); place 4: behind four small queries, the fifth of the first chunk
    (global memory) and the first of the later tiles' chunks."""
    rows = [(5, 1, QMAX - 400 + j) for j in range(5000)] + [(10 + i, 2, 50) for i in range(4)]
    t = _table(S, ctx, rows)
    queries = [[(10 + i, 3)] for i in range(place)] + [[(5, QMAX)]]
    cands = [[(2, 47, 47)] for _ in range(place)] + [[(1, 0, 4095)]]
    r = _check(ctx, t, queries, cands, ("carries", place))
    got = {f: int(r[f][place, 0]) for f in ("count",) + SUMS}
    su = 4095 * 4096 // 2
    assert got == {"count": 4096, "sum_q": 4096 * QMAX, "sum_u": su, "sum_qq": 4096 * QMAX * QMAX, "sum_qu": QMAX * su}
    assert got["sum_qu"] > 1 << 32 and got["sum_qq"] > 1 << 51
    assert r["count"][:place, 0].tolist() == [1] * place and r["sum_q"][:place, 0].tolist() == [3] * place
    t.close()


def _raw(ctx, t, qk, qo, qoff, n, ncand, cs, lo, hi, cn, null=None):
    """shz_match_extents_fit as it is, on outputs filled with a pattern: (status, outputs untouched?)"""
    from shazam_amd import _ffi
    L, ptr = _ffi.lib(), _ffi.ptr
    cells = n * ncand
    outs = {k: np.full(cells, 0xABABABAB, np.uint32) for k in SCALARS}
    outs["hist"] = np.full(cells * 64, 0xABABABAB, np.uint32)
    outs["shift"] = np.full(n, 0xABABABAB, np.uint32)
    outs.update({f: np.full(cells, 0xABABABAB, np.uint64) for f in SUMS})
    a = dict(outs)
    if null:
        a[null] = None
    rc = L.shz_match_extents_fit(ctx.h, t.h, ptr(qk), ptr(qo), qoff.ctypes.data_as(_ffi.u64p), n, ncand, ptr(cs), ptr(lo), ptr(hi),
                                 ptr(cn), ptr(a["count"]), ptr(a["q_first"]), ptr(a["q_last"]), ptr(a["t_first"]), ptr(a["t_last"]),
                                 ptr(a["hist"]), ptr(a["shift"]), *[ptr(a[f]) for f in SUMS])
    return rc, all((v == 0xABABABAB).all() for v in outs.values())


def test_refusals_leave_the_outputs_untouched(S, ctx):
    from shazam_amd import _ffi
    t = _table(S, ctx, [(1, 1, 10), (2, 1, 5000)])
    qk, qo, qoff = _query_arrays([[(1, 5)], [(2, 15)]])
    cs, lo, hi, cn = _cand_arrays([[(1, 5, 5)], [(1, 900, 4995)]], ncand=2)      # (the second: 4,096 bins, the widest allowed)
    rc, same = _raw(ctx, t, qk, qo, qoff, 2, 2, cs, lo, hi, cn)
    assert rc == _ffi.OK and not same
    for f in SUMS:
        assert _raw(ctx, t, qk, qo, qoff, 2, 2, cs, lo, hi, cn, null=f) == (_ffi.E_INVALID, True), f
    wide = hi.copy()
    wide[1, 0] += 1                                                             # d_hi - d_lo = 4096
    assert _raw(ctx, t, qk, qo, qoff, 2, 2, cs, lo, wide, cn) == (_ffi.E_UNSUPPORTED, True)
    with pytest.raises(_ffi.ShzError):
        t.match_extents(qk, qo, qoff, cs, lo, wide, cand_n=cn, fit=True)
    r = t.match_extents(qk, qo, qoff, cs, lo, wide, cand_n=cn)                  # without the sums the width is free
    assert int(r["count"][1, 0]) == 1
    t.close()
