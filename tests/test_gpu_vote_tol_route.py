"""GPU: the tolerant vote route at tolerance 0 (SHZ_DEBUG_VOTE_TOLERANT_ROUTE: 8-byte votes, the full sort, the fold over
runs of equal (query, song, delta)) returns, array for array, what the plain routes return on the same inputs -- the table and
query shapes of tests/test_gpu_match_fuzz.py, with several queries, an empty query and a query without votes in every batch,
at topn 1, 2 and 5 -- and what that file's numpy reference expects; one small host-fed query, which is otherwise queued ahead
of its vote count, is not queued on the tolerant route and gives the same arrays."""
import numpy as np
import pytest

from test_gpu_match_fuzz import _expected

pytestmark = pytest.mark.gpu

ARRAYS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")
TOLERANT = 128   # SHZ_DEBUG_VOTE_TOLERANT_ROUTE


def _forced(ctx, fn):
    ctx.set_debug(TOLERANT)
    try:
        return fn()
    finally:
        ctx.set_debug(0)


def _same(a, b, what):
    for name in ARRAYS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (what, name)


@pytest.mark.parametrize("seed", range(8))
def test_forced_route_equals_plain_routes(seed):
    import shazam_amd as S
    ctx = S.get_context(0)
    rng = np.random.default_rng(4000 + seed)
    n_rows = int([50, 3000, 40000, 250000][seed % 4])
    sizes = [int(rng.choice([1, 9, 150, 2500])) for _ in range(int(rng.choice([3, 7, 40])))]
    # hot keys, but at most ~4M votes in all: every vote goes through the 8-byte sort here
    n_keys = max(int(rng.choice([3, 40, 2000, 60000])), n_rows * sum(sizes) // 4_000_000 + 1)
    n_sid = int(rng.choice([2, 17, 300, 5000]))
    max_off = int(rng.choice([5, 200, 3000]))
    keyspace = ((rng.integers(0, 2049, n_keys) << 20) | (rng.integers(0, 2049, n_keys) << 8) | rng.integers(0, 201, n_keys)).astype(np.uint32)
    tk = keyspace[rng.integers(0, n_keys, n_rows)]
    ts = rng.integers(1, n_sid + 1, n_rows).astype(np.uint32)
    to = rng.integers(0, max_off + 1, n_rows).astype(np.uint32)
    t = S.Table(ctx)
    parts = 1 + seed % 3
    if seed % 3 == 1:   # several segments, song ids of their own per insert (as in the fuzz test)
        t.set_segment_rows(max(16, n_rows // 5))
        for pi, part in enumerate(np.array_split(np.arange(n_rows), parts)):
            ts[part] += np.uint32(pi * (n_sid + 1))
    for part in np.array_split(np.arange(n_rows), parts):
        t.insert(tk[part], ts[part], to[part])
        t.finalize()
    sizes[1:1] = [0, -2]                                     # an empty query; a query of hashes the table does not hold
    qk, qo, qoff = [], [], [0]
    for m in sizes:
        if m < 0:
            k = np.uint32(0xFFF00000) | rng.integers(0, 1 << 20, 30).astype(np.uint32)
        else:
            k = keyspace[rng.integers(0, n_keys, m)] if m else np.zeros(0, np.uint32)
        qk.append(k)
        qo.append(rng.integers(0, int(rng.choice([1, 4, 120])), len(k)).astype(np.uint32))
        qoff.append(qoff[-1] + len(k))
    qk, qo, qoff = np.concatenate(qk).astype(np.uint32), np.concatenate(qo).astype(np.uint32), np.array(qoff, np.uint64)
    for topn in (1, 2, 5):
        plain = t.match(qk, qo, qoff, topn)
        forced = _forced(ctx, lambda: t.match(qk, qo, qoff, topn))
        _same(plain, forced, (seed, topn))
        assert int(forced["nres"][1]) == 0 and int(forced["nhash"][1]) == 0
        assert int(forced["nres"][2]) == 0 and int(forced["npairs"][2]) == 0 and int(forced["nhash"][2]) > 0
        for q, (ranked, npairs, nhash) in enumerate(_expected(tk, ts, to, qk, qo, qoff, topn)):
            assert int(forced["npairs"][q]) == npairs and int(forced["nhash"][q]) == nhash, (seed, q)
            got = [(int(forced["sid"][q, i]), int(forced["delta"][q, i]), int(forced["aligned"][q, i]), int(forced["dedup"][q, i]))
                   for i in range(int(forced["nres"][q]))]
            assert got == ranked, (seed, topn, q)
    # the full sort of the same queries is the third witness; the forced route keeps its place beside the flag
    _same(t.match(qk, qo, qoff, 5, full_sort=True), _forced(ctx, lambda: t.match(qk, qo, qoff, 5, full_sort=True)), (seed, "full sort"))
    t.close()


def test_single_small_query_is_not_queued_on_the_forced_route():
    import shazam_amd as S
    ctx = S.get_context(0)
    rng = np.random.default_rng(77)
    n_songs, n_rows = 60, 20000
    key = ((rng.integers(0, 2049, n_rows) << 20) | (rng.integers(0, 2049, n_rows) << 8) | rng.integers(0, 201, n_rows)).astype(np.uint32)
    sid = rng.integers(1, n_songs + 1, n_rows).astype(np.uint32)
    off = rng.integers(0, 400, n_rows).astype(np.uint32)
    t = S.Table(ctx)
    t.insert(key, sid, off)
    t.finalize()
    pick = rng.integers(0, n_rows, 700)
    qk, qo = key[pick], (off[pick] % 7 + 3).astype(np.uint32)
    qoff = np.array([0, len(qk)], np.uint64)
    t.match(qk, qo, qoff, 3)                                   # (the table's votes per hash are known from here on)
    q0, u0 = ctx.spec_stats()
    plain = t.match(qk, qo, qoff, 3)
    q1, u1 = ctx.spec_stats()
    assert (q1 - q0, u1 - u0) == (1, 1)                        # queued, and its results taken
    forced = _forced(ctx, lambda: t.match(qk, qo, qoff, 3))
    assert ctx.spec_stats() == (q1, u1)
    _same(plain, forced, "single query")
    dev = _forced(ctx, lambda: t.match_device(qk, qo, qoff, 3, bias_bound=int(qo.max())))
    assert ctx.spec_stats() == (q1, u1)
    _same(plain, dev, "single query, device columns")
    assert int(plain["nres"][0]) == 3
    t.close()
