"""GPU: the tolerant vote (Table.match(delta_tol=...)) on tables and queries built by hand, so that the votes per offset bin
are known, against its plain-Python definition (tests/vote_tol_twin.py): which window wins and which bin it reports, the
edges of the delta field and of a query, groups of one vote and of ~40,000, and a random fuzz in which the bins crowd.
Every comparison is exact."""
import numpy as np
import pytest

from vote_tol_twin import assert_match, expected_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


class Built:
    """A table and queries from single votes: vote(q, sid, delta, n) adds n votes of query q for song sid at offset difference
    delta, each through a key of its own (one row, one query hash)."""

    def __init__(self, n_queries=1, q_base=40):
        self.rows, self.hashes, self.key, self.q_base = [], [[] for _ in range(n_queries)], 0, q_base

    def vote(self, q, sid, delta, n=1, q_off=None):
        for _ in range(n):
            self.key += 1
            qo = self.q_base if q_off is None else q_off
            assert qo + delta >= 0
            self.rows.append((self.key, sid, qo + delta))
            self.hashes[q].append((self.key, qo))

    def bins(self, q, sid, bins):
        for d, n in bins.items():
            self.vote(q, sid, d, n)

    def arrays(self):
        tk, ts, to = (np.asarray([r[i] for r in self.rows], np.uint32) for i in range(3))
        qk = np.asarray([h[0] for hs in self.hashes for h in hs], np.uint32)
        qo = np.asarray([h[1] for hs in self.hashes for h in hs], np.uint32)
        qoff = np.cumsum([0] + [len(hs) for hs in self.hashes]).astype(np.uint64)
        return tk, ts, to, qk, qo, qoff

    def table(self, S, ctx):
        tk, ts, to, *_ = self.arrays()
        t = S.Table(ctx)
        t.insert(tk, ts, to)
        t.finalize()
        return t


def _check(S, ctx, b, tols, topns, what):
    tk, ts, to, qk, qo, qoff = b.arrays()
    t = b.table(S, ctx)
    out = {}
    for tol in tols:
        for topn in topns:
            res = t.match(qk, qo, qoff, topn, delta_tol=tol)
            assert_match(res, expected_match(tk, ts, to, qk, qo, qoff, tol, topn), (what, tol, topn))
            out[tol, topn] = res
    assert ctx.vote_tolerance == 0
    t.close()
    return out


def _top(res, q=0, i=0):
    return int(res["sid"][q, i]), int(res["delta"][q, i]), int(res["aligned"][q, i])


def test_window_choice_and_reported_bin(S, ctx):
    b = Built()
    b.bins(0, 1, {10: 3, 11: 4, 13: 5})
    b.bins(0, 2, {5: 2, 6: 2, 20: 3, 21: 1})      # two windows of 4 at tolerance 1: the smaller start; its bins tie: the smaller delta
    b.bins(0, 3, {-7: 1, -6: 2, -4: 2})           # (negative offsets differences too)
    b.bins(0, 6, {0: 2, 1: 1})                    # songs 6 and 5 reach 3 at tolerance 1: the smaller id first
    b.bins(0, 5, {30: 3})
    r = _check(S, ctx, b, (0, 1, 2, 3, 31), (1, 2, 5), "window")
    assert _top(r[1, 1]) == (1, 11, 7)
    assert _top(r[2, 1]) == (1, 13, 9)
    assert _top(r[3, 1]) == (1, 13, 12)
    assert _top(r[31, 1]) == (1, 13, 12)
    rows = {int(r[1, 5]["sid"][0, i]): (int(r[1, 5]["delta"][0, i]), int(r[1, 5]["aligned"][0, i])) for i in range(5)}
    assert rows[2] == (5, 4) and rows[3] == (-6, 3) and rows[5] == (30, 3) and rows[6] == (0, 3)
    assert r[1, 5]["sid"][0].tolist() == [1, 2, 3, 5, 6]


def test_field_edges(S, ctx):
    """The layout: bias = the largest query offset (27), delta bits = bits(largest table offset + bias) = bits(127) = 7.  Song 3
    has a vote at biased delta 127, the top of the field, and song 4 one at biased delta 0: neighbours in the sorted votes that
    no window may join, at any tolerance; the same across a query border (query 0's last vote, query 1's first)."""
    from shazam_amd.shard import vote_layout
    b = Built(n_queries=2)
    b.vote(0, 3, 100, 2, q_off=0)                 # delta 100, biased 127
    b.vote(0, 3, 98, 1, q_off=0)
    b.vote(0, 4, -27, 3, q_off=27)                # delta -27, biased 0
    b.vote(0, 4, -25, 1, q_off=27)
    b.vote(0, 1, -20, 2, q_off=25)                # negative deltas with neighbours on both sides
    b.vote(0, 1, -19, 2, q_off=25)
    b.vote(0, 1, -18, 1, q_off=20)
    b.vote(0, 7, 100, 1, q_off=0)                 # the largest song id of the table at the top of the field: query 0's last vote
    b.vote(1, 1, -27, 2, q_off=27)                # query 1's first vote: song 1 at biased delta 0
    b.vote(1, 1, -26, 1, q_off=27)
    b.vote(1, 7, 100, 1, q_off=0)
    tk, ts, to, qk, qo, qoff = b.arrays()
    assert vote_layout(7, int(to.max()), qo, 2) == (3, 7, 27) and int(to.max()) + 27 == 127
    r = _check(S, ctx, b, (0, 1, 31), (1, 5), "edges")
    got = {int(r[31, 5]["sid"][0, i]): (int(r[31, 5]["delta"][0, i]), int(r[31, 5]["aligned"][0, i])) for i in range(4)}
    assert got == {3: (100, 3), 4: (-27, 4), 1: (-20, 5), 7: (100, 1)}
    assert _top(r[31, 5], 1, 0) == (1, -27, 3) and _top(r[31, 5], 1, 1) == (7, 100, 1)
    # one query alone (no query bits in the vote), device columns with and without a bound
    t = b.table(S, ctx)
    a, e = int(qoff[0]), int(qoff[1])
    one = np.array([0, e - a], np.uint64)
    want = expected_match(tk, ts, to, qk[a:e], qo[a:e], one, 31, 5)
    assert_match(t.match(qk[a:e], qo[a:e], one, 5, delta_tol=31), want, "one query")
    with ctx.tolerance(31):
        assert_match(t.match_device(qk[a:e], qo[a:e], one, 5, bias_bound=27), want, "one query, device, bound")
        assert_match(t.match_device(qk[a:e], qo[a:e], one, 5), want, "one query, device")
    t.close()


def test_group_sizes(S, ctx):
    """Groups of one vote beside groups far larger than one workgroup folds.  Songs 2 and 3 (directly behind it): 40,000 votes
    each over three adjacent bins, the heaviest in the middle -- three runs of ~13,000 votes that cross dozens of workgroups.
    Songs 5 and 6: 200 rows of ONE key against 200 query offsets of that key, 40,000 votes each.  Rows and query hashes are
    sets, so the offset differences of one key spread over |rows| + |offsets| - 1 = 399 bins (1, 2, .., 200, .., 2, 1 votes): a
    group of 399 runs, folded by many waves of several workgroups into one record."""
    b = Built(q_base=300)
    b.vote(0, 1, 5)                                # a group of one vote in front
    b.bins(0, 2, {50: 13000, 51: 14000, 52: 13000})
    b.bins(0, 3, {-9: 12000, -8: 15000, -7: 13000})
    b.vote(0, 4, -2)                               # ... and one between the large ones
    rows, hashes = b.rows, b.hashes[0]
    for sid, key, base in ((5, 1 << 30, 1000), (6, (1 << 30) + 1, 400)):
        rows.extend((key, sid, base + i) for i in range(200))
        hashes.extend((key, 50 + j) for j in range(200))
    b.vote(0, 9, 0)                                # the last group: one vote
    r = _check(S, ctx, b, (0, 1, 2, 31), (1, 8), "groups")
    assert _top(r[0, 8]) == (3, -8, 15000)
    assert _top(r[1, 8]) == (3, -8, 28000) and _top(r[1, 8], 0, 1) == (2, 51, 27000)
    assert _top(r[2, 8]) == (2, 51, 40000) and _top(r[2, 8], 0, 1) == (3, -8, 40000)
    got = {int(r[31, 8]["sid"][0, i]): (int(r[31, 8]["delta"][0, i]), int(r[31, 8]["aligned"][0, i])) for i in range(7)}
    # 32 bins around the peak of 200: 185 .. 200 .. 184 -> the first of the two best windows starts 16 bins below the peak
    assert got[5] == (1000 - 50, sum(range(185, 201)) + sum(range(184, 200))) and got[6][1] == got[5][1]
    assert got[1] == (5, 1) and got[4] == (-2, 1) and got[9] == (0, 1)
    assert int(r[31, 8]["npairs"][0]) == 2 * 40000 + 2 * 40000 + 3


@pytest.mark.parametrize("nq", [1, 17])
@pytest.mark.parametrize("seed", range(3))
def test_random_fuzz_with_crowded_bins(S, ctx, seed, nq):
    """8 songs, 32 distinct keys, offsets below 64, queries of 500 hashes: every (query, song) group fills most of its 127 bins"""
    rng = np.random.default_rng(900 + 10 * seed + nq)
    keys = rng.choice(1 << 31, 32, replace=False).astype(np.uint32)
    n_rows = 700
    tk, ts, to = keys[rng.integers(0, 32, n_rows)], rng.integers(1, 9, n_rows).astype(np.uint32), rng.integers(0, 64, n_rows).astype(np.uint32)
    qk = keys[rng.integers(0, 32, 500 * nq)]
    qo = rng.integers(0, 64, 500 * nq).astype(np.uint32)
    qoff = (np.arange(nq + 1) * 500).astype(np.uint64)
    t = S.Table(ctx)
    t.insert(tk, ts, to)
    t.finalize()
    for tol in (1, 2, 5, 31):
        want5 = expected_match(tk, ts, to, qk, qo, qoff, tol, 5)
        for topn in (1, 2, 5):
            want = [(ranked[:topn], npairs, nhash) for ranked, npairs, nhash in want5]
            assert_match(t.match(qk, qo, qoff, topn, delta_tol=tol), want, (seed, nq, tol, topn))
    t.close()
