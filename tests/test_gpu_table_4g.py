"""GPU: the table build at its REAL run limit, n = 2^32 - 4096 rows (SHZ_RUN_ROWS_MAX, the most rows one sorted run or
one segment cut from runs may hold).  Rows come from a formula, so the answer is known without a CPU table:
row i < n is (key = i * A mod 2^32, sid = 1 + (i >> 12), off = i & 0xFFF) with A odd -- distinct keys, 4096 rows a song,
12 + 20 bits of sid + offset inside the packed run layout.  The row of a key is i = key * A^-1 mod 2^32, present iff i < n.

* A: all n rows staged, ~10,000 of them again (more staged rows than the limit, exactly n distinct ones): one seal_run
  cuts a run of exactly n rows and one of the re-inserted rows, finalize merges them (INSERT IGNORE across the runs);
* B: the same with set_segment_rows(2^32 - 1): the merge cuts one segment of n rows, so probes run at row positions
  >= 2^31; a match of rows that sit there gives what oracle/cpu_ref.py's vote gives over the rows lookup() returned.

The build needs ~220 GB of device memory (reserved up front: 12 B/row staging, 12 B/row segment slab, 8.6 B/row run
arena, 8.5 B/row sort scratch); the test skips where less is free."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (1 << 32) - 4096
A = 0x9E3779B1
A_INV = pow(A, -1, 1 << 32)
CHUNK = 1 << 27
N_AGAIN = 10000
# free device memory a case needs: its peak measured on MI355X (hipMemGetInfo sampled every 20 ms while the build runs)
# was 219 GB above what was free before it; + 7 %.  Each case took ~16 s there (staging ~15 s, seal + finalize < 1 s).
NEED_BYTES = 235 * 10**9


def _rows_of(i):
    i = np.asarray(i, np.uint32)
    return i * np.uint32(A), (i >> np.uint32(12)) + np.uint32(1), i & np.uint32(0xFFF)


def _index_of(keys):
    return np.asarray(keys, np.uint32) * np.uint32(A_INV)


class _Peak:
    """Lowest free device memory seen while the build runs (hipMemGetInfo, sampled every 20 ms)."""

    def __init__(self, ctx):
        self.ctx, self.low, self.stop = ctx, ctx.mem_info()[0], threading.Event()
        self.th = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self.stop.wait(0.02):
            self.low = min(self.low, self.ctx.mem_info()[0])

    def __enter__(self):
        self.th.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.th.join()
        self.low = min(self.low, self.ctx.mem_info()[0])


def _expect(keys):
    """Rows lookup() must return for `keys` (distinct), in key-list order."""
    i = _index_of(keys)
    hit = i < np.uint32(N)
    k, s, o = _rows_of(i[hit])
    assert np.array_equal(k, np.asarray(keys, np.uint32)[hit])
    return k, s, o


def _distinct_in_order(keys):
    keys = np.asarray(keys, np.uint32)
    _, first = np.unique(keys, return_index=True)
    return keys[np.sort(first)]


@pytest.mark.parametrize("case", ["A", "B"])
def test_build_at_the_real_run_limit(case):
    from oracle import cpu_ref as O
    from shazam_amd import _ffi as F
    ctx = F.Context(0)
    try:
        free0, total = ctx.mem_info()
        if free0 < NEED_BYTES:
            pytest.skip(f"needs {NEED_BYTES / 1e9:.0f} GB of free device memory, {free0 / 1e9:.0f} GB are free")
        rng = np.random.default_rng(4 + (case == "B"))
        again = np.unique(np.r_[0, N // 2, N - 1, rng.integers(0, N, N_AGAIN, dtype=np.uint64)]).astype(np.uint32)
        t0 = time.time()
        tbl = F.Table(ctx)
        try:
            with _Peak(ctx) as peak:
                if case == "B":
                    tbl.set_segment_rows((1 << 32) - 1)
                tbl.reserve(N, N, gather=True, wait=True)
                for lo in range(0, N, CHUNK):
                    tbl.insert(*_rows_of(np.arange(lo, min(N, lo + CHUNK), dtype=np.uint32)))
                tbl.insert(*_rows_of(again))
                t_stage = time.time() - t0
                assert tbl.rows() == (0, N + len(again))
                tbl.seal_run()
                assert tbl.exchange_stats()["runs_held"] == 2   # a run of exactly N rows + the re-inserted rows
                tbl.finalize()
            t_build = time.time() - t0
            assert tbl.rows() == (N, 0)
            if case == "B":
                assert tbl.segments() == 1
            else:
                assert tbl.segments() >= 2   # (segments of at most 2^31 rows)

            # lookups: random keys (absent ones among them), 0, 0xFFFFFFFF, the re-inserted rows' keys, the 4096 absent keys
            absent = (np.arange(N, 1 << 32, dtype=np.uint64).astype(np.uint32)) * np.uint32(A)
            keys = _distinct_in_order(np.concatenate([
                np.array([0, 0xFFFFFFFF], np.uint32), rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                _rows_of(again)[0], absent]))
            got = tbl.lookup(keys)
            exp = _expect(keys)
            for g, e in zip(got, exp):
                assert np.array_equal(g, e)
            assert len(tbl.lookup(absent)[0]) == 0
            last_sid = int(_rows_of(N - 1)[1])
            for sid in (1, last_sid, int(rng.integers(2, last_sid))):
                assert tbl.song_rows(sid) == 4096, sid

            if case == "B":
                # a query from the rows of one song that sit at row positions >= 2^31 of the one segment (the position of a
                # key is the count of present keys below it: keys >= 2^31 + 4096 are past 2^31), + rows of another song at
                # scattered offsets, + absent keys
                sid = int(rng.integers(2, last_sid))
                k, s, o = _rows_of(np.arange((sid - 1) << 12, sid << 12, dtype=np.uint32))
                far = k >= np.uint32((1 << 31) + 4096)
                assert far.sum() > 1000
                k2, _, o2 = _rows_of(np.arange(0, 4096, 7, dtype=np.uint32))
                qk = np.concatenate([k[far], k2, absent[:100]])
                qo = np.concatenate([o[far] + np.uint32(5), (o2 * np.uint32(3)) % np.uint32(4000), np.arange(100, dtype=np.uint32)])
                qoff = np.array([0, len(qk)], np.uint64)
                res = tbl.match(qk, qo, qoff, 3)
                lk, ls, lo_ = tbl.lookup(_distinct_in_order(qk))
                db = O.DictDB()
                for kk, ss, oo in zip(lk.tolist(), ls.tolist(), lo_.tolist()):
                    db.rows.setdefault(kk, []).append((ss, oo))
                matches, dedup = O.return_matches(zip(qk.tolist(), qo.tolist()), db)
                want = O.vote(matches, 3)
                assert want[0][:2] == (sid, -5) and want[0][2] == int(far.sum())
                nres = int(res["nres"][0])
                assert nres == len(want)
                assert [(int(res["sid"][0, j]), int(res["delta"][0, j]), int(res["aligned"][0, j])) for j in range(nres)] == \
                    [tuple(w) for w in want]
                assert [int(res["dedup"][0, j]) for j in range(nres)] == [dedup[w[0]] for w in want]
                assert int(res["nhash"][0]) == len(set(zip(qk.tolist(), qo.tolist())))
            t_all = time.time() - t0
        finally:
            tbl.close()
        print(f"\n[table_4g] case {case}: peak {(free0 - peak.low) / 1e9:.1f} GB of {total / 1e9:.1f} GB "
              f"({free0 / 1e9:.1f} GB free before); staging {t_stage:.1f} s, build {t_build:.1f} s, all {t_all:.1f} s")
    finally:
        ctx.close()
