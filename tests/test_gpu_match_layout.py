"""GPU: the match at the limits of its packed vote key, against the exact int64 reference of test_match_layout_ref.py.

shz_match_batch packs every vote into one integer, (query, song id, delta + bias, first-row flag), with field widths
chosen per call: sb = bits(max song id), dbits = bits(max offset + bias), bias = the largest query offset, qb =
bits(queries - 1).  The widths pick the vote path (the queued single query, the one-workgroup fold, the vote tiles up to
20 delta bits with delta-split sweeps above 12, 4-byte passes while qb + sb + dbits + 1 <= 31, the 8-byte sort and
record chain) and, past 64 bits, a split of the sub-batch.  Every case below puts the table's largest song id / offset
or the queries' largest offset exactly on one side of one of those edges, plants a true match plus count and delta ties,
and runs through every path that can take it: the default, full_sort, one host query at a time, ShardedTable with 1 and
3 shards, on one segment and on several; and once more in child processes under SHZ_VOTE32=1 / SHZ_VOTE_TILES=0.

The contract, in both directions: a call returns all seven arrays equal to the reference, or raises
ShzError(SHZ_E_UNSUPPORTED) exactly where shz.h says it must -- a query offset >= 2^20, a table offset >= 2^31, or a
query with hashes whose key alone does not fit: 1 + sb + bits(max offset + its largest offset) + 1 > 64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_match_layout_ref import FIELDS, expected_match, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPNS = (1, 8, 9)            # VT_MAXTOPN = 8: 9 leaves the tile paths


def _bits(v):
    return max(1, int(v).bit_length())


def _spec(name, max_sid, max_off, max_qoff, nq=3, n_rows=400, n_keys=48, qlen=40, tie_sid=None):
    return dict(name=name, kind="planted", max_sid=max_sid, max_off=max_off, max_qoff=max_qoff, nq=nq, n_rows=n_rows,
                n_keys=n_keys, qlen=qlen, tie_sid=tie_sid)


def _cases():
    c = []
    # song-id bits (the rank key is 0xFFFFFFFF - sid: ties on either side of 2^31)
    for s in (1, 2 ** 11 - 1, 2 ** 11, 2 ** 20, 2 ** 24 - 1, 2 ** 31, 2 ** 32 - 1):
        c.append(_spec(f"sid_{s}", s, 3000, 100, tie_sid=2 ** 31 - 1 if s >= 2 ** 31 else None))
    # delta bits: max offset + bias at 2^k - 1 and 2^k (tiles up to 20 bits, sweeps above 12, 32 bits past int32)
    for k in (12, 13, 20, 21, 31):
        for e in (-1, 0):
            c.append(_spec(f"dbits_{k}{e:+d}", 2 ** 20, 2 ** k + e - 50, 50))
    c.append(_spec("delta_most_negative", 2 ** 20, 3000, 2 ** 20 - 1))      # offset 0 against query offset 2^20 - 1
    c.append(_spec("off_2^31-1_qoff_max", 7, 2 ** 31 - 1, 2 ** 20 - 1))      # 32 delta bits, the largest supported
    # offsets >= 2^31: refused (a delta would not fit out_delta's int32)
    c.append(_spec("off_2^31", 2 ** 20, 2 ** 31, 50))
    c.append(_spec("off_2^32-1", 9, 2 ** 32 - 1, 0))
    c.append(_spec("off_3e9_sid_2^24", 2 ** 24 - 1, 3_000_000_000, 1000))
    # query offsets: 2^20 - 1 is the largest accepted
    c.append(_spec("qoff_2^20", 300, 3000, 2 ** 20))
    # 4-byte boundary: sb + dbits in {30, 31, 32} with enough votes (> 8,192) for the 4-byte passes and the tiles
    for sd in (30, 31, 32):
        c.append(_spec(f"vote32_sb+db={sd}", 2 ** 20, 2 ** (sd - 21) - 1 - 20, 20, n_rows=20000, n_keys=40))
        c.append(_spec(f"vote32w_sb+db={sd}", 2 ** 12, 2 ** (sd - 13) - 1 - 20, 20, n_rows=20000, n_keys=40))
    # 64-bit boundary: qb + sb + dbits + 1 = 64 / 65 (sb = 32; qb = 1 for 1 or 2 queries, 3 for 5)
    for nq in (1, 2, 5):
        qb = _bits(nq - 1)
        for tot in (64, 65):
            db = tot - 1 - 32 - qb                                              # bits(max offset + 100)
            c.append(_spec(f"key64_nq{nq}_{tot}", 2 ** 32 - 1, 2 ** db - 101 if tot == 64 else 2 ** (db - 1) - 100, 100, nq=nq))
    c.append(_spec("key65_sb31_db32", 2 ** 30, 2 ** 31 - 50, 100, nq=1))     # 1 + 31 + 32 + 1
    c.append(_spec("key64_sb30_db32", 2 ** 29, 2 ** 31 - 50, 100, nq=2))     # 1 + 30 + 32 + 1
    # many one-hash queries: MAX_Q_SUB = 4,096 per sub-batch, QIDX_SHIFT + qb = 64 in the small head; and a layout that
    # fits 4,096 queries only in halves (12 + 32 + 20 + 1 = 65)
    for nq in (4095, 4096, 4097):
        c.append(dict(name=f"onehash_{nq}", kind="onehash", nq=nq, max_sid=2 ** 24 - 1, max_off=3000, max_qoff=100))
    c.append(dict(name="onehash_4097_key65", kind="onehash", nq=4097, max_sid=2 ** 32 - 1, max_off=600000, max_qoff=100))
    # vote counts: just above / at the one-workgroup limit (32,768), one (song, delta) group of 400 votes
    # (m_reduce_long_kernel), and > 2^22 votes in one pass (the unforced default takes 4-byte votes)
    for nv in (32768, 32769):
        c.append(dict(name=f"votes_{nv}", kind="hot", votes=nv, reps=1, max_sid=2 ** 20, max_off=4000))
    c.append(dict(name="long_group", kind="long", max_sid=2 ** 24 - 1, max_off=2 ** 20))
    c.append(dict(name="votes_4.5M", kind="hot", votes=3000, reps=1500, max_sid=1000, max_off=4000))
    return c


CASES = _cases()


def build_case(spec):
    """(tk, ts, to, qk, qo, qoff) as int64 arrays"""
    seed = 7 + sum(map(ord, spec["name"]))
    rng = np.random.default_rng(seed)
    kind = spec["kind"]
    if kind == "planted":
        return make_case(seed, spec["max_sid"], spec["max_off"], spec["max_qoff"], n_rows=spec["n_rows"], nq=spec["nq"],
                         n_keys=spec["n_keys"], qlen=spec["qlen"], tie_sid=spec["tie_sid"])
    if kind == "onehash":
        tk, ts, to, _, _, _ = make_case(seed, spec["max_sid"], spec["max_off"], spec["max_qoff"], n_rows=3000, nq=1,
                                        n_keys=400)
        nq = spec["nq"]
        qk = tk[rng.integers(0, len(tk), nq)]
        qo = rng.integers(0, spec["max_qoff"] + 1, nq)
        qo[0] = spec["max_qoff"]
        return tk, ts, to, qk, qo, np.arange(nq + 1, dtype=np.int64)
    if kind == "hot":
        # one hot key with `votes` rows (songs 1..max_sid, offsets 0..max_off: count ties everywhere), queried at `reps`
        # offsets; plus a cold table and a second query
        n = spec["votes"]
        K = np.int64(0x12345678)
        tk = np.full(n, K)
        cell = rng.choice(39 * 4001, n, replace=False)                          # distinct (song, offset) rows
        ts, to = 1 + cell // 4001, cell % 4001
        ts[0], to[0] = spec["max_sid"], spec["max_off"]
        ck = rng.integers(0, 1 << 32, 500)
        tk, ts, to = (np.concatenate([tk, ck]), np.concatenate([ts, rng.integers(1, 40, 500)]),
                      np.concatenate([to, rng.integers(0, spec["max_off"] + 1, 500)]))
        rows = np.unique(np.stack([tk, ts, to], 1), axis=0)
        tk, ts, to = rows[:, 0], rows[:, 1], rows[:, 2]
        reps = spec["reps"]
        qk = np.concatenate([np.full(reps, K), ck[:30]])
        qo = np.concatenate([np.arange(reps) * 3 % 2000, rng.integers(0, 2000, 30)])
        return tk, ts, to, qk, qo, np.array([0, reps, reps + 30], np.int64)
    if kind == "long":
        # song max_sid: 400 rows aligned at one delta; 3 queries (8-byte sort and record chain when not forced)
        tk, ts, to, _, _, _ = make_case(seed, spec["max_sid"], spec["max_off"], 500, n_rows=3000, nq=1, n_keys=2000)
        lk = rng.integers(0, 1 << 32, 400)
        lo = rng.integers(10000, spec["max_off"] + 1, 400)
        tk, ts, to = np.concatenate([tk, lk]), np.concatenate([ts, np.full(400, spec["max_sid"])]), np.concatenate([to, lo])
        qk = np.concatenate([lk, tk[:50], lk[:200]])
        qo = np.concatenate([lo - 9000, rng.integers(0, 500, 50), lo[:200] - 9500])
        return tk, ts, to, qk, qo, np.array([0, 400, 450, 650], np.int64)
    raise ValueError(kind)


def refused(tk, ts, to, qk, qo, qoff):
    """the documented refusal rule of shz_match_batch (include/shz.h)"""
    if len(qoff) < 2:
        return False
    if int(to.max()) >= 2 ** 31 or (len(qo) and int(qo.max()) >= 2 ** 20):
        return True
    sb = _bits(ts.max())
    for q in range(len(qoff) - 1):
        a, b = int(qoff[q]), int(qoff[q + 1])
        if a < b and 1 + sb + _bits(int(to.max()) + int(qo[a:b].max())) + 1 > 64:
            return True
    return False


def _compare(res, want):
    """mismatching field names (result entries past nres are not part of the contract)"""
    bad = [f for f in ("nres", "nhash", "npairs") if not np.array_equal(np.asarray(res[f], np.int64), want[f])]
    if bad:
        return bad
    for q in range(len(want["nres"])):
        n = int(want["nres"][q])
        for f in FIELDS[:4]:
            if not np.array_equal(np.asarray(res[f][q, :n], np.int64), want[f][q, :n]):
                bad.append(f"{f}[{q}]")
    return bad


def _tables(ctx, form, tk, ts, to):
    """(path name, table) pairs of one table form: "one" -- one segment; "seg" -- several segments"""
    import shazam_amd as S
    from shazam_amd.shard import ShardedTable
    u = [np.ascontiguousarray(x, np.uint32) for x in (tk, ts, to)]
    out = []
    kinds = (("table", S.Table(ctx)), ("shard1", ShardedTable(ctx, nshards=1)), ("shard3", ShardedTable(ctx, nshards=3)))
    for name, t in kinds:
        if form == "seg":
            if name == "shard1":
                t.close()
                continue
            t.set_segment_rows(max(16, len(u[0]) // 4))
            for part in np.array_split(np.arange(len(u[0])), 4):
                t.insert(u[0][part], u[1][part], u[2][part])
                t.finalize()
            if name == "table":
                assert t.segments() >= 3
        else:
            t.insert(*u)
            t.finalize()
        out.append((name, t))
    return out


def run_case(ctx, spec, forms=("one", "seg")):
    """every path x topn on the case: list of failure strings"""
    import shazam_amd as S
    tk, ts, to, qk, qo, qoff = build_case(spec)
    rows = np.unique(np.stack([tk, ts, to], 1), axis=0)       # each row once (unique across segments)
    tk, ts, to = rows[:, 0], rows[:, 1], rows[:, 2]
    assert int(ts.max()) == spec["max_sid"] and int(to.max()) == spec["max_off"], spec["name"]
    nq = len(qoff) - 1
    qk32, qo32, qoff64 = (np.ascontiguousarray(qk, np.uint32), np.ascontiguousarray(qo, np.uint32),
                          np.ascontiguousarray(qoff, np.uint64))
    want_refused = refused(tk, ts, to, qk, qo, qoff)
    one_refused = [refused(tk, ts, to, qk[qoff[q]:qoff[q + 1]], qo[qoff[q]:qoff[q + 1]], np.array([0, qoff[q + 1] - qoff[q]]))
                   for q in range(nq)] if nq <= 64 else None
    fails = []

    def call(label, fn, refuse, want):
        try:
            res = fn()
        except S.ShzError as e:
            if not (refuse and e.code == -5):                               # SHZ_E_UNSUPPORTED
                fails.append(f"{spec['name']} {label}: ShzError {e.code} {e} (refusal expected: {refuse})")
            return
        bad = _compare(res, want)
        if refuse:
            fails.append(f"{spec['name']} {label}: returned ({'wrong ' + str(bad[:4]) if bad else 'exact'}), "
                         "SHZ_E_UNSUPPORTED expected")
            return
        if bad:
            f0 = bad[0].split("[")[0]
            q = int(np.nonzero([not np.array_equal(np.asarray(res[f0][i]).ravel()[:1], np.asarray(want[f0][i]).ravel()[:1])
                                for i in range(len(want["nres"]))] + [True])[0][0]) % len(want["nres"])
            fails.append(f"{spec['name']} {label}: {bad[:6]} query {q}: {f0} {np.asarray(res[f0][q]).ravel()[:4].tolist()}, "
                         f"expected {np.asarray(want[f0][q]).ravel()[:4].tolist()}")

    w9 = expected_match(tk, ts, to, qk, qo, qoff, max(TOPNS))
    wants = {topn: dict(w9, nres=np.minimum(w9["nres"], topn), **{f: w9[f][:, :topn] for f in FIELDS[:4]}) for topn in TOPNS}
    for form in forms:
        for name, t in _tables(ctx, form, tk, ts, to):
            for topn in TOPNS:
                want = wants[topn]
                lab = f"{form}/{name}/top{topn}"
                call(lab, lambda: t.match(qk32, qo32, qoff64, topn), want_refused, want)
                if name == "table":
                    call(lab + "/full_sort", lambda: t.match(qk32, qo32, qoff64, topn, full_sort=True), want_refused, want)
                    if one_refused is not None and nq > 1:           # one host query at a time (spec where it fits)
                        for q in range(nq):
                            a, b = int(qoff[q]), int(qoff[q + 1])
                            wq = {f: want[f][q:q + 1] for f in FIELDS}
                            call(f"{lab}/single{q}", lambda: t.match(qk32[a:b], qo32[a:b], np.array([0, b - a], np.uint64),
                                                                      topn), one_refused[q], wq)
            t.close()
    return fails


def child_main(names):
    """run the named cases in this process (the switches are read once per process); print the failures as JSON"""
    import shazam_amd as S
    ctx = S.get_context(0)
    fails = []
    for spec in CASES:
        if spec["name"] in names:
            fails += run_case(ctx, spec, forms=("one",))
    print("FAILS " + json.dumps(fails))


@pytest.mark.parametrize("spec", CASES, ids=[c["name"] for c in CASES])
def test_match_layout_contract(spec):
    import shazam_amd as S
    fails = run_case(S.get_context(0), spec)
    assert not fails, "\n".join(fails[:20])


# the cases a forced or disabled switch changes the path of (4-byte votes, tiles, the one-workgroup fold) -- and the
# field edges in them
CHILD_CASES = [c["name"] for c in CASES if c["kind"] != "onehash"]
CHILD = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_match_layout as L; L.child_main(sys.argv[1:])"
         % (ROOT, os.path.join(ROOT, "tests")))


@pytest.mark.parametrize("env", [{"SHZ_VOTE32": "1"}, {"SHZ_VOTE_TILES": "0"}], ids=["vote32", "no_tiles"])
def test_match_layout_contract_under_switches(env):
    e = dict(os.environ)
    for k in ("SHZ_VOTE32", "SHZ_VOTE_TILES"):
        e.pop(k, None)
    e.update(env)
    out = subprocess.run([sys.executable, "-c", CHILD] + CHILD_CASES, env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("FAILS ")][-1]
    fails = json.loads(line[6:])
    assert not fails, "\n".join(fails[:20])
