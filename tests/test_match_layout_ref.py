"""CPU: an exact numpy statement of return_matches + align_matches (recognizer.py:222-338) over the whole result of
Table.match, in plain int64 -- no packed vote key, so it holds at every song-id and offset width the schema allows
(song_id MEDIUMINT UNSIGNED, offset INT UNSIGNED: mysql_database.py:34-50, and wider).  It is checked here against
oracle/cpu_ref.py's return_matches / vote / align_matches over a DictDB, on small cases at the field limits: offsets
near 2^32 - 1, deltas of -(2^20 - 1), song ids near 2^24 and 2^32 - 1, count ties between songs and delta ties inside
a song.  tests/test_gpu_match_layout.py holds the HIP match to it.

make_case() builds those cases: random rows and queries around a planted true match per query, a second song with the
same votes (a count tie: the smaller id ranks first), a third song with two equally strong deltas (the smaller delta
wins) and votes at both delta extremes (the row at the largest offset with query offset 0, the row at offset 0 with
the largest query offset)."""
import numpy as np
import pytest

FIELDS = ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")


def _ranges(lo, cnt):
    """concatenation of arange(lo[i], lo[i] + cnt[i])"""
    cnt = np.asarray(cnt, np.int64)
    if cnt.sum() == 0:
        return np.zeros(0, np.int64)
    return np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))


def expected_match(tk, ts, to, qk, qo, qoff, topn):
    """Table.match's seven arrays, exactly: per query the set of (hash, offset) pairs (recognizer.py:378-382) is
    looked up in the rows UNIQUE(song_id, offset, hash) (INSERT IGNORE); every DB row of a queried hash counts once in
    dedup[sid] and votes once per query offset of that hash for (sid, db_off - q_off); per song the first largest
    count in ascending delta order; songs by count descending, then smaller song id; the first topn.
    Returns int64 arrays: sid / delta / aligned / dedup [nq, topn] (zero past nres), nres / nhash / npairs [nq]."""
    qoff = np.asarray(qoff, np.int64)
    nq = len(qoff) - 1
    out = {f: np.zeros((nq, topn), np.int64) for f in FIELDS[:4]}
    out.update({f: np.zeros(nq, np.int64) for f in FIELDS[4:]})
    rows = np.unique(np.stack([np.asarray(tk, np.int64), np.asarray(ts, np.int64), np.asarray(to, np.int64)], 1), axis=0)
    rk, rs, ro = rows[:, 0], rows[:, 1], rows[:, 2]                               # sorted by key
    qidx = np.repeat(np.arange(nq, dtype=np.int64), np.diff(qoff))
    hs = np.unique(np.stack([qidx, np.asarray(qk, np.int64), np.asarray(qo, np.int64)], 1), axis=0)
    if len(hs) == 0:
        return out
    out["nhash"] = np.bincount(hs[:, 0], minlength=nq).astype(np.int64)
    lo, hi = np.searchsorted(rk, hs[:, 1], "left"), np.searchsorted(rk, hs[:, 1], "right")
    idx = _ranges(lo, hi - lo)
    vq, vs = np.repeat(hs[:, 0], hi - lo), rs[idx]
    vd = ro[idx] - np.repeat(hs[:, 2], hi - lo)
    out["npairs"] = np.bincount(vq, minlength=nq).astype(np.int64)
    if len(vq) == 0:
        return out
    # dedup_hashes[sid]: the DB rows of every distinct queried hash, once per row
    qkeys = np.unique(hs[:, :2], axis=0)
    l2, h2 = np.searchsorted(rk, qkeys[:, 1], "left"), np.searchsorted(rk, qkeys[:, 1], "right")
    i2 = _ranges(l2, h2 - l2)
    dpair = (np.repeat(qkeys[:, 0], h2 - l2) << 33) | rs[i2]        # (query, sid) as one int64: sid < 2^33
    dk, dc = np.unique(dpair, return_counts=True)
    # counts per (query, sid, delta); per (query, sid) the largest count at the smallest delta
    g, c = np.unique(np.stack([vq, vs, vd], 1), axis=0, return_counts=True)
    order = np.lexsort((g[:, 2], -c, g[:, 1], g[:, 0]))
    g, c = g[order], c[order]
    first = np.ones(len(g), bool)
    first[1:] = (g[1:, 0] != g[:-1, 0]) | (g[1:, 1] != g[:-1, 1])
    b, bc = g[first], c[first]
    rank = np.lexsort((b[:, 1], -bc, b[:, 0]))
    b, bc = b[rank], bc[rank]
    pos = np.arange(len(b)) - np.searchsorted(b[:, 0], b[:, 0], "left")
    keep = pos < topn
    b, bc, pos = b[keep], bc[keep], pos[keep]
    q = b[:, 0]
    out["sid"][q, pos] = b[:, 1]
    out["delta"][q, pos] = b[:, 2]
    out["aligned"][q, pos] = bc
    out["dedup"][q, pos] = dc[np.searchsorted(dk, (q << 33) | b[:, 1])]
    out["nres"] = np.bincount(q, minlength=nq).astype(np.int64)
    return out


def make_case(seed, max_sid, max_off, max_qoff, n_rows=400, nq=3, n_keys=48, qlen=40, tie_sid=None):
    """(tk, ts, to, qk, qo, qoff): rows whose largest song id / offset are exactly max_sid / max_off (the row at
    max_off belongs to song max_sid) and queries whose largest offset is exactly max_qoff (every query holds it).
    Query q plants an aligned run on one song, the same run on a second song (tie_sid if given: a count tie, the
    smaller id must rank first), half of it at two deltas on a third song (a delta tie: the smaller delta must win)."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << 32, n_keys * 2, dtype=np.int64))[:n_keys]
    pool = {1, max_sid, max(1, max_sid - 1), max(1, max_sid // 2), max(1, max_sid >> 12)}
    pool.update(rng.integers(1, max_sid + 1, 6).tolist())
    if tie_sid is not None:
        pool.add(int(tie_sid))
    pool = np.array(sorted(pool), np.int64)
    tk = keys[rng.integers(0, len(keys), n_rows)]
    ts = pool[rng.integers(0, len(pool), n_rows)]
    to = rng.integers(0, max_off + 1, n_rows, dtype=np.int64)
    ts[0], to[0], to[1] = max_sid, max_off, 0
    rk, rsid, roff = [tk], [ts], [to]
    qk, qo, qoff = [], [], [0]
    for q in range(nq):
        d = int(rng.integers(-max_qoff, max_off + 1))                   # the planted delta
        qa, qb = max(0, -d), min(max_qoff, max_off - d)                 # query offsets whose row offset fits
        L = int(rng.integers(4, 13))
        pq = rng.integers(qa, qb + 1, L, dtype=np.int64)
        pk = keys[rng.integers(0, len(keys), L)]
        a = int(pool[rng.integers(0, len(pool))]) if q else max_sid
        b = int(tie_sid) if tie_sid is not None else int(pool[rng.integers(0, len(pool))])
        rk += [pk, pk]
        rsid += [np.full(L, a, np.int64), np.full(L, b, np.int64)]
        roff += [pq + d, pq + d]
        # third song: half the run at d and at a second delta d2
        c_ = int(pool[rng.integers(0, len(pool))])
        d2 = int(rng.integers(-max_qoff, max_off + 1))
        h = pq[(pq + d2 >= 0) & (pq + d2 <= max_off)][: L // 2]
        hk = pk[: len(h)]
        rk += [hk, hk]
        rsid += [np.full(len(h), c_, np.int64)] * 2
        roff += [h + d, h + d2]
        # the query: the planted pairs, the extremes, random pairs of table keys
        n_rand = int(rng.integers(0, qlen))
        k_ = np.concatenate([pk, [tk[0], tk[1]], keys[rng.integers(0, len(keys), n_rand)]])
        o_ = np.concatenate([pq, [0, max_qoff], rng.integers(0, max_qoff + 1, n_rand, dtype=np.int64)])
        qk.append(k_)
        qo.append(o_)
        qoff.append(qoff[-1] + len(k_))
    return (np.concatenate(rk), np.concatenate(rsid), np.concatenate(roff), np.concatenate(qk), np.concatenate(qo),
            np.array(qoff, np.int64))


def _oracle(tk, ts, to, qk, qo, qoff, topn):
    """the same arrays from cpu_ref's return_matches / vote / align_matches over a DictDB"""
    from oracle import cpu_ref as O
    db = O.DictDB()
    for k, s, o in zip(tk.tolist(), ts.tolist(), to.tolist()):
        db.insert_hashes(s, [(k, o)])
        db.songs.setdefault(s, {"song_name": f"s{s}", "file_sha1": "00", "total_hashes": 1, "fingerprinted": 1})
    nq = len(qoff) - 1
    out = {f: np.zeros((nq, topn), np.int64) for f in FIELDS[:4]}
    out.update({f: np.zeros(nq, np.int64) for f in FIELDS[4:]})
    for q in range(nq):
        hashes = set(zip(qk[qoff[q]:qoff[q + 1]].tolist(), qo[qoff[q]:qoff[q + 1]].tolist()))
        matches, dedup = O.return_matches(hashes, db)
        out["nhash"][q], out["npairs"][q] = len(hashes), len(matches)
        if not matches:
            continue
        ranked = O.vote(matches, topn)
        aligned = O.align_matches(matches, dedup, len(hashes), db, topn)
        assert [(r["song_id"], r["offset"]) for r in aligned] == [(s, d) for s, d, _ in ranked]
        out["nres"][q] = len(ranked)
        for i, ((s, d, c), r) in enumerate(zip(ranked, aligned)):
            out["sid"][q, i], out["delta"][q, i], out["aligned"][q, i] = s, d, c
            out["dedup"][q, i] = r["hashes_matched_in_input"]
    return out


# (max_sid, max_off, max_qoff): the limits the schema allows and the edges of the packed vote key
LIMIT_CASES = [
    (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 20 - 1), (2 ** 32 - 1, 2 ** 32 - 2, 0), (2 ** 24 - 1, 2 ** 32 - 1, 5),
    (2 ** 24, 2 ** 31, 2 ** 20 - 1), (2 ** 24 - 1, 0, 2 ** 20 - 1), (1, 0, 2 ** 20 - 1), (1, 2 ** 32 - 1, 2 ** 20 - 1),
    (2 ** 31, 2 ** 31 - 1, 1), (2 ** 31 - 1, 2 ** 31, 2 ** 20 - 2), (2 ** 11, 2 ** 12 - 1, 0), (5, 40, 30),
    (2 ** 32 - 2, 2 ** 20 - 1, 2 ** 20 - 1),
]


@pytest.mark.parametrize("case", range(len(LIMIT_CASES) * 3))
def test_reference_equals_cpu_oracle(case):
    max_sid, max_off, max_qoff = LIMIT_CASES[case // 3]
    tie = (2 ** 31 - 1) if max_sid >= 2 ** 31 and case % 3 == 1 else None     # a count tie across 2^31
    tk, ts, to, qk, qo, qoff = make_case(case, max_sid, max_off, max_qoff, n_rows=120, nq=4, tie_sid=tie)
    assert ts.max() == max_sid and to.max() == max_off and qo.max() == max_qoff
    topn = (1, 3, 9)[case % 3]
    want = expected_match(tk, ts, to, qk, qo, qoff, topn)
    got = _oracle(tk, ts, to, qk, qo, qoff, topn)
    for f in FIELDS:
        assert np.array_equal(want[f], got[f]), (case, f)
    assert want["nres"].min() >= 1 and want["npairs"].min() > 0


def test_reference_ties_and_extreme_deltas():
    """hand-made: two songs tie on count (the smaller id first), one song has two deltas of equal count (the smaller
    delta wins), deltas of 2^32 - 1 and -(2^20 - 1), a hash the table does not hold, an empty query"""
    K = np.int64(0xABCD1234)
    tk = np.array([K, K, K, K, 7, 7, 9], np.int64)
    ts = np.array([2 ** 32 - 1, 2 ** 24 - 1, 5, 5, 5, 2 ** 24, 3], np.int64)
    to = np.array([2 ** 32 - 1, 2 ** 32 - 1, 10, 20, 0, 0, 0], np.int64)
    qk = np.array([K, 7, 7, 123456, K, K, 7], np.int64)
    qo = np.array([0, 2 ** 20 - 1, 2 ** 20 - 1, 0, 0, 10, 0], np.int64)
    qoff = np.array([0, 4, 4, 7], np.int64)
    for topn in (1, 2, 8):
        want = expected_match(tk, ts, to, qk, qo, qoff, topn)
        got = _oracle(tk, ts, to, qk, qo, qoff, topn)
        for f in FIELDS:
            assert np.array_equal(want[f], got[f]), (topn, f)
    w = expected_match(tk, ts, to, qk, qo, qoff, 8)
    # query 0: songs 2^24-1 and 2^32-1 tie at delta 2^32-1 (one vote each), songs 5 and 2^24 at -(2^20-1) likewise; song 5
    # also votes 10 and 20 (one each): its first max is its smallest delta
    assert w["sid"][0, :4].tolist() == [5, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1]
    assert w["delta"][0, :4].tolist() == [-(2 ** 20 - 1), 2 ** 32 - 1, -(2 ** 20 - 1), 2 ** 32 - 1]
    assert w["dedup"][0, 0] == 3 and w["nhash"][0] == 3 and w["npairs"][0] == 6
    assert w["nres"][1] == 0 and w["nhash"][1] == 0
    # query 2: song 5 votes 0 twice and 10 twice (a delta tie: 0 wins), songs 2^24-1 and 2^32-1 once at 2^32-11 and
    # 2^32-1 (the smaller), song 2^24 once at 0
    assert w["sid"][2, :4].tolist() == [5, 2 ** 24 - 1, 2 ** 24, 2 ** 32 - 1]
    assert w["delta"][2, :4].tolist() == [0, 2 ** 32 - 11, 0, 2 ** 32 - 11]
    assert w["aligned"][2, :4].tolist() == [2, 1, 1, 1] and w["nres"][2] == 4
