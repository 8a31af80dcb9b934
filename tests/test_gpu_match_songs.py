"""GPU: shz_match_songs -- listed songs matched against the rest of the table in one call -- against expected_match of
tests/test_match_layout_ref.py, the project's int64 statement of the reference's return_matches + align_matches: it is run
on the exported rows with every listed song's rows as a query and topn + 1, and the song itself is stripped in numpy.  The
expected value never comes from Table.match of the same library.  Every comparison is exact.

The table: 30 random songs of 30 to 300 rows over a shared key pool, in three segments, and the plants
  B      A's rows at offset + 17 under another id: aligned == rows of A at delta 17 (an exact duplicate);
  C      the middle third of A's rows (by offset): an excerpt, fully covered by A at delta 0;
  D, E   twenty of A's rows each, at deltas 100 and 200, among rows of their own: equal counts against A, the smaller id first;
  F      seven copies of one song (topn + 2 for topn = 5): listed with the largest id of them, the song itself falls off its
         own topn + 1 list -- six copies with smaller ids tie with it at the full count;
  LONE   a song that shares no key with anyone: nres == 0;
  NOROWS a listed id inside the range without rows: everything zero."""
import numpy as np
import pytest

from test_match_layout_ref import FIELDS, expected_match

pytestmark = pytest.mark.gpu

A, B, C, D, E = 5, 41, 42, 43, 44
F, F_COPIES = 10, (45, 46, 47, 48, 49, 50)
LONE, NOROWS, LAST = 51, 52, 53
LISTED = [B, 50, A, 17, NOROWS, C, E, D, F, LONE, 3, 29, LAST, 47]


def make_table(seed=2024):
    """rows (key32, sid, off) as int64, every row once"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 31, 1500, dtype=np.int64))
    ks, ss, os_ = [], [], []

    def song(sid, n, keys=pool):
        cell = rng.choice(len(keys) * 400, n, replace=False)               # distinct (key, offset) pairs
        ks.append(keys[cell // 400]); ss.append(np.full(n, sid, np.int64)); os_.append(cell % 400)
        return keys[cell // 400], cell % 400

    own = {}
    for sid in range(1, 31):
        own[sid] = song(sid, int(rng.integers(30, 301)))
    ak, ao = own[A]
    ks.append(ak); ss.append(np.full(len(ak), B, np.int64)); os_.append(ao + 17)
    by_off = np.argsort(ao, kind="stable")
    third = by_off[len(ak) // 3: 2 * len(ak) // 3]
    ks.append(ak[third]); ss.append(np.full(len(third), C, np.int64)); os_.append(ao[third])
    for sid, shift, pick in ((D, 100, slice(0, 20)), (E, 200, slice(20, 40))):
        song(sid, 60)
        ks.append(ak[pick]); ss.append(np.full(20, sid, np.int64)); os_.append(ao[pick] + shift)
    fk, fo = own[F]
    for sid in F_COPIES:
        ks.append(fk); ss.append(np.full(len(fk), sid, np.int64)); os_.append(fo)
    song(LONE, 80, keys=np.arange(1, 200, dtype=np.int64) + (1 << 31))     # keys nobody else draws from
    song(LAST, 50)
    rows = np.unique(np.stack([np.concatenate(ks), np.concatenate(ss), np.concatenate(os_)], 1), axis=0)
    rows = rows[rng.permutation(len(rows))]
    return rows[:, 0], rows[:, 1], rows[:, 2]


def build(ctx, tk, ts, to, parts=3):
    import shazam_amd as S
    t = S.Table(ctx)
    u = [np.ascontiguousarray(x, np.uint32) for x in (tk, ts, to)]
    t.set_segment_rows(max(16, (len(tk) + parts - 1) // parts))
    for part in np.array_split(np.arange(len(tk)), parts):
        t.insert(u[0][part], u[1][part], u[2][part])
        t.finalize()
    return t


def expected_songs(ex, listed, topn):
    """the arrays of match_songs from the exported rows: expected_match with topn + 1, the song itself stripped"""
    ek, es, eo = (np.asarray(x, np.int64) for x in ex)
    qk, qo, qoff = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [0]
    for s in listed:
        m = es == s
        qk.append(ek[m]); qo.append(eo[m]); qoff.append(qoff[-1] + int(m.sum()))
    w = expected_match(ek, es, eo, np.concatenate(qk), np.concatenate(qo), qoff, topn + 1)
    out = {f: np.zeros((len(listed), topn), np.int64) for f in FIELDS[:4]}
    out["nres"] = np.zeros(len(listed), np.int64)
    self_seen = []
    for q, s in enumerate(listed):
        keep = [i for i in range(int(w["nres"][q])) if w["sid"][q, i] != s]
        self_seen.append(len(keep) < int(w["nres"][q]))
        keep = keep[:topn]
        for f in FIELDS[:4]:
            out[f][q, :len(keep)] = w[f][q, keep]
        out["nres"][q] = len(keep)
    out["nhash"], out["npairs"], out["rows"] = w["nhash"], w["npairs"], np.diff(np.asarray(qoff, np.int64))
    return out, self_seen


def compare(got, want, label):
    for f in FIELDS + ("rows",):
        assert np.array_equal(np.asarray(got[f], np.int64), want[f]), f"{label}: {f}\n{got[f]}\n{want[f]}"


@pytest.fixture(scope="module")
def case():
    import shazam_amd as S
    ctx = S.get_context(0)
    tk, ts, to = make_table()
    t = build(ctx, tk, ts, to)
    assert t.segments() == 3
    ex = t.export()
    assert len(ex[0]) == len(tk)
    yield t, ex
    t.close()


@pytest.mark.parametrize("topn", (1, 5))
def test_match_songs_equals_the_reference_statement(case, topn):
    t, ex = case
    want, self_seen = expected_songs(ex, LISTED, topn)
    q = {s: i for i, s in enumerate(LISTED)}
    rows_a = int((ex[1] == A).sum())
    # the plants say what they were planted for (in the expected arrays, before the GPU is asked)
    assert want["sid"][q[A], 0] == B and want["delta"][q[A], 0] == 17 and want["aligned"][q[A], 0] == rows_a == want["rows"][q[A]]
    assert want["sid"][q[B], 0] == A and want["delta"][q[B], 0] == -17 and want["aligned"][q[B], 0] == rows_a
    assert want["sid"][q[C], 0] == A and want["delta"][q[C], 0] == 0 and want["aligned"][q[C], 0] == want["rows"][q[C]] < rows_a // 2
    assert want["nres"][q[LONE]] == 0 and want["npairs"][q[LONE]] >= want["rows"][q[LONE]] == 80   # (its pairs are its own)
    assert want["rows"][q[NOROWS]] == 0 and want["nres"][q[NOROWS]] == 0 and want["npairs"][q[NOROWS]] == 0
    assert not self_seen[q[50]] and self_seen[q[F]]                            # the largest copy fell off its own list
    assert self_seen[q[47]] == (topn == 5)                                     # (three copies carry smaller ids than 47)
    if topn == 5:
        assert want["sid"][q[50]].tolist() == [F, 45, 46, 47, 48] and (want["aligned"][q[50]] == want["rows"][q[50]]).all()
        got_a = want["sid"][q[A]].tolist()
        i = got_a.index(D)
        assert got_a[i + 1] == E and want["aligned"][q[A], i] == want["aligned"][q[A], i + 1] == 20   # a count tie: smaller id first
        assert want["delta"][q[A], i] == 100 and want["delta"][q[A], i + 1] == 200
    got = t.match_songs(LISTED, topn=topn)
    compare(got, want, f"top{topn}")
    compare(t.match_songs(LISTED, topn=topn, full_sort=True), want, f"top{topn} full_sort")
    assert np.array_equal(np.asarray(got["nhash"], np.int64), want["rows"])
    # batch invariance: the same songs in two calls, and one at a time
    cut = 6
    two = [t.match_songs(LISTED[:cut], topn=topn), t.match_songs(LISTED[cut:], topn=topn)]
    compare({f: np.concatenate([r[f] for r in two]) for f in FIELDS + ("rows",)}, want, f"top{topn} two calls")
    for s in (A, 50, NOROWS, LONE):
        one = t.match_songs([s], topn=topn)
        compare(one, {f: want[f][q[s]:q[s] + 1] for f in FIELDS + ("rows",)}, f"top{topn} song {s} alone")


def test_public_form_and_refusals(case):
    import shazam_amd as S
    from shazam_amd import _ffi
    t, ex = case
    want, _ = expected_songs(ex, LISTED, 3)
    compare(S.match_songs(t, LISTED, topn=3), want, "S.match_songs")
    for topn in (0, 64):
        with pytest.raises(S.ShzError) as e:
            t.match_songs(LISTED, topn=topn)
        assert e.value.code == _ffi.E_INVALID and "topn" in str(e.value)
    with pytest.raises(S.ShzError) as e:
        t.match_songs([A, B, A])
    assert e.value.code == _ffi.E_INVALID and "twice" in str(e.value)
    res = t.match_songs(np.zeros(0, np.uint32))
    assert res["sid"].shape == (0, 5) and len(res["rows"]) == 0
    res = t.match_songs([NOROWS, 1000], topn=2)                                  # no listed song has a row
    assert not res["nres"].any() and not res["rows"].any() and not res["sid"].any() and not res["npairs"].any()


def test_a_listed_song_at_offset_2_pow_20_is_refused():
    """a listed song's offsets are query offsets: 2^20 is one too many (2^20 - 1 still matches), and the message names it"""
    import shazam_amd as S
    from shazam_amd import _ffi
    ctx = S.get_context(0)
    tk, ts, to = make_table(seed=7)
    for top, refused in ((2 ** 20 - 1, False), (2 ** 20, True)):
        k2, s2, o2 = np.append(tk, 12345), np.append(ts, A), np.append(to, top)
        t = build(ctx, k2, s2, o2)
        ex = t.export()
        if refused:
            with pytest.raises(S.ShzError) as e:
                t.match_songs([3, A], topn=2)
            assert e.value.code == _ffi.E_UNSUPPORTED and str(2 ** 20) in str(e.value)
            compare(t.match_songs([3, B], topn=2), expected_songs(ex, [3, B], 2)[0], "beside the long song")
        else:
            compare(t.match_songs([3, A], topn=2), expected_songs(ex, [3, A], 2)[0], "offset 2^20 - 1")
        t.close()
