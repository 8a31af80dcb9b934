"""GPU: the key cap gives one answer through every door of the library.  One small fixture -- three synthetic clips of 4 s,
one of them in the table under three song ids, so that its keys hold three rows and the others' one -- and a cap chosen
from Table.key_hist() that drops some keys and keeps others.  Doors: recognize_batch fused, in two calls, and as
fingerprint_batch + Table.match; scan_windows against the windows' hash lists; match_songs inside `with ctx.key_cap(c)`
against the gathered rows; match_extents against extent_twin on the masked table.  Every comparison is exact."""
import numpy as np
import pytest

from extent_twin import assert_extents
from key_cap_twin import expected_extents_cap, kept_rows
from shazam_amd import floor, keycap
from test_gpu_vote_floor import ARRAYS, _host_windows, _same

pytestmark = pytest.mark.gpu

SR = 44100
OWNER = [0, 0, 1, 2, 0]          # song id s + 1 holds clip OWNER[s]: clip 0 three times


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def clips():
    from oracle import synth
    return [synth.synth_clip(31, c, 4 * SR, 4000, 1500) for c in range(3)]


@pytest.fixture(scope="module")
def env(S, ctx, clips):
    """(database, cap): songs 1, 2 and 5 are clip 0, song 3 clip 1, song 4 clip 2; the cap is the upper edge of the lowest
    occupied bucket of the key histogram, so the keys of that bucket stay and the largest key goes"""
    k, t1, ho = S.fingerprint_batch(clips, ctx=ctx)
    d = S.get_database("hip")(ctx=ctx)
    for s, c in enumerate(OWNER):
        assert d.insert_song(f"song{s}", "AB" * 20, int(ho[c + 1] - ho[c])) == s + 1
        d.set_song_fingerprinted(s + 1)
        d.table.insert(k[int(ho[c]):int(ho[c + 1])], s + 1, t1[int(ho[c]):int(ho[c + 1])])
    d.table.finalize()
    h = d.key_hist()
    lowest = int(np.flatnonzero(h["keys"])[0])
    cap = keycap.bucket_hi(lowest)
    assert int(h["keys"][lowest]) > 0 and floor.bucket_of(cap) == lowest        # some key is kept ...
    assert h["max_rows"] > cap and h["max_rows"] >= 3                           # ... and some key is dropped
    assert 0 < keycap.rows_kept(h, cap) < int(h["rows"].sum())
    yield d, cap
    d.close()


@pytest.fixture(scope="module")
def queries(clips):
    """clip 0 (its keys hold three rows), clip 1, and a stereo query of clip 2 with noise on one channel"""
    from oracle import synth
    noisy = synth.mix_query(clips[2][SR // 2:3 * SR], synth.synth_clip(5, 9, 3 * SR - SR // 2, 0, 8000), 6.0)
    return [clips[0][SR:3 * SR + 700], clips[1][SR // 3:3 * SR], [clips[2][SR // 2:3 * SR], noisy]]


def test_recognize_batch_fused_unfused_and_match(S, ctx, env, queries):
    db, cap = env
    fused, tf = S.recognize_batch(queries, db, topn=3, fused=True, max_key_rows=cap)
    two, tt = S.recognize_batch(queries, db, topn=3, max_key_rows=cap)
    assert fused == two
    assert np.array_equal(tf["n_matches"], tt["n_matches"]) and np.array_equal(tf["n_hashes"], tt["n_hashes"])
    chans = [queries[0], queries[1], queries[2][0], queries[2][1]]
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    res = db.table.match(k, t1, ho[[0, 1, 2, 4]], 3, max_key_rows=cap)
    assert np.array_equal(tt["n_matches"], res["npairs"]) and np.array_equal(tt["n_hashes"], res["nhash"])
    for q in range(3):
        assert [r["song_id"] for r in two[q]] == res["sid"][q, :int(res["nres"][q])].tolist(), q
    assert ctx.key_cap_stats()["groups"] > 0 and ctx.key_cap == 0
    plain, tp = S.recognize_batch(queries, db, topn=3)
    assert plain[0][0]["song_id"] in (1, 2, 5) and int(tp["n_matches"][0]) > int(tt["n_matches"][0])
    assert np.array_equal(tp["n_hashes"], tt["n_hashes"])                       # nhash comes from the query alone
    assert two[1][0]["song_id"] == 3 == plain[1][0]["song_id"] and two[2][0]["song_id"] == 4
    one, *_ = S.recognize(queries[1], db=db, topn=3, max_key_rows=cap)
    assert one == two[1]
    with ctx.key_cap(cap):
        inside, _ = S.recognize_batch(queries, db, topn=3, fused=True)
    assert inside == fused and ctx.key_cap == 0


def test_scan_windows(S, ctx, env, clips):
    db, cap = env
    recs = [np.concatenate([clips[0][0:3 * SR], clips[1][SR:4 * SR]]), [clips[2][0:3 * SR], clips[2][SR // 4:3 * SR + SR // 4]]]
    chans = [recs[0], recs[1][0], recs[1][1]]
    first = np.array([0, 1, 3], np.uint32)
    k, t1, ho = S.fingerprint_batch(chans, ctx=ctx)
    got = S.scan_windows(recs, db, window_seconds=2, step_seconds=1, topn=2, max_key_rows=cap)
    hk, hq, hqo = _host_windows(ctx, [S._as_pcm(c) for c in chans], first, k, t1, ho, got["window_frames"], got["step_frames"])
    want = db.table.match(hk, hq, hqo, 2, max_key_rows=cap)
    _same(got, want, "scan_windows under the cap")
    plain = S.scan_windows(recs, db, window_seconds=2, step_seconds=1, topn=2)
    assert int(plain["npairs"].sum()) > int(got["npairs"].sum()) > 0 and np.array_equal(plain["nhash"], got["nhash"])
    assert len(got["nres"]) == int(got["win_off"][-1]) > 4 and ctx.key_cap == 0


def test_match_songs_inside_the_block(S, ctx, env):
    db, cap = env
    t, listed, topn = db.table, [1, 3, 5, 4], 2
    with ctx.key_cap(cap):
        got = S.match_songs(db, listed, topn=topn)
    ro, qk, qo = t.song_hashes(listed)                                         # the gather is not capped: a song's own rows
    w = t.match(qk, qo, ro, topn + 1, max_key_rows=cap)
    for q, s in enumerate(listed):                                             # the song itself left out
        keep = [i for i in range(int(w["nres"][q])) if int(w["sid"][q, i]) != s][:topn]
        assert int(got["nres"][q]) == len(keep), q
        for f in ("sid", "delta", "aligned", "dedup"):
            assert got[f][q, :len(keep)].tolist() == w[f][q, keep].tolist() and not got[f][q, len(keep):].any(), (q, f)
    assert np.array_equal(got["nhash"], w["nhash"]) and np.array_equal(got["npairs"], w["npairs"])
    assert np.array_equal(got["rows"], np.diff(ro))
    plain = S.match_songs(db, listed, topn=topn)
    assert plain["sid"][0, :2].tolist() == [2, 5] and int(got["nres"][0]) == 0          # clip 0's copies are found by the dropped keys
    assert (got["npairs"] <= plain["npairs"]).all() and int(got["npairs"].sum()) < int(plain["npairs"].sum())
    assert ctx.key_cap == 0


def test_match_extents_inside_the_block(S, ctx, env, queries):
    db, cap = env
    t = db.table
    tk, ts, to = t.export()
    chans = [queries[0], queries[1], queries[2][0]]
    qk, qo, qoff = S.fingerprint_batch(chans, ctx=ctx)
    plain = t.match(qk, qo, qoff, 3)
    cs = plain["sid"].astype(np.uint32)                                        # the plain match's candidates: songs 1, 2, 5 among them
    lo, hi, cn = plain["delta"] - 2, plain["delta"] + 2, plain["nres"]
    assert {1, 2, 5} <= set(cs[0, :int(cn[0])].tolist()) and int(cn.min()) >= 1
    off = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn)
    with ctx.key_cap(cap):
        got = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn)
        fit = t.match_extents(qk, qo, qoff, cs, lo, hi, cand_n=cn, hist=False, fit=True)
    assert_extents(got, expected_extents_cap(tk, ts, to, qk, qo, qoff, cs.tolist(), lo.tolist(), hi.tolist(), cap, cand_n=cn))
    assert np.array_equal(fit["count"], got["count"]) and np.array_equal(fit["q_first"], got["q_first"])
    m = kept_rows(tk, cap, ts, to)
    assert not m[np.isin(ts, [1, 2, 5])].all() and m[ts == 3].any()
    assert int(got["count"][0].sum()) < int(off["count"][0].sum()) and int(got["count"][1, 0]) > 0
    assert ctx.key_cap == 0
