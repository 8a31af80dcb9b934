"""GPU: recognize(..., extents=True) and find_duplicates(..., extents=True) on real hashes.

The table holds eight 10 s clips of the music-like synthetic corpus (oracle.synth.music_clip, seed 91) as songs 1 .. 8, and
song 9, the samples of clip 1 from frame 40 on (an excerpt; the cut lies on a multiple of the 2,048-sample hop).  The query is
PRE = 64 hops of traffic_noise, then CUTN = 86 hops (3.99 s) cut from clip 3 at frame CUT0 = 70, then 65 hops of
traffic_noise: frame f of the query covers the samples [2048 f, 2048 f + 4096), so the frames 64 .. 148 lie inside the excerpt
and 63 and 149 straddle its two cuts.

The margin: run beforehand on the CPU with oracle/cpu_ref.py -- fingerprint_keys of the eight clips and of the query,
return_matches + the vote of tests/vote_tol_twin.py, then tests/extent_twin.py on the winner -- this fixture gives song 4 at
delta 6 with 1,167 aligned of 2,750 query hashes, and q_first = 65, q_last = 148, t_first = 71, t_last = 154: both ends lie
INSIDE the excerpt's frames 64 .. 149 (a hash needs both of its peaks inside the excerpt), so the margin is 0 frames.  The
runners-up there are chance: song 6 with 9 pairs, all at query frame 72, and song 1 with 3."""
import numpy as np
import pytest

from extent_twin import extents

pytestmark = pytest.mark.gpu

SEED, N_CLIPS, N_SAMPLES = 91, 8, 10 * 44100
PRE, CUT0, CUTN, POST, TARGET = 64, 70, 86, 65, 3
EXCERPT_OF, EXCERPT_CUT, EXCERPT_SID = 1, 40, 9
MARGIN = 0                                       # frames; from the oracle run in the docstring
EXTENT_KEYS = {"query_first", "query_last", "song_first", "song_last", "query_start_secs", "query_end_secs", "song_start_secs",
               "song_end_secs", "extent_hist", "extent_shift"}


@pytest.fixture(scope="module")
def fixture():
    import shazam_amd as S
    from oracle import synth
    ctx = S.get_context(0)
    songs = [synth.music_clip(SEED, c, N_SAMPLES) for c in range(N_CLIPS)]
    clips = songs + [songs[EXCERPT_OF][EXCERPT_CUT * 2048:]]
    k, t1, ho = S.fingerprint_batch(clips, ctx=ctx)
    db = S.get_database("hip")(ctx=ctx)
    for c in range(len(clips)):
        kk, tt = k[ho[c]:ho[c + 1]], t1[ho[c]:ho[c + 1]]
        sid = db.insert_song(f"clip{c}", f"{c:040X}", len(set(zip(kk.tolist(), tt.tolist()))))
        assert sid == c + 1
        db.insert_keys(sid, kk, tt)
        db.set_song_fingerprinted(sid)
    db.finalize()
    query = np.concatenate([synth.traffic_noise(SEED, 100, PRE * 2048), songs[TARGET][CUT0 * 2048:(CUT0 + CUTN) * 2048],
                            synth.traffic_noise(SEED, 101, POST * 2048)])
    yield S, db, query
    db.close()


def _secs(frames):
    return round(float(frames) / 44100 * 4096 * 0.5, 5)


def test_recognize_says_where_the_song_plays(fixture):
    S, db, query = fixture
    got, *_ = S.recognize(query, db=db, topn=3, extents=True)
    assert got and got[0]["song_id"] == TARGET + 1 and got[0]["offset"] == CUT0 - PRE
    # the twin on the query's own hashes and the table's export
    qk, qt, _ = S.fingerprint_batch([query], ctx=db.ctx)
    tk, ts, to = db.table.export()
    want, shift = extents(zip(tk.tolist(), ts.tolist(), to.tolist()), zip(qk.tolist(), qt.tolist()),
                          [(r["song_id"], r["offset"], r["offset"]) for r in got])
    for r, w in zip(got, want):
        assert EXTENT_KEYS <= set(r)
        assert (r["query_first"], r["query_last"], r["song_first"], r["song_last"]) == (w["q_first"], w["q_last"], w["t_first"], w["t_last"])
        assert r["extent_hist"].tolist() == w["hist"] and r["extent_shift"] == shift and sum(w["hist"]) == w["count"] > 0
        assert r["query_start_secs"] == _secs(w["q_first"]) and r["query_end_secs"] == _secs(w["q_last"] + 1)
        assert r["song_start_secs"] == _secs(w["t_first"]) and r["song_end_secs"] == _secs(w["t_last"] + 1)
    top = got[0]
    print("extent of the winner:", top["query_first"], top["query_last"], top["song_first"], top["song_last"])
    assert PRE - MARGIN <= top["query_first"] <= top["query_last"] <= PRE + CUTN - 1 + MARGIN
    assert top["song_first"] - top["query_first"] == CUT0 - PRE == top["song_last"] - top["query_last"]
    assert top["query_last"] - top["query_first"] >= CUTN - 8                 # ... and it fills the excerpt
    from shazam_amd.extent import dense_span
    a, b = dense_span(top["extent_hist"], top["extent_shift"])
    w = 1 << top["extent_shift"]
    assert PRE - w < a <= top["query_first"] and top["query_last"] < b <= PRE + CUTN - 1 + w


def test_without_extents_the_dicts_are_todays(fixture):
    S, db, query = fixture
    plain, *_ = S.recognize(query, db=db, topn=3)
    assert plain and not (EXTENT_KEYS & set(plain[0]))
    ext, *_ = S.recognize(query, db=db, topn=3, extents=True)
    assert [{k: v for k, v in r.items() if k not in EXTENT_KEYS} for r in ext] == plain
    batch, _ = S.recognize_batch([query, query[: 40 * 2048]], db, topn=3, extents=False)
    assert batch[0] == plain
    # at a tolerance the range widens with it: a superset of the winning window, never fewer pairs
    tol, *_ = S.recognize(query, db=db, topn=1, extents=True, delta_tol=2)
    assert tol[0]["song_id"] == TARGET + 1 and int(tol[0]["extent_hist"].sum()) >= int(ext[0]["extent_hist"].sum())
    assert db.ctx.vote_tolerance == 0
    with pytest.raises(ValueError):
        S.recognize(query, db=db, fused=True, extents=True)
    with pytest.raises(ValueError):
        S.recognize_batch([query], db, fused=True, extents=True)


def test_find_duplicates_reports_the_position_of_an_excerpt(fixture):
    S, db, _ = fixture
    from shazam_amd.catalog import EXTENT_PAIR_FIELDS, PAIR_FIELDS
    plain = db.find_duplicates(topn=3)
    assert plain["pairs"].dtype == np.dtype(list(PAIR_FIELDS))
    out = db.find_duplicates(topn=3, extents=True)
    assert out["pairs"].dtype == np.dtype(list(EXTENT_PAIR_FIELDS)) and out["clusters"] == plain["clusters"]
    for f, _ in PAIR_FIELDS:
        assert np.array_equal(out["pairs"][f], plain["pairs"][f]), f
    a, b = EXCERPT_OF + 1, EXCERPT_SID
    assert [(int(p["a"]), int(p["b"])) for p in out["pairs"]] == [(a, b)]
    p = out["pairs"][0]
    assert p["delta"] == -EXCERPT_CUT
    tk, ts, to = db.table.export()
    _, ak, ao = db.table.song_hashes([a])
    want, _ = extents(zip(tk.tolist(), ts.tolist(), to.tolist()), zip(ak.tolist(), ao.tolist()), [(b, -EXCERPT_CUT, -EXCERPT_CUT)])
    w = want[0]
    assert (int(p["a_first"]), int(p["a_last"]), int(p["b_first"]), int(p["b_last"])) == (w["q_first"], w["q_last"], w["t_first"], w["t_last"])
    assert w["count"] == int(p["aligned"])
    # the excerpt begins at frame 40 of the longer track and runs to its end: the first frames of song 9 are song 2's 40 ..
    assert int(p["a_first"]) - EXCERPT_CUT == int(p["b_first"]) <= 2 and int(p["a_last"]) - EXCERPT_CUT == int(p["b_last"])
    assert int(p["a_last"]) >= int(ao.max()) - 2
    one_by_one = S.find_duplicates(db, topn=3, extents=True, batch_rows=1)
    assert np.array_equal(one_by_one["pairs"], out["pairs"])
    with pytest.raises(ValueError):
        db.find_duplicates(extents=True, speeds=[65536])
    none = S.find_duplicates(db, sids=[], extents=True)
    assert len(none["pairs"]) == 0 and none["pairs"].dtype == np.dtype(list(EXTENT_PAIR_FIELDS))
