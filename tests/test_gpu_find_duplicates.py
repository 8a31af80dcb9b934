"""GPU: find_duplicates end to end from audio.  Twelve 10 s clips of the music-like synthetic corpus (seed 77) are
fingerprinted and inserted as songs 1 .. 12; clip 0 is inserted again as song 13 (a re-upload); the hashes of clip 1's
samples from frame 40 on -- the cut lies on a multiple of the 2,048-sample hop, so the frames coincide -- become song 14 (an
excerpt).

Checked beforehand on the CPU with oracle/cpu_ref.py (fingerprint_keys of the same fourteen sample arrays into a DictDB,
return_matches + vote of every song's own hashes, the song itself left out), for this seed:
  * the excerpt's first match is clip 1 (song 2) at delta 40 with 2,537 aligned of its 2,682 hashes (0.946); song 2 has 3,218
    (0.788 covered);
  * the copy's first match is song 1 at delta 0 with all 3,090 hashes of both;
  * between unrelated songs the largest aligned count is 22 and the largest coverage of the smaller song 0.0074.
The thresholds passed below come from that run: min_aligned 200 lies between 22 and 2,537; min_coverage 0.9 lies above every
unrelated pair and between the two sides of the excerpt (0.788 and 0.946), so the excerpt is "b_in_a" and the copy alone is
"same".  Extraction is deterministic and batch-invariant (tests/test_gpu_batch_invariance.py), so the copy's counts are exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, N_CLIPS, N_SAMPLES, CUT_FRAMES = 77, 12, 10 * 44100, 40
MIN_ALIGNED, MIN_COVERAGE = 200, 0.9       # from the oracle run above
COPY, EXCERPT = 13, 14


@pytest.fixture(scope="module")
def catalogue():
    import shazam_amd as S
    ctx = S.get_context(0)
    d = ctx.synth_corpus(1, SEED, 0, N_CLIPS, N_SAMPLES)
    pcm = d.download(np.int16, N_CLIPS * N_SAMPLES).reshape(N_CLIPS, N_SAMPLES)
    d.free()
    clips = [pcm[c] for c in range(N_CLIPS)] + [pcm[0], pcm[1][CUT_FRAMES * 2048:]]
    k, t1, ho = S.fingerprint_batch(clips, ctx=ctx)
    db = S.get_database("hip")(ctx=ctx)
    for c in range(len(clips)):
        kk, tt = k[ho[c]:ho[c + 1]], t1[ho[c]:ho[c + 1]]
        sid = db.insert_song(f"clip{c}", f"{c:040X}", len(set(zip(kk.tolist(), tt.tolist()))))
        assert sid == c + 1
        db.insert_keys(sid, kk, tt)
        db.set_song_fingerprinted(sid)
    db.finalize()
    yield S, db
    db.close()


def _pairs(out):
    return {(int(p["a"]), int(p["b"])): p for p in out["pairs"]}


def test_copy_and_excerpt_are_found_and_nothing_else(catalogue):
    S, db = catalogue
    out = db.find_duplicates(topn=5, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    p = _pairs(out)
    assert set(p) == {(1, COPY), (2, EXCERPT)}, sorted(p)
    rows1 = db.table.song_rows(1)
    assert rows1 == db.songs[1]["total_hashes"] == db.songs[COPY]["total_hashes"] == 3090
    c = p[(1, COPY)]
    assert c["delta"] == 0 and c["aligned"] == c["rows_a"] == c["rows_b"] == rows1
    assert c["coverage_a"] == 1.0 and c["coverage_b"] == 1.0 and c["relation"] == "same"
    assert out["clusters"] == [[1, COPY]]
    e = p[(2, EXCERPT)]
    assert e["delta"] == -CUT_FRAMES                       # off_b - off_a: the excerpt's frame 0 is clip 1's frame 40
    assert (e["aligned"], e["rows_a"], e["rows_b"]) == (2537, 3218, 2682)      # the oracle's figures
    assert e["relation"] == "b_in_a"
    assert int((out["pairs"]["relation"] == "same").sum()) == 1          # no other pair is "same"
    # the excerpt's own top match: clip 1 at delta 40
    top = S.match_songs(db, [EXCERPT], topn=1)
    assert top["nres"][0] == 1 and top["sid"][0, 0] == 2 and top["delta"][0, 0] == CUT_FRAMES and top["aligned"][0, 0] == 2537
    assert top["rows"][0] == top["nhash"][0] == 2682


def test_listed_songs_in_batches_and_below_the_thresholds(catalogue):
    S, db = catalogue
    whole = S.find_duplicates(db, topn=5, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    # two listed songs, one song a batch: both pairs are seen from b's side alone, their partners' rows come from a count
    out = S.find_duplicates(db, sids=[EXCERPT, COPY], topn=5, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE, batch_rows=1)
    assert np.array_equal(out["pairs"], whole["pairs"]) and out["clusters"] == whole["clusters"]
    small = S.find_duplicates(db, topn=5, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE, batch_rows=7000)
    assert np.array_equal(small["pairs"], whole["pairs"]) and small["clusters"] == whole["clusters"]
    # with the bar at 1 the unrelated pairs show: none above the oracle's 22 aligned, none "same" but the copy
    low = S.find_duplicates(db.table, topn=5, min_aligned=1, min_coverage=MIN_COVERAGE)
    rest = [x for x in low["pairs"] if (int(x["a"]), int(x["b"])) not in ((1, COPY), (2, EXCERPT))]
    assert len(rest) > 10 and max(int(x["aligned"]) for x in rest) == 22
    assert max(max(x["coverage_a"], x["coverage_b"]) for x in rest) < 0.0075
    assert all(x["relation"] == "overlap" for x in rest) and low["clusters"] == [[1, COPY]]
    # a song that is not there, and no songs at all
    none = S.find_duplicates(db, sids=[99], min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    assert len(none["pairs"]) == 0 and none["clusters"] == []
    none = S.find_duplicates(db, sids=[], min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    assert len(none["pairs"]) == 0 and none["clusters"] == []


def test_sharded_database_refuses(catalogue):
    S, db = catalogue
    sharded = S.get_database("hip")(ctx=db.ctx, shards=2)
    with pytest.raises(NotImplementedError):
        sharded.find_duplicates()
    with pytest.raises(NotImplementedError):
        S.find_duplicates(sharded)
    with pytest.raises(NotImplementedError):
        S.match_songs(sharded, [1])
    sharded.close()
