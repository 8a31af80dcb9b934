"""GPU: find_duplicates at a speed ladder, end to end from audio.  The catalogue of tests/test_gpu_find_duplicates.py: twelve
10 s clips of the music-like synthetic corpus (seed 77) are songs 1 .. 12; song 13 is clip 0 played 1.03 times as fast and
song 14 is clip 1 played 0.97 times as fast, both made by tests/speed_twin.py's speed_up (linear interpolation; not by the
code under test).

Checked beforehand on the CPU with oracle/cpu_ref.py and tests/rows_warp_twin.py (fingerprint_keys of the same fourteen
sample arrays, every song's rows warped at {q16(0.97), 65536, q16(1.03)} and voted against a dict table, the song itself left
out), for this seed:
  * 13 -> 1 at 1.03: 466 aligned at delta 0 (0.149 of song 13, 0.151 of song 1); 14 -> 2 at 0.97: 426 at delta 0 (0.133 / 0.132);
  * from the other side the rung misses the true factor (1 / 1.03 = 0.97087) by 0.09 %: 1 -> 13 at 0.97: 200, 2 -> 14 at 1.03: 189;
  * between unrelated songs the largest aligned count at ANY rung is 22.
The thresholds passed below come from that run: min_aligned 100 lies between 22 and 426, min_coverage 0.1 below 0.132.  The
GPU extraction decides exact ties in the spectrogram as the reference does but its hashes of resampled audio are not pinned
to the oracle's count here, so the counts are asserted as >= 300 rather than equal to 466 and 426."""
import numpy as np
import pytest

from speed_twin import q16, speed_up

pytestmark = pytest.mark.gpu

SEED, N_CLIPS, N_SAMPLES = 77, 12, 10 * 44100
MIN_ALIGNED, MIN_COVERAGE = 100, 0.1       # from the oracle run above
FAST, SLOW = 13, 14
SPEEDS = np.array([q16(0.97), 65536, q16(1.03)], np.uint32)


@pytest.fixture(scope="module")
def catalogue():
    import shazam_amd as S
    ctx = S.get_context(0)
    d = ctx.synth_corpus(1, SEED, 0, N_CLIPS, N_SAMPLES)
    pcm = d.download(np.int16, N_CLIPS * N_SAMPLES).reshape(N_CLIPS, N_SAMPLES)
    d.free()
    clips = [pcm[c] for c in range(N_CLIPS)] + [speed_up(pcm[0], 1.03), speed_up(pcm[1], 0.97)]
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


def _same_but_plain(x, y):
    """the same records; aligned_plain left out: it is the greater of the sides that were LISTED, and a song's plain topn
    need not hold the partner that its partner's holds"""
    names = [n for n in x["pairs"].dtype.names if n != "aligned_plain"]
    return x["pairs"].dtype == y["pairs"].dtype and np.array_equal(x["pairs"][names], y["pairs"][names]) and x["clusters"] == y["clusters"]


def test_the_two_altered_copies_are_found_and_nothing_else(catalogue):
    S, db = catalogue
    out = db.find_duplicates(speeds=SPEEDS, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    p = _pairs(out)
    for x in out["pairs"]:
        print("pair", x)
    assert set(p) == {(1, FAST), (2, SLOW)}, sorted(p)
    assert out["pairs"].dtype.names == tuple(n for n, _ in S.catalog.WARP_PAIR_FIELDS)
    for key, s16 in (((1, FAST), q16(1.03)), ((2, SLOW), q16(0.97))):
        c = p[key]
        assert c["warped"] == "b" and c["tempo_q16"] == s16 and c["pitch_q16"] == s16     # the copy's rows, at its true factor
        assert c["delta"] == 0 and c["relation"] == "same"
        assert c["aligned"] >= 300 and c["aligned_plain"] < MIN_ALIGNED
        assert c["rows_a"] == db.table.song_rows(key[0]) and c["rows_b"] == db.table.song_rows(key[1])
        assert c["coverage_a"] == c["aligned"] / c["rows_a"] and c["coverage_b"] == c["aligned"] / c["rows_b"]
    assert out["clusters"] == [[1, FAST], [2, SLOW]]
    # the plain search sees neither
    plain = db.find_duplicates(min_aligned=MIN_ALIGNED)
    assert len(plain["pairs"]) == 0 and plain["clusters"] == []
    assert plain["pairs"].dtype.names == tuple(n for n, _ in S.catalog.PAIR_FIELDS)


def test_batches_listed_songs_and_the_unrelated_pairs(catalogue):
    S, db = catalogue
    whole = S.find_duplicates(db, speeds=SPEEDS, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    # one song a batch; the two copies alone are listed: both pairs are seen from b's side, their partners' rows come from a count
    out = S.find_duplicates(db, sids=[SLOW, FAST], speeds=SPEEDS, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE, batch_rows=1)
    assert _same_but_plain(out, whole)
    small = S.find_duplicates(db, speeds=SPEEDS, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE, batch_rows=20000)
    assert np.array_equal(small["pairs"], whole["pairs"]) and small["clusters"] == whole["clusters"]
    # the originals alone: a's side, whose rung misses 1 / 1.03 by 0.09 % -- fewer rows align (the oracle: 200 and 189), same pairs
    orig = S.find_duplicates(db, sids=[1, 2], speeds=SPEEDS, min_aligned=MIN_ALIGNED, min_coverage=0.03)
    po, pw = _pairs(orig), _pairs(whole)
    assert set(po) == set(pw)
    assert po[(1, FAST)]["warped"] == "a" and po[(1, FAST)]["tempo_q16"] == q16(0.97) and po[(2, SLOW)]["tempo_q16"] == q16(1.03)
    assert MIN_ALIGNED <= po[(1, FAST)]["aligned"] < pw[(1, FAST)]["aligned"]
    # with the bar at 1 the unrelated pairs show: far below the bar at every rung
    low = S.find_duplicates(db, speeds=SPEEDS, min_aligned=1, min_coverage=MIN_COVERAGE)
    rest = [x for x in low["pairs"] if (int(x["a"]), int(x["b"])) not in pw]
    print("unrelated: max aligned", max(int(x["aligned"]) for x in rest))
    assert len(rest) > 10 and max(int(x["aligned"]) for x in rest) < MIN_ALIGNED // 2
    assert low["clusters"] == whole["clusters"]
    # tempos= with pitches= is their product, warps= an explicit list: the diagonal written both ways is the speed ladder
    grid = S.find_duplicates(db, sids=[FAST, SLOW], tempos=SPEEDS, pitches=SPEEDS, min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    listw = S.find_duplicates(db, sids=[FAST, SLOW], warps=(SPEEDS, SPEEDS), min_aligned=MIN_ALIGNED, min_coverage=MIN_COVERAGE)
    assert _same_but_plain(listw, whole)
    assert set(_pairs(grid)) == set(pw) and all(_pairs(grid)[k]["aligned"] >= pw[k]["aligned"] for k in pw)   # (nine pairs: no fewer)
    none = S.find_duplicates(db, sids=[], speeds=SPEEDS)
    assert len(none["pairs"]) == 0 and none["clusters"] == []


def test_sharded_database_refuses_the_ladder_too(catalogue):
    S, db = catalogue
    sharded = S.get_database("hip")(ctx=db.ctx, shards=2)
    with pytest.raises(NotImplementedError):
        sharded.find_duplicates(speeds=SPEEDS)
    with pytest.raises(NotImplementedError):
        S.find_duplicates(sharded, speeds=SPEEDS)
    with pytest.raises(NotImplementedError):
        S.match_songs(sharded, [1], speeds=SPEEDS)
    sharded.close()
