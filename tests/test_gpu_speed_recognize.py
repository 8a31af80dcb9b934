"""GPU: recognize_speeds -- the peaks of every query extracted once, warped for every factor of a ladder, all variants in one
match -- equals the CPU pipeline exactly: oracle.cpu_ref.fingerprint_keys on every channel, the numpy twin of the warp
(tests/speed_twin.py) per factor, the reference's vote per variant, the same best-variant rule.  Song ids, offsets, aligned
and dedup counts, the best index and the whole speed profile are compared for equality (the extraction is bit-exact with
the oracle).  The chosen factor is within one rung of the truth, the offset within one frame of the cut; slicing the
queries x speeds into several match passes changes nothing; 48 kHz queries go through resample_to."""
import numpy as np
import pytest

import speed_twin as T

pytestmark = pytest.mark.gpu

SR = 44100
N_SONGS, SONG_S, QUERY_S = 16, 30, 10
TRUE = [0.96, 1.0, 1.03, 0.96, 1.0, 1.03]     # speed of query i; query i is cut from song 2 i + 1 at second 5 + i
TOPN = 2


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def songs():
    from oracle import synth
    return [synth.music_clip(7, c, SONG_S * SR) for c in range(N_SONGS)]


@pytest.fixture(scope="module")
def ladder():
    """21 rungs on the default grid (step 92 / 65536, anchored at 65536): the rung nearest each true factor and three on
    either side of it."""
    from shazam_amd.speed import DEFAULT_STEP_Q16 as st
    rungs = set()
    for s in sorted(set(TRUE)):
        mid = 65536 + st * int(round((T.q16(s) - 65536) / st))
        rungs |= {mid + st * k for k in range(-3, 4)}
    lad = np.asarray(sorted(rungs), np.uint32)
    assert len(lad) == 21 and 65536 in lad.tolist()
    return lad


def _cut(song, second, s):
    return T.speed_up(song[second * SR: second * SR + int(QUERY_S * SR * s) + 2], s)[:QUERY_S * SR]


@pytest.fixture(scope="module")
def queries(songs):
    from oracle import synth
    qs = []
    for i, s in enumerate(TRUE):
        x = _cut(songs[2 * i + 1], 5 + i, s)
        if i == 3:   # stereo: the second channel carries noise at 10 dB
            qs.append([x, synth.mix_query(x, synth.synth_clip(5, 9, len(x), 0, 8000), 10.0)])
        else:
            qs.append(x)
    return qs


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    """Songs 1..16; returns (db, key32 -> [(sid, offset)]): one set of rows for the device table and for the CPU vote."""
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(songs, ctx=ctx)
    per_song = []
    for c in range(N_SONGS):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        assert sid == c + 1
        d.set_song_fingerprinted(sid)
        per_song.append((k[int(ho[c]):int(ho[c + 1])], t1[int(ho[c]):int(ho[c + 1])]))
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    yield d, T.table_of(per_song)
    d.close()


@pytest.fixture(scope="module")
def expected(queries, db, ladder):
    """The CPU pipeline, once: per query the peaks of every channel (oracle), per factor the twin's hashes and the vote."""
    from oracle import cpu_ref as O
    _, table = db
    nq, K = len(queries), len(ladder)
    exp = {"sid": np.zeros((nq, K, TOPN), np.uint32), "delta": np.zeros((nq, K, TOPN), np.int32),
           "aligned": np.zeros((nq, K, TOPN), np.uint32), "dedup": np.zeros((nq, K, TOPN), np.uint32),
           "nres": np.zeros((nq, K), np.uint32), "nhash": np.zeros((nq, K), np.uint32)}
    for q, query in enumerate(queries):
        chans = [query] if isinstance(query, np.ndarray) else query
        peaks = [O.fingerprint_keys(c)[2:] for c in chans]
        for v, s16 in enumerate(ladder.tolist()):
            hk = [T.warp_pair(f, t, s16) for f, t in peaks]
            ranked, dedup, nhash = T.aligned_votes(np.concatenate([k for k, _ in hk]), np.concatenate([t for _, t in hk]), table, TOPN)
            exp["nres"][q, v], exp["nhash"][q, v] = len(ranked), nhash
            for n, (sid, delta, aligned) in enumerate(ranked):
                exp["sid"][q, v, n], exp["delta"][q, v, n], exp["aligned"][q, v, n] = sid, delta, aligned
                exp["dedup"][q, v, n] = dedup[sid]
    exp["profile"] = np.where(exp["nres"] > 0, exp["aligned"][:, :, 0], 0).astype(np.uint32)
    exp["best"] = np.asarray([T.best_variant(exp["profile"][q], ladder) for q in range(nq)], np.uint32)
    return exp


def _raw(S, ctx, db, queries, ladder):
    chans, first = [], [0]
    for q in queries:
        cs = [q] if isinstance(q, np.ndarray) else list(q)
        chans.extend(S._as_pcm(c) for c in cs)
        first.append(len(chans))
    off = np.zeros(len(chans) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chans])
    res, _ = ctx.recognize_speeds(db.table, np.concatenate(chans), off, np.asarray(first, np.uint32), ladder, topn=TOPN)
    return res


def _assert_equals_cpu(res, exp):
    nq = len(exp["best"])
    print("profile (gpu):", res["profile"].tolist())
    print("best (gpu, cpu):", res["best"].tolist(), exp["best"].tolist())
    assert np.array_equal(res["profile"], exp["profile"])
    assert np.array_equal(res["best"], exp["best"])
    for q in range(nq):
        b = int(exp["best"][q])
        n = int(exp["nres"][q, b])
        assert int(res["nres"][q]) == n and int(res["nhash"][q]) == int(exp["nhash"][q, b])
        for name in ("sid", "delta", "aligned", "dedup"):
            assert np.array_equal(res[name][q, :n], exp[name][q, b, :n]), (name, q)


def test_equals_the_cpu_pipeline(S, ctx, db, queries, ladder, expected):
    _assert_equals_cpu(_raw(S, ctx, db[0], queries, ladder), expected)


def test_finds_speed_song_and_offset(S, db, queries, ladder):
    from shazam_amd.speed import DEFAULT_STEP_Q16 as st
    results, tm = S.recognize_speeds(queries, db[0], speeds=ladder, topn=TOPN)
    assert tm["speed_profile"].shape == (len(queries), len(ladder))
    for i, s in enumerate(TRUE):
        top = results[i][0]
        assert top["song_id"] == 2 * i + 2
        assert abs(top["speed"] * 65536 - T.q16(s)) <= st, (i, top["speed"], s)               # within one rung of the truth
        assert abs(top["offset"] - (5 + i) * SR / 2048) <= 1, (i, top["offset"])             # the cut, in the TABLE's frames
        assert top["offset_seconds"] == round(float(top["offset"]) / 44100 * 2048, 5)
        assert top["speed"] == float(ladder[int(tm["speed_best"][i])]) / 65536
        assert all(r["speed"] == top["speed"] for r in results[i])
    # the plain fused path loses the queries that are off speed and keeps the others: the feature, end to end
    plain, _ = S.recognize_batch(queries, db[0], topn=TOPN, fused=True)
    for i, s in enumerate(TRUE):
        hit = bool(plain[i]) and plain[i][0]["song_id"] == 2 * i + 2 and abs(plain[i][0]["offset"] - (5 + i) * SR / 2048) <= 1
        assert hit == (s == 1.0), (i, s, plain[i][:1])


def test_slices_of_queries_give_the_same(S, ctx, db, queries, ladder, expected):
    from shazam_amd import _ffi
    ctx.set_debug(_ffi.DEBUG_SPEED_SMALL_SLICES)       # 6 queries: 3 slices of 2, 42 matched queries each
    try:
        res = _raw(S, ctx, db[0], queries, ladder)
    finally:
        ctx.set_debug(0)
    _assert_equals_cpu(res, expected)
    whole = _raw(S, ctx, db[0], queries, ladder)
    for name in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "best", "profile"):
        assert np.array_equal(res[name], whole[name]), name


def test_single_query_single_rung_is_the_fused_call(S, ctx, db, queries):
    """A ladder of 65536 alone: the arrays of shz_recognize_batch."""
    res = _raw(S, ctx, db[0], queries, np.asarray([65536], np.uint32))
    plain, _ = S.recognize_batch(queries, db[0], topn=TOPN, fused=True)
    for q in range(len(queries)):
        assert int(res["nres"][q]) == len(plain[q])
        for n, r in enumerate(plain[q]):
            assert (int(res["sid"][q, n]), int(res["delta"][q, n]), int(res["dedup"][q, n]), int(res["nhash"][q])) == \
                (r["song_id"], r["offset"], r["hashes_matched_in_input"], r["input_total_hashes"])


def test_48k_queries_go_through_resample_to(S, db, songs, ladder):
    from shazam_amd.speed import DEFAULT_STEP_Q16 as st
    qs, truth = [], [(3, 6, 1.03), (8, 9, 1.0)]
    for c, second, s in truth:
        qs.append(T.speed_up(_cut(songs[c], second, s), 44100 / 48000))    # the same audio sampled at 48 kHz
    results, tm = S.recognize_speeds(qs, db[0], speeds=ladder, Fs=48000, topn=TOPN, resample_to=44100)
    for (c, second, s), r in zip(truth, results):
        assert r and r[0]["song_id"] == c + 1
        assert abs(r[0]["speed"] * 65536 - T.q16(s)) <= st
        assert abs(r[0]["offset"] - second * SR / 2048) <= 1
