"""GPU: recognize_warps -- the peaks of every query extracted once, warped for every (tempo, pitch) pair of a list, all
variants in one match -- equals the CPU pipeline exactly: oracle.cpu_ref.fingerprint_keys on every channel, the numpy twin
of the two-factor warp (tests/warp_twin.py) per pair, the reference's vote per variant, the same best-variant rule.

3 songs x 30 s of the note corpus (warp_twin.notes_clip(7, c, 30)) in the table; 10 s queries cut at second 8 of a song
rendered at the query's own tempo and pitch -- (1, 1), (1.04, 1), (0.95, 1), (1, 1.03), (1.03, 0.97) --, a silent query and
a two-channel one.  The grid: tempo rungs 65536 + 655 k, k in -5 .. 5, x pitch rungs 65536 + 92 k within 4 rungs of a true
pitch or of 65536: 11 x 27 = 297 pairs.

Figures of the CPU pipeline on these inputs are printed by the tests (run with -s)."""
import numpy as np
import pytest

import speed_twin as T
import warp_twin as W

pytestmark = pytest.mark.gpu

SR = 44100
N_SONGS, SONG_S, QUERY_S, CUT_S = 3, 30, 10, 8
TRUE = [(1.0, 1.0), (1.04, 1.0), (0.95, 1.0), (1.0, 1.03), (1.03, 0.97)]
SONG = [0, 2, 0, 1, 1]                                                      # the song query i is cut from
SILENT, STEREO = 5, 6                                                       # query 6: (1.04, 1) of song 2 and a noisy copy
TOPN = 2
T_STEP, F_STEP = 655, 92
CUT = CUT_S * SR / 2048                                                     # 172.27 frames


def _render(song, tempo, pitch, seconds=QUERY_S):
    """`seconds` of song `song` from its second 8, heard at (tempo, pitch): rendered, not made by the code under test"""
    x = W.notes_clip(7, song, CUT_S / tempo + seconds + 0.1, tempo, pitch)
    s0 = int(round(CUT_S / tempo * SR))
    return x[s0:s0 + int(seconds * SR)]


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def songs():
    return [W.notes_clip(7, c, SONG_S) for c in range(N_SONGS)]


@pytest.fixture(scope="module")
def ladders():
    tl = np.asarray([65536 + T_STEP * k for k in range(-5, 6)], np.uint32)
    ks = set()
    for p in sorted({p for _, p in TRUE}):
        mid = int(round((W.q16(p) - 65536) / F_STEP))
        ks |= set(range(mid - 4, mid + 5))
    pl = np.asarray([65536 + F_STEP * k for k in sorted(ks)], np.uint32)
    assert len(tl) == 11 and len(pl) == 27 and 65536 in pl.tolist()
    return tl, pl


@pytest.fixture(scope="module")
def grid(S, ladders):
    return S.warp_grid(*ladders)


@pytest.fixture(scope="module")
def queries():
    from oracle import synth
    qs = [_render(SONG[i], a, p) for i, (a, p) in enumerate(TRUE)]
    qs.append(np.zeros(QUERY_S * SR, np.int16))
    x = _render(2, 1.04, 1.0)
    qs.append([x, synth.mix_query(x, synth.synth_clip(5, 9, len(x), 0, 8000), 10.0)])
    for q in qs[:5]:
        q.setflags(write=False)
    return qs


@pytest.fixture(scope="module")
def db(S, ctx, songs):
    """Songs 1..3; returns (db, key32 -> [(sid, offset)]): one set of rows for the device table and for the CPU vote."""
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
def peaks(queries):
    """The oracle's peaks of every channel of every query, once"""
    from oracle import cpu_ref as O
    return [[O.fingerprint_keys(c)[2:] for c in ([q] if isinstance(q, np.ndarray) else q)] for q in queries]


def _cpu(peaks, table, t16, f16):
    """The CPU pipeline over a pair list: per query and pair the twin's hashes of every channel and the vote"""
    nq, K = len(peaks), len(t16)
    exp = {"sid": np.zeros((nq, K, TOPN), np.uint32), "delta": np.zeros((nq, K, TOPN), np.int32),
           "aligned": np.zeros((nq, K, TOPN), np.uint32), "dedup": np.zeros((nq, K, TOPN), np.uint32),
           "nres": np.zeros((nq, K), np.uint32), "nhash": np.zeros((nq, K), np.uint32)}
    for q, chans in enumerate(peaks):
        for v, (a, b) in enumerate(zip(t16.tolist(), f16.tolist())):
            hk = [W.warp_pair_tf(f, t, a, b) for f, t in chans]
            ranked, dedup, nhash = T.aligned_votes(np.concatenate([k for k, _ in hk]), np.concatenate([t for _, t in hk]), table, TOPN)
            exp["nres"][q, v], exp["nhash"][q, v] = len(ranked), nhash
            for n, (sid, delta, aligned) in enumerate(ranked):
                exp["sid"][q, v, n], exp["delta"][q, v, n], exp["aligned"][q, v, n] = sid, delta, aligned
                exp["dedup"][q, v, n] = dedup[sid]
    exp["profile"] = np.where(exp["nres"] > 0, exp["aligned"][:, :, 0], 0).astype(np.uint32)
    exp["best"] = np.asarray([W.best_variant_tf(exp["profile"][q], t16, f16) for q in range(nq)], np.uint32)
    return exp


@pytest.fixture(scope="module")
def expected(peaks, db, grid):
    return _cpu(peaks, db[1], *grid)


def _raw(S, ctx, db, queries, t16, f16):
    chans, first = [], [0]
    for q in queries:
        cs = [q] if isinstance(q, np.ndarray) else list(q)
        chans.extend(S._as_pcm(c) for c in cs)
        first.append(len(chans))
    off = np.zeros(len(chans) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chans])
    res, _ = ctx.recognize_warps(db.table, np.concatenate(chans), off, np.asarray(first, np.uint32), t16, f16, topn=TOPN)
    return res


def _assert_equals_cpu(res, exp):
    nq = len(exp["best"])
    print("best (gpu, cpu):", res["best"].tolist(), exp["best"].tolist())
    assert np.array_equal(res["profile"], exp["profile"])
    assert np.array_equal(res["best"], exp["best"])
    for q in range(nq):
        b = int(exp["best"][q])
        n = int(exp["nres"][q, b])
        assert int(res["nres"][q]) == n and int(res["nhash"][q]) == int(exp["nhash"][q, b])
        for name in ("sid", "delta", "aligned", "dedup"):
            assert np.array_equal(res[name][q, :n], exp[name][q, b, :n]), (name, q)


def test_equals_the_cpu_pipeline(S, ctx, db, queries, grid, expected):
    _assert_equals_cpu(_raw(S, ctx, db[0], queries, *grid), expected)


def _right(ranked, sid):
    """rank 0 is song sid within 2 frames of the cut"""
    return bool(ranked) and ranked[0][0] == sid and abs(ranked[0][1] - CUT) <= 2


def test_the_feature_end_to_end(S, db, queries, ladders, grid, peaks):
    """recognize_warps names the right song, the chosen rungs are within one rung of the truth on each axis, OFFSET within 2
    frames of the cut.  Preconditions, asserted on the CPU twin and not on the code under test: every off-unity query's
    count warped by its true pair is at least twice its unwarped count, and the unwarped (1.03, 0.97) query does not give
    the right song at rank 0 (CPU figures: unwarped rank 0 is song 1 with 15 votes, the right song 2 is absent from the
    top two; warped by the true pair: song 2 at offset 173 with 324)."""
    d, table = db
    tl, pl = ladders
    for i, (a, p) in enumerate(TRUE):
        sid = SONG[i] + 1
        (f, t), = peaks[i]
        plain, _, _ = T.aligned_votes(*W.warp_pair_tf(f, t, 65536, 65536), table, TOPN)
        warped, _, _ = T.aligned_votes(*W.warp_pair_tf(f, t, W.q16(a), W.q16(p)), table, TOPN)
        print(f"true ({a}, {p}): unwarped {plain}, warped by the true pair {warped}")
        assert _right(warped, sid)
        if (a, p) != (1.0, 1.0):
            plain_n = max([n for s, _, n in plain if s == sid], default=0)
            assert warped[0][2] >= 2 * plain_n, (a, p)
        if (a, p) == (1.03, 0.97):
            assert not (plain and plain[0][0] == sid)
    results, tm = S.recognize_warps(queries, d, tempos=tl, pitches=pl, topn=TOPN)
    assert tm["warp_profile"].shape == (len(queries), len(grid[0]))
    assert np.array_equal(tm["warps"][0], grid[0]) and np.array_equal(tm["warps"][1], grid[1])
    truth = [(SONG[i] + 1, a, p) for i, (a, p) in enumerate(TRUE)] + [None, (3, 1.04, 1.0)]
    for i, tr in enumerate(truth):
        if tr is None:
            assert results[i] == []
            continue
        sid, a, p = tr
        top = results[i][0]
        print(i, tr, top["song_id"], top["offset"], top["tempo"], top["pitch"])
        assert top["song_id"] == sid
        assert abs(top["tempo"] * 65536 - W.q16(a)) <= T_STEP, (i, top["tempo"], a)
        assert abs(top["pitch"] * 65536 - W.q16(p)) <= F_STEP, (i, top["pitch"], p)
        assert abs(top["offset"] - CUT) <= 2, (i, top["offset"])
        assert top["offset_seconds"] == round(float(top["offset"]) / 44100 * 2048, 5)
        b = int(tm["warp_best"][i])
        assert (top["tempo"], top["pitch"]) == (float(grid[0][b]) / 65536, float(grid[1][b]) / 65536)
        assert all((r["tempo"], r["pitch"]) == (top["tempo"], top["pitch"]) for r in results[i])


def test_slices_of_queries_give_the_same(S, ctx, db, queries, grid, expected):
    from shazam_amd import _ffi
    ctx.set_debug(_ffi.DEBUG_SPEED_SMALL_SLICES)       # 7 queries: 4 slices of at most 2
    try:
        res = _raw(S, ctx, db[0], queries, *grid)
    finally:
        ctx.set_debug(0)
    _assert_equals_cpu(res, expected)


def test_a_diagonal_list_is_recognize_speeds(S, ctx, db, queries):
    lad = np.asarray([62259, 65536 - 92, 65536, 65536 + 92, 68157, 68813], np.uint32)
    res = _raw(S, ctx, db[0], queries, lad, lad)
    chans, first = [], [0]
    for q in queries:
        cs = [q] if isinstance(q, np.ndarray) else list(q)
        chans.extend(cs)
        first.append(len(chans))
    off = np.zeros(len(chans) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chans])
    sp, _ = ctx.recognize_speeds(db[0].table, np.concatenate(chans), off, np.asarray(first, np.uint32), lad, topn=TOPN)
    for name in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "best", "profile"):
        assert np.array_equal(res[name], sp[name]), name
    assert int(res["best"][0]) == 2 and int(res["nres"][0]) >= 1
    # the single pair (65536, 65536) on one query: the fused call's answer
    one = _raw(S, ctx, db[0], queries[:1], [65536], [65536])
    plain, _ = S.recognize_batch(queries[:1], db[0], topn=TOPN, fused=True)
    assert int(one["nres"][0]) == len(plain[0]) >= 1
    for n, r in enumerate(plain[0]):
        assert (int(one["sid"][0, n]), int(one["delta"][0, n]), int(one["dedup"][0, n]), int(one["nhash"][0])) == \
            (r["song_id"], r["offset"], r["hashes_matched_in_input"], r["input_total_hashes"])


def _separable_cpu(exp, tl, pl, q):
    """The separable search on the grid's own CPU results (65536 is a tempo rung, so both stages are rows and columns of the
    grid): stage 1 the pitch ladder at tempo 65536, stage 2 the tempo ladder at the best pitch rung.  Returns the grid index."""
    i0, P = tl.tolist().index(65536), len(pl)
    row = np.arange(i0 * P, (i0 + 1) * P)
    j = W.best_variant_tf(exp["profile"][q, row], np.full(P, 65536), pl)
    col = np.arange(len(tl)) * P + j
    return int(col[W.best_variant_tf(exp["profile"][q, col], tl, np.full(len(tl), pl[j]))])


def test_separable_search_finds_what_the_grid_finds(S, db, queries, ladders, grid, expected):
    tl, pl = ladders
    keep = []
    for q in range(5):
        g, s = int(expected["best"][q]), _separable_cpu(expected, tl, pl, q)
        same = (expected["sid"][q, g, 0], expected["delta"][q, g, 0], g) == (expected["sid"][q, s, 0], expected["delta"][q, s, 0], s)
        print(f"query {q} {TRUE[q]}: cpu grid pair {g}, cpu separable pair {s}")
        if same:
            keep.append(q)          # (a query is left out only where the CPU pipeline's two searches disagree)
    assert len(keep) >= 4
    gr, gtm = S.recognize_warps(queries, db[0], tempos=tl, pitches=pl, topn=TOPN, search="grid")
    sr, stm = S.recognize_warps(queries, db[0], tempos=tl, pitches=pl, topn=TOPN, search="separable")
    assert stm["warp_profile"].shape == (len(queries), len(tl)) and stm["stage1"]["warp_profile"].shape == (len(queries), len(pl))
    for q in keep:
        a, b = gr[q][0], sr[q][0]
        assert (a["song_id"], a["offset"], a["tempo"], a["pitch"]) == (b["song_id"], b["offset"], b["tempo"], b["pitch"]), q
        g = int(expected["best"][q])
        assert (b["tempo"], b["pitch"]) == (float(grid[0][g]) / 65536, float(grid[1][g]) / 65536)
        # the profile is that of the pairs matched: the grid's column at the chosen pitch
        col = np.arange(len(tl)) * len(pl) + g % len(pl)
        assert np.array_equal(stm["warp_profile"][q], expected["profile"][q, col])
        assert np.array_equal(stm["warps"][1][q], np.full(len(tl), grid[1][g]))
    assert sr[SILENT] == [] and sr[STEREO][0]["song_id"] == 3


def test_a_grid_above_1024_pairs_goes_in_chunks(S, ctx, db, queries):
    """11 tempo rungs x 101 pitch rungs = 1,111 pairs: chunks of 10 rows and 1 row, merged by the best-variant rule, equal
    the same pairs passed to the library in two explicit calls and merged here."""
    tl = np.asarray([65536 + T_STEP * k for k in range(-5, 6)], np.uint32)
    pl = np.asarray([65536 + 46 * k for k in range(-50, 51)], np.uint32)
    t16, f16 = S.warp_grid(tl, pl)
    qs = [queries[4], queries[SILENT], queries[3]]
    results, tm = S.recognize_warps(qs, db[0], tempos=tl, pitches=pl, topn=TOPN)
    a = _raw(S, ctx, db[0], qs, t16[:1010], f16[:1010])
    b = _raw(S, ctx, db[0], qs, t16[1010:], f16[1010:])
    profile = np.concatenate([a["profile"], b["profile"]], axis=1)
    assert np.array_equal(tm["warp_profile"], profile) and profile.shape == (3, 1111)
    for q in range(3):
        g = W.best_variant_tf(profile[q], t16, f16)
        assert int(tm["warp_best"][q]) == g
        part, v = (a, g) if g < 1010 else (b, g - 1010)
        assert int(part["best"][q]) == v
        assert len(results[q]) == int(part["nres"][q])
        assert int(tm["n_hashes"][q]) == int(part["nhash"][q])
        for n, r in enumerate(results[q]):
            assert (r["song_id"], r["offset"], r["hashes_matched_in_input"]) == \
                (int(part["sid"][q, n]), int(part["delta"][q, n]), int(part["dedup"][q, n]))
            assert (r["tempo"], r["pitch"]) == (float(t16[g]) / 65536, float(f16[g]) / 65536)
    assert results[0][0]["song_id"] == 2 and results[1] == [] and results[2][0]["song_id"] == 2
    # an explicit pair list above 1,024 goes in chunks of 1,024 pairs and gives the same
    r2, tm2 = S.recognize_warps(qs, db[0], warps=(t16, f16), topn=TOPN)
    assert np.array_equal(tm2["warp_profile"], profile) and np.array_equal(tm2["warp_best"], tm["warp_best"])
    assert r2 == results
