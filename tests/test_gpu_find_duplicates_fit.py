"""GPU: find_duplicates(..., tempos=, extents="fit"), end to end from audio: where an altered copy overlaps its original, in
both songs' own frames, and the tempo it really runs at.

The catalogue is the note corpus of tests/test_gpu_warp_recognize.py, whose tempo and pitch are rendered separately: songs 1 ..
3 are its three 30 s songs; song 4 (WHOLE) is the whole of song 1 rendered at tempo 1.04; song 5 (PART) is 10 s of song 2 from
its second 8 rendered at tempo 0.95 (that module's _render: in song 2's own time the stretch runs from second 8 to second
17.5, frames 172.27 .. 376.83); song 6 is an unrelated 10 s rendering.  The search has three tempo rungs, 65536 + 2753 k for
k in -1 .. 1, as tests/test_gpu_warp_recognize_extents.py: 1.04 lies 0.2 % beside its rung 68289 and 0.95 lies 0.8 % beside
its rung 62783.

Checked beforehand on the CPU (oracle/cpu_ref.py's hashes of the same six sample arrays, tests/rows_warp_twin.py's search,
catalog.fold_pairs_warps, tests/rows_fit_twin.py as the table of catalog.pair_extents_warps), vote tolerance 0:
  * (1, 4): song 4's rows at 68289 align 1,919 rows at delta 0; (2, 5): song 5's rows at 62783 align 459 at delta -172; both
    "b" sides; no other pair aligns more than 15 rows at any rung -- the defaults of the warped search (100 rows, 0.03) part them;
  * the table's largest offset is 643, the ladder's largest rung 68289: t_max = 670, gap 2753, drift_bins = ceil(670 x 2753 /
    131072) = 15.  From the PAIRS' rungs alone (62783 and 68289 are not neighbours: gap 5506) it is 29;
  * at 15: (1, 4) count 3,449, a 0 .. 642, b 0 .. 617, tempo_fit 1.04008 (rung 1.04201, true 1.04);
           (2, 5) count 900, a 172 .. 376, b 0 .. 213, tempo_fit 0.95049 (rung 0.95799, true 0.95): the fit misses by 0.0005
           where the rung misses by 0.0080, a factor of 16 -- asserted below, as the rung misses by more than 0.5 %;
  * at 29 six chance pairs enter the range of (2, 5): a 160 .. 376 -- 12 frames before the stretch -- and tempo_fit 0.95424.
    That is why find_duplicates derives drift_bins from the ladder's rungs and not from the pairs'.
A stretch is widened by 10 frames each side before the spans are compared with it: a peak is a maximum over 21 frames
(get_2D_peaks' neighbourhood), so a cut moves peaks up to 10 frames inside it -- a property of the algorithm."""
import numpy as np
import pytest

import warp_twin as W
from rows_fit_twin import TwinTable
from test_gpu_warp_recognize import CUT_S, N_SONGS, SONG_S, SR, S, _render, ctx, songs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

T_STEP = 2753
TEMPOS = np.asarray([65536 + T_STEP * k for k in (-1, 0, 1)], np.uint32)
WHOLE, PART, OTHER = 4, 5, 6
WHOLE_TEMPO, PART_TEMPO, PART_S = 1.04, 0.95, 10
PART_LO, PART_HI = CUT_S * SR / 2048, (CUT_S + PART_S * PART_TEMPO) * SR / 2048          # in song 2's own frames
MARGIN = 10


@pytest.fixture(scope="module")
def catalogue(S, ctx, songs):
    assert N_SONGS == 3
    clips = list(songs) + [W.notes_clip(7, 0, SONG_S / WHOLE_TEMPO, WHOLE_TEMPO, 1.0), _render(1, PART_TEMPO, 1.0, PART_S),
                           W.notes_clip(7, 9, 10)]
    k, t1, ho = S.fingerprint_batch(clips, ctx=ctx)
    db = S.get_database("hip")(ctx=ctx)
    for c in range(len(clips)):
        kk, tt = k[ho[c]:ho[c + 1]], t1[ho[c]:ho[c + 1]]
        sid = db.insert_song(f"clip{c}", f"{c:040X}", len(set(zip(kk.tolist(), tt.tolist()))))
        assert sid == c + 1
        db.insert_keys(sid, kk, tt)
        db.set_song_fingerprinted(sid)
    db.finalize()
    assert ctx.vote_tolerance == 0
    yield db, [ctx.frames_of(len(x)) for x in clips]
    db.close()


@pytest.fixture(scope="module")
def runs(S, catalogue):
    db, _ = catalogue
    plain = db.find_duplicates(tempos=TEMPOS)
    fit = db.find_duplicates(tempos=TEMPOS, extents="fit", timings=True)
    return plain, fit


def _drift(max_off, rungs, tol=0):
    """the formula, written out: ceil(t_max x half the largest gap / 65536), clamped"""
    rungs = sorted(set(int(r) for r in rungs))
    gap = max(b - a for a, b in zip(rungs, rungs[1:]))
    t_max = (int(max_off) * rungs[-1] + 32768) >> 16
    return max(0, min(-(-t_max * gap // 131072), 2047 - tol))


def test_both_copies_are_found_and_the_old_columns_are_unchanged(S, runs):
    plain, fit = runs
    assert plain["pairs"].dtype == np.dtype(list(S.catalog.WARP_PAIR_FIELDS))
    assert fit["pairs"].dtype == np.dtype(list(S.catalog.WARP_EXTENT_PAIR_FIELDS))
    for x in fit["pairs"]:
        print("pair", {f: x[f] for f in fit["pairs"].dtype.names})
    assert [(int(x["a"]), int(x["b"])) for x in fit["pairs"]] == [(1, WHOLE), (2, PART)]
    assert fit["pairs"]["warped"].tolist() == ["b", "b"] and fit["pairs"]["tempo_q16"].tolist() == [int(TEMPOS[2]), int(TEMPOS[0])]
    for f, _ in S.catalog.WARP_PAIR_FIELDS:
        assert np.array_equal(fit["pairs"][f], plain["pairs"][f]), f
    assert fit["clusters"] == plain["clusters"]
    assert len(fit["ms"]) == 4 and "ms" not in plain and fit["ms"][3] > 0


def test_the_new_columns_are_the_twins_on_the_exported_table(S, catalogue, runs):
    db, _ = catalogue
    plain, fit = runs
    tk, ts, to = db.table.export()
    drift = _drift(to.max(), TEMPOS)
    assert fit["pairs"]["drift_bins"].tolist() == [drift, drift] and drift == S.catalog.warp_drift_bins(int(to.max()), TEMPOS, 0)
    twin = TwinTable(tk, ts, to)
    want = S.catalog.pair_extents_warps(twin, plain["pairs"], tol=0, drift_bins=drift)
    assert len(twin.calls) == 1 and twin.calls[0]["job_sid"] == [WHOLE, PART]
    for f in fit["pairs"].dtype.names:
        assert np.array_equal(fit["pairs"][f], want[f]), (f, fit["pairs"][f], want[f])
    assert not np.isnan(fit["pairs"]["tempo_fit"]).any() and (fit["pairs"]["count"] >= fit["pairs"]["aligned"]).all()
    one = S.find_duplicates(db, tempos=TEMPOS, extents="fit", batch_rows=1)
    assert np.array_equal(one["pairs"], fit["pairs"]) and one["clusters"] == fit["clusters"]
    # an explicit drift_bins is taken as given; pair_extents_warps on its own knows the pairs' rungs only
    given = S.find_duplicates(db, tempos=TEMPOS, extents="fit", drift_bins=3)
    assert given["pairs"]["drift_bins"].tolist() == [3, 3]
    assert np.array_equal(given["pairs"], S.catalog.pair_extents_warps(twin, plain["pairs"], tol=0, drift_bins=3))
    alone = S.catalog.pair_extents_warps(db.table, plain["pairs"])
    wide = _drift(to.max(), plain["pairs"]["tempo_q16"])
    assert alone["drift_bins"].tolist() == [wide, wide] and wide > drift
    assert np.array_equal(alone, S.catalog.pair_extents_warps(twin, plain["pairs"], tol=0, drift_bins=wide))


def test_the_spans_lie_where_the_copies_were_cut_and_the_fit_beats_a_rung_that_misses(catalogue, runs):
    _, frames = catalogue
    whole, part = runs[1]["pairs"]
    # the excerpt: song 2 is the longer track; its span lies inside the true stretch widened by the peak neighbourhood
    assert PART_LO - MARGIN <= int(part["a_first"]) <= int(part["a_last"]) <= PART_HI + MARGIN
    assert int(part["b_first"]) <= MARGIN and int(part["b_last"]) >= frames[PART - 1] - 1 - MARGIN
    # the whole-song copy: both spans cover their track to within the margin at both ends
    assert int(whole["a_first"]) <= MARGIN and int(whole["a_last"]) >= frames[0] - 1 - MARGIN
    assert int(whole["b_first"]) <= MARGIN and int(whole["b_last"]) >= frames[WHOLE - 1] - 1 - MARGIN
    for x, true in ((whole, WHOLE_TEMPO), (part, PART_TEMPO)):
        rung = int(x["tempo_q16"]) / 65536
        print(f"pair ({x['a']}, {x['b']}): tempo_fit {x['tempo_fit']:.5f}  rung {rung:.5f}  true {true}  "
              f"|fit - true| {abs(x['tempo_fit'] - true):.5f}  |rung - true| {abs(rung - true):.5f}")
    rung = int(part["tempo_q16"]) / 65536
    assert abs(rung - PART_TEMPO) >= 0.005 * PART_TEMPO                    # the rung misses by 0.5 % or more: the fit must beat it
    assert abs(part["tempo_fit"] - PART_TEMPO) < abs(rung - PART_TEMPO)


def test_refusals(S, catalogue):
    db, _ = catalogue
    with pytest.raises(ValueError):
        db.find_duplicates(extents="fit")                                   # no ladder
    with pytest.raises(ValueError):
        db.find_duplicates(extents=True, tempos=TEMPOS)                     # extents=True keeps refusing a ladder
    with pytest.raises(ValueError):
        db.find_duplicates(extents="span", tempos=TEMPOS)
    sharded = S.get_database("hip")(ctx=db.ctx, shards=2)
    with pytest.raises(NotImplementedError):
        sharded.find_duplicates(tempos=TEMPOS, extents="fit")
    with pytest.raises(NotImplementedError):
        S.find_duplicates(sharded, tempos=TEMPOS, extents="fit")
    sharded.close()
