"""GPU: scan(..., tempos=, pitches=) end to end on the fixture of tests/scan_warp_cases.py -- three table songs rendered at
(1.16, 1), (1.10, 0.97) and (1, 0.97) between noise, windows 2 s apart: the grid returns the three segments with their pairs,
the separable search returns the same songs, positions and pairs on every window for far less work, speeds= together with tempos= is refused, and the speed
scan and the plain scan return on this recording what they return through their own library calls."""
import numpy as np
import pytest

import scan_warp_cases as SC
import speed_twin as T

pytestmark = pytest.mark.gpu

STEP, SR = SC.FIX_STEP, SC.SR
STEP_SECONDS = 2                  # seconds_to_frames(2, 44100) == SC.FIX_STEP


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


@pytest.fixture(scope="module")
def recording():
    return SC.recording()


@pytest.fixture(scope="module")
def db(S, ctx):
    d, _ = SC.make_db(S, ctx, SC.songs())
    yield d
    d.close()


@pytest.fixture(scope="module")
def ladders(S):
    from shazam_amd.speed import pitch_ladder, tempo_ladder
    tl, pl = tempo_ladder(0.8, 1.2), pitch_ladder()
    assert np.array_equal(tl, SC.TEMPOS) and set(SC.PITCHES.tolist()) <= set(pl.tolist()) and len(pl) == 83
    return tl, pl


def _check_segments(segs):
    assert len(segs) == 1 and len(segs[0]) == 3, segs
    for seg, (sid, first, last, pair), (_, tempo, pitch, _s) in zip(segs[0], SC.SEGMENTS, SC.PIECES):
        assert seg["song_id"] == sid and seg["song_name"] == f"song{sid - 1}".encode()
        assert (round(seg["tempo"] * 65536), round(seg["pitch"] * 65536)) == pair
        assert abs(seg["tempo"] * 65536 - T.q16(tempo)) <= SC.TEMPO_RUNG and abs(seg["pitch"] * 65536 - T.q16(pitch)) <= SC.PITCH_RUNG
        assert "speed" not in seg and "shift" not in seg
    return segs[0]


def test_the_grid_returns_the_three_segments(S, db, recording, ladders):
    tl, pl = ladders
    segs = S.scan([recording], db, tempos=tl, pitches=pl, min_aligned=SC.MIN_ALIGNED, step_seconds=STEP_SECONDS)
    print(segs[0])
    for seg, (sid, first, last, pair) in zip(_check_segments(segs), SC.SEGMENTS):
        assert (seg["first_window"], seg["last_window"], seg["windows"]) == (first, last, last - first + 1)
        assert (seg["pos_first"], seg["pos_last"]) == (SC.DELTA[first], SC.DELTA[last])
        assert seg["hashes_aligned"] == max(SC.ALIGNED[first:last + 1])
        assert seg["offset_seconds"] == round(seg["pos_first"] / SR * 2048, 5)
        assert seg["tempo_fit"] == (seg["pos_last"] - seg["pos_first"]) / ((last - first) * STEP)
        assert abs(seg["tempo_fit"] - pair[0] / 65536) < 0.02
    assert segs[0][0]["start_seconds"] == 0.0 and segs[0][2]["end_seconds"] == round(537 * 2048 / SR, 5)
    # the raw arrays: the pair list, the chosen factors and the work per window
    w = S.scan_windows([recording], db, tempos=tl, pitches=pl, step_seconds=STEP_SECONDS)
    t16, f16 = w["warps"]
    assert w["step_frames"] == STEP and w["profile"].shape == (11, 9 * 83) and len(t16) == len(f16) == 9 * 83 and len(w["ms"]) == 4 and w["tried"].all()
    assert np.array_equal(w["tempo"], t16[w["best"]] / 65536.0) and np.array_equal(w["pitch"], f16[w["best"]] / 65536.0)
    assert [(int(t16[b]), int(f16[b])) for b in w["best"]] == [SC.SEGMENTS[0][3]] * 5 + [SC.SEGMENTS[1][3]] * 2 + [SC.SEGMENTS[2][3]] * 4
    assert w["delta"][:, 0].tolist() == SC.DELTA and w["aligned"][:, 0].tolist() == SC.ALIGNED and w["sid"][:, 0].tolist() == SC.SID
    assert w["work"] == SC.WORK_GRID
    # an explicit pair list, and no recordings
    three = S.scan([recording], db, warps=([76548, 71042, 65536], [65536, 63561, 63561]), min_aligned=SC.MIN_ALIGNED,
                   tempo_tol=0, pitch_tol=0, step_seconds=STEP_SECONDS)
    assert [(s["song_id"], s["first_window"], s["last_window"]) for s in three[0]] == [s[:3] for s in SC.SEGMENTS]
    assert S.scan([], db, tempos=tl, pitches=pl) == []


def test_the_separable_search_returns_the_grids_segments_for_less_work(S, db, recording, ladders):
    tl, pl = ladders
    grid = S.scan_windows([recording], db, tempos=tl, pitches=pl, step_seconds=STEP_SECONDS)
    sep = S.scan_windows([recording], db, tempos=tl, pitches=pl, search="separable", step_seconds=STEP_SECONDS)
    print("work: grid", grid["work"], "separable", sep["work"], sep["stage1"]["work"], sep["stage2"]["work"])
    assert sep["work"][1] < grid["work"][1] and sep["work"][0] < grid["work"][0]
    assert sep["work"] == tuple(a + b for a, b in zip(sep["stage1"]["work"], sep["stage2"]["work"]))
    assert grid["work"] == SC.WORK_GRID and sep["work"] == SC.WORK_SEPARABLE        # the counts DESIGN.md 3.7i states
    # every window: the grid's song, position (+-1 frame), pair and count
    g_pair = list(zip(grid["warps"][0][grid["best"]].tolist(), grid["warps"][1][grid["best"]].tolist()))
    s_pair = list(zip(sep["warps"][0][sep["best"]].tolist(), sep["warps"][1][sep["best"]].tolist()))
    assert len(grid["best"]) == len(sep["best"]) == 11
    for w in range(11):
        assert int(sep["sid"][w, 0]) == int(grid["sid"][w, 0]) and s_pair[w] == g_pair[w], w
        assert abs(int(sep["delta"][w, 0]) - int(grid["delta"][w, 0])) <= 1, w
        assert int(sep["aligned"][w, 0]) == int(grid["aligned"][w, 0]), w
    # a window tried the 83 pitches and 8 tempos beside its own: 91 variants instead of 747
    assert (sep["tried"].sum(axis=1) == 83 + 8).all() and sep["profile"].shape == sep["tried"].shape
    # every segment: the grid's song, windows, pair and positions (+-1 frame)
    kw = dict(tempos=tl, pitches=pl, min_aligned=SC.MIN_ALIGNED, step_seconds=STEP_SECONDS)
    g_segs = S.scan([recording], db, **kw)[0]
    s_segs = _check_segments(S.scan([recording], db, search="separable", **kw))
    assert len(g_segs) == len(s_segs) == 3
    for g, s_ in zip(g_segs, s_segs):
        assert all(s_[k] == g[k] for k in ("song_id", "first_window", "last_window", "windows", "tempo", "pitch", "hashes_aligned"))
        assert abs(s_["pos_first"] - g["pos_first"]) <= 1 and abs(s_["pos_last"] - g["pos_last"]) <= 1


def test_speeds_together_with_warps_is_refused(S, db, recording, ladders):
    tl, pl = ladders
    for kw in (dict(tempos=tl), dict(pitches=pl), dict(warps=(tl, tl)), dict(search="separable")):
        with pytest.raises(ValueError):
            S.scan([recording], db, speeds=True, **kw)
        with pytest.raises(ValueError):
            S.scan_windows([recording], db, speeds=tl, **kw)
    with pytest.raises(TypeError):
        S.scan([recording], db, tempos=tl, warps=(tl, tl))
    with pytest.raises(TypeError):
        S.scan([recording], db, warps=(tl, tl), search="separable")
    with pytest.raises(ValueError):
        S.scan([recording], db, tempos=tl, search="coarse")


def test_the_speed_scan_and_the_plain_scan_are_untouched(S, ctx, db, recording):
    """scan(speeds=) and the plain scan on this recording: the timelines of their own library calls' arrays."""
    from shazam_amd import _ffi
    from shazam_amd.speed import speed_ladder
    _, pcm, off, first = SC.flatten(S, [recording])
    ladder = speed_ladder(0.97, 1.03)
    raw, wo, _ = ctx.scan_speeds(db.table, pcm, off, first, SC.WINDOW, STEP, ladder)
    want = _ffi.scan_timeline_speeds(wo, raw["sid"], raw["delta"], raw["aligned"], raw["nres"], raw["best"], STEP, ladder, 40, 1, 1, 2)
    segs = S.scan([recording], db, speeds=ladder, min_aligned=40, step_seconds=STEP_SECONDS)[0]
    assert len(segs) == len(want["rec"]) > 0
    for i, s in enumerate(segs):
        assert (s["song_id"], s["first_window"], s["last_window"], s["pos_first"], s["pos_last"], s["windows"]) == tuple(
            int(want[k][i]) for k in ("sid", "first", "last", "pos_first", "pos_last", "hits"))
        assert s["speed"] == float(ladder[int(want["rung"][i])]) / 65536.0 and "tempo" not in s
    w = S.scan_windows([recording], db, speeds=ladder, step_seconds=STEP_SECONDS)
    SC.same(w, raw, "speed scan")
    assert "warps" not in w and "work" not in w
    raw, wo, _ = ctx.scan_batch(db.table, pcm, off, first, SC.WINDOW, STEP)
    want = _ffi.scan_timeline(wo, raw["sid"], raw["delta"], raw["aligned"], raw["nres"], STEP, 40, 1)
    segs = S.scan([recording], db, min_aligned=40, step_seconds=STEP_SECONDS)[0]
    assert len(segs) == len(want["rec"]) > 0
    for i, s in enumerate(segs):
        assert (s["song_id"], s["shift"], s["windows"]) == (int(want["sid"][i]), int(want["shift"][i]), int(want["hits"][i]))
    w = S.scan_windows([recording], db, step_seconds=STEP_SECONDS)
    SC.same(w, raw, "plain scan", SC.ARRAYS)
    assert "best" not in w and np.where(w["nres"] > 0, w["aligned"][:, 0], 0).tolist() == SC.PLAIN
    assert S.scan([recording], db, min_aligned=SC.MIN_ALIGNED, step_seconds=STEP_SECONDS) == [[]]
