"""CPU: the host half of altered content shared between recordings (shazam_amd/shared.py) and its definition
(tests/shared_warp_twin.py): the twin against shared_twin / repeat_twin where they must agree, the two-recording fixture on
the reference's peaks against the table of DESIGN.md 3.7r, cells_fit, the rung choice, the job plan, shared_occurrences on the
new dicts."""
from fractions import Fraction

import numpy as np
import pytest

import repeat_twin
import shared_twin
import shared_warp_cases as K
import shared_warp_twin as twin
from oracle import cpu_ref as O
from shazam_amd import extent, shared

S_ONE = 65536
T_MAX = K.T_MAX


@pytest.fixture(scope="module")
def fx():
    """the fixture on the reference's peaks: peaks, the twin's cells of the eight jobs of the table, their fold"""
    pf, pt, po = K.oracle_peaks(K.recordings())
    cells = K.twin_cells(pf, pt, po, K.table_jobs())
    return dict(pf=pf, pt=pt, po=po, cells=cells, reps=K.twin_fold(cells))


def _hashes(pf, pt, po):
    ks, ts, ho = [], [], [0]
    for c in range(len(po) - 1):
        k, t1 = O.pair_keys(pf[po[c]:po[c + 1]], pt[po[c]:po[c + 1]], 5)
        ks += [int(x) for x in k]
        ts += [int(x) for x in t1]
        ho.append(len(ks))
    return ks, ts, ho


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def test_twin_at_the_unit_warp_is_the_plain_join_on_the_reference_hashes(fx):
    ks, ts, ho = _hashes(fx["pf"], fx["pt"], fx["po"])
    want = shared_twin.cells(ks, ts, ho, [0, 1, 2], [(1, 0), (0, 1)], -300, 300, 64, 5, 8)
    got = K.twin_cells(fx["pf"], fx["pt"], fx["po"], [(1, 0, 0, -300, 300), (0, 1, 0, -300, 300)], [S_ONE], [S_ONE])
    for k in want:
        assert got[k] == want[k], k
    assert got["job_hashes"] == [want["rec_hashes"][1], want["rec_hashes"][0]]


def test_twin_windows_per_job_are_per_window_calls_of_the_plain_twin(fx):
    ks, ts, ho = _hashes(fx["pf"], fx["pt"], fx["po"])
    windows = [(-300, 300), (5, 5), (-40, 4), (6, T_MAX), (-T_MAX, -700)]                # (the last: beyond the recordings)
    got = K.twin_cells(fx["pf"], fx["pt"], fx["po"], [(1, 0, 0, lo, hi) for lo, hi in windows], [S_ONE], [S_ONE], min_cell_pairs=2)
    for j, (lo, hi) in enumerate(windows):
        want = shared_twin.cells(ks, ts, ho, [0, 1, 2], [(1, 0)], lo, hi, 64, 5, 2)
        a, b = got["cell_off"][j], got["cell_off"][j + 1]
        for k in twin.CELL_KEYS:
            assert got[k][a:b] == want[k], (k, j)
        for k in twin.JOB_KEYS:
            assert got[k][j] == want[k][0], (k, j)
    assert got["job_pairs"][1] > 1000 and got["job_pairs"][4] == 0


def test_twin_self_job_at_unity_gives_the_cells_of_the_repeat_twin():
    rng = np.random.default_rng(11)                                             # a pattern of 100 peaks, aired five times
    pt, pf = rng.integers(0, 60, 100), rng.integers(0, 400, 100)
    t = np.concatenate([pt + 83 * k for k in range(5)])
    f = np.concatenate([pf] * 5)
    order = np.lexsort((f, t))
    f, t = f[order], t[order]
    ks, ts, ho = _hashes(f, t, [0, 500])
    for lo, hi in ((1, T_MAX), (80, 170), (83, 83)):                           # (the airings lie 83 frames apart)
        want = repeat_twin.cells(ks, ts, ho, [0, 1], lo, hi, 8, 3, 1)
        got = twin.cells(f, t, [0, 500], [0, 1], [S_ONE], [S_ONE], [(0, 0, 0, lo, hi)], 8, 3, 1)
        assert len(want["lag"]) >= 10
        for k in twin.CELL_KEYS:                                                 # (the skip counters are defined differently)
            assert got[k] == want[k], (k, lo, hi)


# ---- the fixture on the reference's peaks: the table of DESIGN.md 3.7r --------------------------------------------------------
def test_fixture_reproduces_the_table(fx):
    assert fx["po"] == [0, 2227, 4399]
    assert fx["cells"]["rec_hashes"] == [8898, 8678]
    assert fx["cells"]["job_pairs"][3:5] == [107, 149]                          # the speed rungs 1 % off: nothing left to fold
    by_job = {}
    for r in fx["reps"]:
        by_job.setdefault(r["rec"], []).append((r["lag"], r["lag_lo"], r["lag_hi"], r["first"], r["last"], r["pairs"], r["cells"]))
    assert by_job == {
        0: [(5, 5, 5, 274, 403, 1755, 5)],                                       # plain: Y alone
        1: [(20, 20, 21, 43, 214, 415, 10)],                                     # (1.03, 1.03): X
        2: [(-35, -35, -34, 464, 634, 526, 12)],                                 # (1.04, 0.97): Z
        5: [(-2, -4, 8, 433, 592, 518, 18)],                                     # (0.97, 0.97): Z, the lag drifting
        6: [(-29, -30, -28, 459, 628, 518, 12)],                                 # (1.03, 0.97): Z
        7: [(-9, -11, -6, 285, 419, 1706, 9)],                                   # (1.04, 1.00): Y, the lag drifting
    }
    assert extent.own_frames(43, 214, K.T16[1]) == (42, 208)


def test_fixture_tempo_fit(fx):
    want = {0: 1.0, 1: 1.03, 2: 1.04, 5: 1.04, 6: 1.04, 7: 1.0}
    for r in fx["reps"]:
        slope, _ = shared.cells_fit(K.stretch_cells(fx["cells"], r))
        fit = float(extent.tempo_of(K.T16[r["rec"]], slope))
        print(r["rec"], K.WARPS[r["rec"]], fit, abs(fit - want[r["rec"]]))
        assert abs(fit - want[r["rec"]]) <= 0.003, (r["rec"], fit)


# ---- cells_fit on built cells -------------------------------------------------------------------------------------------------
def test_cells_fit():
    # an exact line: lag = 7 + mid / 4, mids 12, 44, 76 at any weights
    cells = [(7 + m // 4, m - 4, m + 4, w) for m, w in ((12, 3), (44, 50), (76, 9))]
    assert shared.cells_fit(cells) == (Fraction(1, 4), Fraction(7))
    # the weights count: two cells at one mid pull the line to the heavier one
    slope, c = shared.cells_fit([(0, 0, 0, 1), (10, 10, 10, 1), (30, 10, 10, 3)])
    assert slope == Fraction(25, 10) and c == 0
    # a half-frame mid (first + last odd) is exact too
    assert shared.cells_fit([(1, 0, 1, 5), (2, 1, 2, 5)]) == (Fraction(1), Fraction(1, 2))
    # one cell, no cell, equal mids: no line
    assert shared.cells_fit([(5, 10, 20, 100)]) is None
    assert shared.cells_fit([]) is None
    assert shared.cells_fit([(5, 10, 20, 100), (6, 12, 18, 50), (7, 15, 15, 1)]) is None
    # tempo_of: slope 0.04 at the unit rung is tempo 1.04
    assert extent.tempo_of(S_ONE, Fraction(1, 25)) == Fraction(26, 25)


# ---- the rung choice ----------------------------------------------------------------------------------------------------------
def _st(warp, pairs, lag_lo=0, lag_hi=0, a=(100, 199), b=(300, 399), t16=S_ONE, f16=S_ONE, job=0):
    return dict(job=job, warp=warp, t16=t16, f16=f16, pairs=pairs, lag_lo=lag_lo, lag_hi=lag_hi, a_first=a[0], a_last=a[1],
                b_first=b[0], b_last=b[1])


def test_rung_choice_tie_rules():
    pick = lambda *s: [(x["warp"], x["candidates"]) for x in shared.choose_rungs(list(s))]   # noqa: E731
    # most pairs
    assert pick(_st(0, 500), _st(1, 501), _st(2, 499)) == [(1, [(0, 500, 0, 0), (2, 499, 0, 0)])]
    # ... then the narrower lag range
    assert pick(_st(0, 500, -3, 4), _st(1, 500, 10, 12)) == [(1, [(0, 500, -3, 4)])]
    # ... then the warp nearer (65536, 65536), the two distances added
    assert pick(_st(0, 500, t16=S_ONE + 300, f16=S_ONE), _st(1, 500, t16=S_ONE - 100, f16=S_ONE + 199)) == [(1, [(0, 500, 0, 0)])]
    # ... then the lower index
    assert pick(_st(3, 500, t16=S_ONE + 7), _st(2, 500, t16=S_ONE - 7)) == [(2, [(3, 500, 0, 0)])]


def test_rung_choice_joins_only_what_overlaps_in_a_and_in_b():
    # overlap of exactly half of the shorter interval in a and in b: one stretch; one frame less in b: two
    one = shared.choose_rungs([_st(0, 10, a=(100, 199), b=(300, 399)), _st(1, 20, a=(150, 189), b=(380, 419))])
    assert [s["warp"] for s in one] == [1]
    two = shared.choose_rungs([_st(0, 10, a=(100, 199), b=(300, 399)), _st(1, 20, a=(150, 189), b=(381, 420))])
    assert [s["warp"] for s in two] == [0, 1] and all(s["candidates"] == [] for s in two)
    # the same frames of a against two places of b (an advert that b airs twice): not merged
    two = shared.choose_rungs([_st(0, 10, b=(300, 399)), _st(1, 20, b=(900, 999))])
    assert len(two) == 2
    # two stretches of ONE warp are two stretches, and so are those of different jobs
    assert len(shared.choose_rungs([_st(1, 10), _st(1, 20)])) == 2
    assert len(shared.choose_rungs([_st(0, 10, job=0), _st(1, 20, job=1)])) == 2
    # a chain: 0 ~ 1 and 1 ~ 2 make one stretch of the three
    got = shared.choose_rungs([_st(0, 10, a=(100, 199)), _st(1, 30, a=(150, 249), b=(350, 449)), _st(2, 20, a=(200, 299), b=(400, 499))])
    assert [(s["warp"], len(s["candidates"])) for s in got] == [(1, 2)]


def test_rung_choice_on_the_fixture(fx):
    """Y is kept plain (1,755 pairs against 1,706), Z at (1.04, 0.97) (526 against 518 and 518), X has one rung"""
    st = []
    for r in fx["reps"]:
        v = r["rec"]
        sc = K.stretch_cells(fx["cells"], r)
        a_first, a_last = extent.own_frames(r["first"], r["last"], K.T16[v])
        st.append(_st(v, r["pairs"], r["lag_lo"], r["lag_hi"], (a_first, a_last),
                      (min(f + g for g, f, _, _ in sc), max(l + g for g, _, l, _ in sc)), K.T16[v], K.F16[v]))
    got = {s["warp"]: s["candidates"] for s in shared.choose_rungs(st)}
    assert got == {0: [(7, 1706, -11, -6)], 1: [], 2: [(5, 518, -4, 8), (6, 518, -30, -28)]}


# ---- the job list and its calls -------------------------------------------------------------------------------------------------
def test_warp_table_and_jobs():
    assert shared._warp_table(None, None, None, None) is None
    t16, f16 = shared._warp_table([67502], None, None, None)
    assert t16.tolist() == [67502, S_ONE] and f16.tolist() == [67502, S_ONE]     # the unit rung is appended ...
    t16, f16 = shared._warp_table(None, [S_ONE, 68157], [63570, S_ONE], None)
    assert list(zip(t16.tolist(), f16.tolist())) == [(S_ONE, 63570), (S_ONE, S_ONE), (68157, 63570), (68157, S_ONE)]   # ... not twice
    t16, _ = shared._warp_table(True, None, None, None)
    from shazam_amd.speed import speed_ladder
    assert t16.tolist() == speed_ladder().tolist()
    with pytest.raises(TypeError):
        shared._warp_table([1.03], None, None, None)                             # Q16 integers, as everywhere
    jobs = shared._warp_jobs([(1, 0), (2, 2)], [67502, S_ONE], [67502, S_ONE], -900, 700, 22)
    assert jobs == [(1, 0, 0, -900, 700, 0), (1, 0, 1, -900, 700, 0), (2, 2, 0, 22, 700, 1), (2, 2, 0, -900, -22, 1)]
    # a window that leaves one side of a self pair only
    assert shared._warp_jobs([(2, 2)], [67502], [67502], 5, 700, 22) == [(2, 2, 0, 22, 700, 0)]
    with pytest.raises(ValueError):
        shared._check_warp_pairs([(0, 3)], 3)
    assert shared._check_warp_pairs([(2, 2)], 3) == [(2, 2)]


def test_plan_warp_calls_respects_the_three_limits(monkeypatch):
    jobs = [(a, b, v, 0, 0, p) for p, (a, b) in enumerate([(0, 1), (2, 3), (4, 4)]) for v in range(5)]
    assert shared._plan_warp_calls(jobs) == [(0, 15, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4])]
    monkeypatch.setattr(shared, "MAX_JOBS", 4)
    assert [(c[0], c[1]) for c in shared._plan_warp_calls(jobs)] == [(0, 4), (4, 8), (8, 12), (12, 15)]
    monkeypatch.setattr(shared, "MAX_JOBS", 4096)
    monkeypatch.setattr(shared, "MAX_WARPS", 2)
    calls = shared._plan_warp_calls(jobs)
    assert all(len(c[3]) <= 2 for c in calls) and [c[0] for c in calls] == list(range(0, 15, 2))
    monkeypatch.setattr(shared, "MAX_WARPS", 1024)
    monkeypatch.setattr(shared, "MAX_RECS", 6)                                   # recordings named + distinct (a, warp)
    calls = shared._plan_warp_calls(jobs)
    assert [(c[0], c[1]) for c in calls] == [(0, 4), (4, 6), (6, 10), (10, 15)]
    for j0, j1, recs, warps in calls:
        assert len(recs) + len({(a, v) for a, _, v, *_ in jobs[j0:j1]}) <= 6
    assert sum(c[1] - c[0] for c in calls) == len(jobs)


# ---- shared_occurrences on the new dicts ----------------------------------------------------------------------------------------
def test_shared_occurrences_reads_own_frames_and_b_intervals():
    # first / last are warped frames (tempo 2: twice a's own) and lag is taken at one cell; the intervals are the dict's own
    new = dict(rec_a=0, rec_b=1, first=200, last=398, lag=50, a_first=100, a_last=199, b_first=260, b_last=440)
    old = dict(rec_a=2, rec_b=0, first=500, last=560, lag=-390)                  # airs in 0 at [110, 170]: inside a's own frames
    got = shared.shared_occurrences([new, old])
    assert len(got) == 1 and got[0]["airings"] == [(0, 100, 199), (1, 260, 440), (2, 500, 560)] and got[0]["shared"] == [0, 1]
    # read as warped frames the same stretch would lie at [200, 398] of recording 0 and join nothing
    plain = {k: new[k] for k in ("rec_a", "rec_b", "first", "last", "lag")}
    assert len(shared.shared_occurrences([plain, old])) == 2
    # the twin's occurrences on the intervals the new dict names
    as_plain = dict(rec_a=0, rec_b=1, first=100, last=199, lag=160)              # b at [260, 359]: its hull differs, the groups not
    want = shared_twin.occurrences([as_plain, old])
    assert [g["shared"] for g in got] == [w[1] for w in want]
