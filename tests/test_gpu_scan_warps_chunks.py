"""GPU: scan_windows over more pairs than one library call takes (1,024).  A grid of 600 tempos x 5 pitches goes in calls of whole
tempo rows, merged by the best-variant rule: it must equal the same pairs sent through Context.scan_warps in chunks cut
elsewhere and merged here with the twin's rule.  The separable search's stage 2 over 600 tempos x the pitch rungs stage 1 chose
goes in several selected calls, each window's list cut at the chunk borders and rebased: every count it reports must be the
grid's count of that pair, every window must have tried stage 1's pitches and the tempos at its own best pitch, and its answer
must be the best of those by the pair rule."""
import numpy as np
import pytest

import scan_warp_cases as SC
import warp_twin as WT

pytestmark = pytest.mark.gpu

TEMPOS = np.unique(np.append(52429 + 44 * np.arange(599), 65536)).astype(np.uint32)   # 0.8 .. 1.2 and 65536: 600 values
STEP_SECONDS = 2


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def db(S):
    d, _ = SC.make_db(S, S.get_context(0), SC.songs())
    yield d
    d.close()


@pytest.fixture(scope="module")
def part():
    return SC.recording()[6 * SC.SR:16 * SC.SR]            # the end of the tempo-only piece and most of the mixed one


@pytest.fixture(scope="module")
def grid(S, db, part):
    assert len(TEMPOS) == 600
    return S.scan_windows([part], db, tempos=TEMPOS, pitches=SC.PITCHES, step_seconds=STEP_SECONDS)


def test_a_grid_above_one_call_equals_other_chunks_merged_by_the_twin(S, db, part, grid):
    from shazam_amd.speed import warp_chunks, warp_grid
    t16, f16 = warp_grid(TEMPOS, SC.PITCHES)
    assert len(t16) == 3000 and len(warp_chunks(3000, 5)) == 3 and np.array_equal(grid["warps"][0], t16)
    _, pcm, off, first = SC.flatten(S, [part])
    parts = [db.ctx.scan_warps(db.table, pcm, off, first, SC.WINDOW, SC.FIX_STEP, t16[a:a + 751], f16[a:a + 751])[0] for a in range(0, 3000, 751)]
    profile = np.concatenate([p["profile"] for p in parts], axis=1)
    assert profile.shape == (len(grid["best"]), 3000) and len(grid["best"]) >= 3 and np.array_equal(grid["profile"], profile)
    for w in range(len(grid["best"])):
        v = WT.best_variant_tf(profile[w], t16.tolist(), f16.tolist())
        assert int(grid["best"][w]) == v, w
        for k in SC.ARRAYS:
            assert np.array_equal(grid[k][w], parts[v // 751][k][w]), (w, k)
    assert grid["work"] == tuple(sum(p["work"][i] for p in parts) for i in range(2))
    assert profile.max() >= SC.MIN_ALIGNED                 # the pieces are found, so the merge had something to choose


def test_a_separable_stage_two_above_one_call(S, db, part, grid):
    sep = S.scan_windows([part], db, tempos=TEMPOS, pitches=SC.PITCHES, step_seconds=STEP_SECONDS, search="separable")
    t16, f16 = (a.tolist() for a in sep["warps"])
    n_p = len(SC.PITCHES)
    assert len(t16) - n_p > 1024 and (len(t16) - n_p) % 600 == 0           # stage 2: several calls
    column = {pair: i for i, pair in enumerate(zip(*(a.tolist() for a in grid["warps"])))}
    hits = 0
    for w in range(len(sep["best"])):
        s1 = sep["profile"][w, :n_p]
        b1 = WT.best_variant_tf(s1, [65536] * n_p, SC.PITCHES.tolist())
        want = list(range(n_p))
        if s1[b1] >= 1:
            want += [j for j in range(n_p, len(t16)) if f16[j] == int(SC.PITCHES[b1]) and t16[j] != 65536]
            assert len(want) == n_p + 599
        assert np.flatnonzero(sep["tried"][w]).tolist() == want, w
        assert not sep["profile"][w][~sep["tried"][w]].any()
        for j in want:
            assert int(sep["profile"][w, j]) == int(grid["profile"][w, column[(t16[j], f16[j])]]), (w, j)
        j = want[WT.best_variant_tf(sep["profile"][w, want], [t16[i] for i in want], [f16[i] for i in want])]
        assert int(sep["best"][w]) == j, w
        assert int(sep["aligned"][w, 0] if sep["nres"][w] else 0) == int(sep["profile"][w, j]), w
        g = int(grid["best"][w])
        if (t16[j], f16[j]) == (int(grid["warps"][0][g]), int(grid["warps"][1][g])):
            hits += 1
            for k in SC.ARRAYS:
                assert np.array_equal(sep[k][w], grid[k][w]), (w, k)
    assert hits >= 2
