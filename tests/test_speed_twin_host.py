"""CPU: the numpy twin of the speed warp (tests/speed_twin.py), speed_ladder, and the statement of what the feature is worth
-- on the reference's own pipeline (oracle/cpu_ref.py) a query played 2-4 % off speed is lost, and warping its peaks by the
true factor brings it back.  No GPU.

Measured with these inputs (one 40 s music_clip(7, 3) in the table, 10 s cut at second 10, sped up by linear interpolation):
aligned votes of the right song, plain path / peaks warped by the true factor: 0.96: 6 / 283, 1.02: 13 / 305, 1.04: 12 / 411
(1.00: 641 / 641); the warped answer is at offset 216 frames, the plain path's top offset is noise."""
import numpy as np
import pytest

import speed_twin as T
from oracle import cpu_ref as O, synth
from shazam_amd.speed import DEFAULT_STEP_Q16, speed_ladder

R = 44100


def _random_peaks(seed, frames=60, per_frame=5):
    rng = np.random.default_rng(seed)
    f, t = [], []
    for fr in range(frames):
        n = int(rng.integers(0, per_frame + 1))
        f.extend(sorted(rng.choice(2049, n, replace=False).tolist()))
        t.extend([fr] * n)
    return np.asarray(f, np.int64), np.asarray(t, np.int64)


@pytest.mark.parametrize("fan", [1, 2, 5, 64])
def test_twin_at_unity_is_pair_keys(fan):
    f, t = _random_peaks(1)
    k, t1 = T.warp_pair(f, t, T.S_ONE, fan)
    ok, ot1 = O.pair_keys(f, t, fan)
    assert np.array_equal(k, ok) and np.array_equal(t1, ot1)
    wf, wt = T.warp_peaks(f, t, T.S_ONE)
    assert np.array_equal(wf, f) and np.array_equal(wt, t)


@pytest.mark.parametrize("s16", [32768, 40000, 65535, 65536, 65537, 70000, 131072])
def test_warped_time_is_monotone_and_rounded(s16):
    f, t = _random_peaks(2)
    wf, wt = T.warp_peaks(f, t, s16)
    assert np.all(np.diff(wt) >= 0)
    same = np.diff(wt) == 0
    assert np.all(np.diff(wf)[same] >= 0)                 # inside a warped frame: by f'
    tt = np.arange(0, 5000, dtype=np.int64)
    wt_all = (tt * s16 + 32768) >> 16
    assert np.all(np.diff(wt_all) >= 0)
    assert np.array_equal(wt_all, np.floor(tt * (s16 / 65536) + 0.5).astype(np.int64))
    if s16 >= T.S_ONE:
        assert np.all(np.diff(wt_all) >= 1)               # no two frames merge
    else:
        assert np.bincount(wt_all).max() <= 2             # at most two neighbouring frames share a t'


def test_frames_merge_below_unity_and_interleave_by_frequency():
    s16 = 40000                                           # frames 1 and 2 (0.61 and 1.22) both round to t' = 1
    assert [(x * s16 + 32768) >> 16 for x in (0, 1, 2, 3)] == [0, 1, 1, 2]
    f = np.array([100, 300, 500, 200, 400, 600, 50], np.int64)
    t = np.array([1, 1, 1, 2, 2, 2, 3], np.int64)
    wf, wt = T.warp_peaks(f, t, s16)
    fp = (2 * 65536 * f + s16) // (2 * s16)
    assert wt.tolist() == [1] * 6 + [2]
    assert wf[:6].tolist() == sorted(fp[:6].tolist())     # the two frames interleave by f'
    assert wf[:6].tolist() != fp[:6].tolist()
    # equal f' in a merged frame: the earlier peak first -- the pairing sees (t', f', index) order
    f2, t2 = np.array([300, 300], np.int64), np.array([1, 2], np.int64)
    k, t1 = T.warp_pair(f2, t2, s16, 2)
    assert len(k) == 1 and (int(k[0]) & 0xFF) == 0 and int(t1[0]) == 1


def test_peaks_leave_above_the_last_bin():
    f, t = np.array([1500, 2048], np.int64), np.array([4, 4], np.int64)
    wf, wt = T.warp_peaks(f, t, 32768)
    assert wf.tolist() == [] and wt.tolist() == []        # 3000 and 4096
    wf, _ = T.warp_peaks(np.array([1024, 1025, 2048], np.int64), np.array([0, 0, 0], np.int64), 32768)
    assert wf.tolist() == [2048]                           # 2048 stays, 2050 and 4096 leave
    wf, _ = T.warp_peaks(f, t, 131072)
    assert wf.tolist() == [750, 1024]
    # round-half-up of f * 65536 / s16
    for s16 in (32768, 40000, 65535, 65537, 70000, 131072):
        ff = np.arange(0, 2049, dtype=np.int64)
        fp = (2 * 65536 * ff + s16) // (2 * s16)
        assert np.array_equal(fp, np.floor(ff * 65536 / s16 + 0.5).astype(np.int64))


def test_speed_ladder_properties():
    for args in ((), (0.95, 1.05, 0.0025), (1.01, 1.03), (0.9, 0.97, 0.001), (1.0, 1.0), (0.5, 2.0, 0.01)):
        lad = speed_ladder(*args)
        assert lad.dtype == np.uint32 and lad.ndim == 1
        assert 65536 in lad.tolist()
        assert np.all(np.diff(lad.astype(np.int64)) > 0)   # sorted, no duplicates
        assert lad.min() >= 32768 and lad.max() <= 131072
    lad = speed_ladder()
    assert np.all(np.diff(lad.astype(np.int64)) == DEFAULT_STEP_Q16)
    assert lad[0] >= np.ceil(0.95 * 65536) and lad[-1] <= np.floor(1.05 * 65536)
    assert lad[0] - DEFAULT_STEP_Q16 < 0.95 * 65536 and lad[-1] + DEFAULT_STEP_Q16 > 1.05 * 65536
    # the documented default: twice the measured half-width of 0.07 %, which the issue's figures bound below 0.25 %
    assert DEFAULT_STEP_Q16 == round(0.0014 * 65536) and DEFAULT_STEP_Q16 / 65536 / 2 < 0.0025
    inner = speed_ladder(1.01, 1.03)
    assert set(inner.tolist()) - {65536} <= set(lad.tolist())   # every ladder lies on the grid anchored at 65536
    with pytest.raises(ValueError):
        speed_ladder(0.4, 1.0)
    with pytest.raises(ValueError):
        speed_ladder(0.95, 1.05, 0.0)


@pytest.fixture(scope="module")
def song_table():
    song = synth.music_clip(7, 3, 40 * R)
    k, t1, _, _ = O.fingerprint_keys(song)
    return song, T.table_of([(k, t1)])


@pytest.mark.parametrize("s", [0.96, 1.02, 1.04])
def test_plain_path_loses_the_query_and_the_warp_finds_it(song_table, s):
    song, table = song_table
    q = T.speed_up(song[10 * R: 10 * R + int(10 * R * s) + 2], s)[:10 * R]
    qk, qt, qf, qpt = O.fingerprint_keys(q)
    plain, _, _ = T.aligned_votes(qk, qt, table, 1)
    warped, _, _ = T.aligned_votes(*T.warp_pair(qf, qpt, T.q16(s)), table, 1)
    cut = 10 * R / 2048                                     # 215.33 frames
    plain_right = [a for sid, d, a in plain if sid == 1]
    plain_count = plain_right[0] if plain_right else 0
    print(f"speed {s}: plain {plain}, warped {warped}")
    assert warped and warped[0][0] == 1 and abs(warped[0][1] - cut) <= 1
    assert warped[0][2] >= 5 * max(plain_count, 1)
    assert not (plain and plain[0][0] == 1 and abs(plain[0][1] - cut) <= 1)   # the plain path's top answer is not (song, offset)
