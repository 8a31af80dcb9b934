"""CPU: the two ladders, the grid and its chunks, the merge of chunked results, and the numpy twin of the two-factor warp
(tests/warp_twin.py): on the diagonal it is speed_twin's, at (65536, 65536) it is the oracle's pair_keys, and in the two
quadrants the speed ladder never reaches the order rule (t', f', index) does what DESIGN.md 3.7e says.  The note corpus
is stable: the score of a clip does not depend on its length or tempo.  No GPU."""
import numpy as np
import pytest

import speed_twin as T
import warp_twin as W
from oracle import cpu_ref as O
from shazam_amd import speed as SP


def _random_peaks(seed, frames=60, per_frame=5):
    rng = np.random.default_rng(seed)
    f, t = [], []
    for fr in range(frames):
        n = int(rng.integers(0, per_frame + 1))
        f.extend(sorted(rng.choice(2049, n, replace=False).tolist()))
        t.extend([fr] * n)
    return np.asarray(f, np.int64), np.asarray(t, np.int64)


@pytest.mark.parametrize("name", ["tempo_ladder", "pitch_ladder"])
def test_ladder_properties(name):
    ladder = getattr(SP, name)
    default = {"tempo_ladder": SP.DEFAULT_TEMPO_STEP_Q16, "pitch_ladder": SP.DEFAULT_PITCH_STEP_Q16}[name]
    for args in ((), (0.95, 1.05, 0.0025), (1.01, 1.03), (0.9, 0.97, 0.001), (1.0, 1.0), (0.5, 2.0, 0.01)):
        lad = ladder(*args)
        assert lad.dtype == np.uint32 and lad.ndim == 1
        assert 65536 in lad.tolist()
        assert np.all(np.diff(lad.astype(np.int64)) > 0)   # sorted, no duplicates
        assert lad.min() >= 32768 and lad.max() <= 131072
    lad = ladder()
    assert np.all(np.diff(lad.astype(np.int64)) == default)
    assert lad[0] >= np.ceil(0.95 * 65536) and lad[-1] <= np.floor(1.05 * 65536)
    assert lad[0] - default < 0.95 * 65536 and lad[-1] + default > 1.05 * 65536
    assert np.array_equal(ladder(0.95, 1.05, 92 / 65536), SP.speed_ladder())   # one construction for the three ladders
    with pytest.raises(ValueError, match=name):
        ladder(0.4, 1.0)
    with pytest.raises(ValueError, match=name):
        ladder(1.0, 2.5)
    with pytest.raises(ValueError):
        ladder(0.95, 1.05, 0.0)


def test_default_steps_are_the_measured_ones():
    """twice the half-widths 0.06 % (pitch) and 2.1 % (tempo, 10 s queries).  The tempo axis is the tolerant
    one by more than an order of magnitude, so a +-5 % x +-5 % grid has far fewer tempo rungs than pitch rungs."""
    assert SP.DEFAULT_PITCH_STEP_Q16 == round(0.0012 * 65536) and SP.DEFAULT_TEMPO_STEP_Q16 == round(0.042 * 65536)
    assert SP.DEFAULT_TEMPO_STEP_Q16 > 10 * SP.DEFAULT_PITCH_STEP_Q16
    assert len(SP.tempo_ladder()) * 10 < len(SP.pitch_ladder())


def test_grid_is_the_tempo_major_product():
    t16, f16 = SP.warp_grid([60000, 65536, 70000], [65000, 65536])
    assert t16.dtype == np.uint32 and f16.dtype == np.uint32
    assert t16.tolist() == [60000, 60000, 65536, 65536, 70000, 70000]
    assert f16.tolist() == [65000, 65536, 65000, 65536, 65000, 65536]
    t16, f16 = SP.warp_grid(SP.tempo_ladder(step=0.01), SP.pitch_ladder(step=92 / 65536))
    assert len(t16) == 11 * 71 == len(f16)                              # 1 % tempo steps x the speed ladder's pitch steps
    with pytest.raises(TypeError, match="Q16"):
        SP.warp_grid([1.0, 1.02], [65536])
    with pytest.raises(TypeError, match="Q16"):
        SP.warp_grid([65536], [0.97])


def test_chunks_are_whole_rows_of_at_most_1024_pairs():
    assert SP.warp_chunks(803, 73) == [(0, 803)]
    assert SP.warp_chunks(1024, 1) == [(0, 1024)]
    assert SP.warp_chunks(1025, 1) == [(0, 1024), (1024, 1025)]
    ch = SP.warp_chunks(11 * 101, 101)                                  # 1,111 pairs: 10 rows, then 1
    assert ch == [(0, 1010), (1010, 1111)]
    ch = SP.warp_chunks(21 * 400, 400)                                  # two rows a call
    assert ch[0] == (0, 800) and ch[-1] == (8000, 8400) and len(ch) == 11
    for a, b in ch:
        assert a % 400 == 0 and b % 400 == 0 and 0 < b - a <= 1024
    assert [a for a, _ in ch[1:]] == [b for _, b in ch[:-1]]
    assert SP.warp_chunks(0, 5) == []
    with pytest.raises(ValueError, match="does not fit one call"):
        SP.warp_chunks(3 * 1025, 1025)
    with pytest.raises(ValueError, match="whole number of rows"):
        SP.warp_chunks(10, 3)


def _part(best, profile, tag):
    nq = len(best)
    return {"best": np.asarray(best, np.uint32), "profile": np.asarray(profile, np.uint32),
            "sid": np.full((nq, 2), tag, np.uint32), "delta": np.full((nq, 2), tag, np.int32),
            "aligned": np.full((nq, 2), tag, np.uint32), "dedup": np.full((nq, 2), tag, np.uint32),
            "nres": np.full(nq, tag, np.uint32), "nhash": np.full(nq, tag, np.uint32)}


def test_merge_of_chunks_follows_the_best_variant_rule():
    t16 = np.asarray([65536, 66000, 65000, 65536], np.uint32)
    f16 = np.asarray([65000, 65536, 65536, 65600], np.uint32)          # distances 536, 464, 536, 64
    # query 0: the greater count wins; query 1: a tie goes to the smaller distance (pair 3); query 2: a tie in count and
    # distance (pairs 0 and 2) goes to the lower index; query 3: nothing anywhere -- the pair nearest the identity
    a = _part([1, 1, 0, 1], [[3, 9], [2, 7], [5, 1], [0, 0]], 1)
    b = _part([0, 1, 0, 1], [[4, 2], [1, 7], [5, 4], [0, 0]], 2)
    m = SP.merge_warp_chunks([a, b], t16, f16)
    assert m["best"].tolist() == [1, 3, 0, 3]
    assert m["nres"].tolist() == [1, 2, 1, 2] and m["sid"][:, 0].tolist() == [1, 2, 1, 2]
    assert m["profile"].tolist() == [[3, 9, 4, 2], [2, 7, 1, 7], [5, 1, 5, 4], [0, 0, 0, 0]]
    for q in range(4):
        assert int(m["best"][q]) == W.best_variant_tf(m["profile"][q], t16, f16)
    assert SP.merge_warp_chunks([a], t16[:2], f16[:2]) is a


@pytest.mark.parametrize("fan", [1, 2, 5, 64])
def test_twin_on_the_diagonal_is_the_speed_twin(fan):
    f, t = _random_peaks(3)
    g, u = _random_peaks(4, frames=30)
    pf, pt = np.concatenate([f, g, f[:0]]), np.concatenate([t, u, t[:0]])
    po = np.asarray([0, len(f), len(f) + len(g), len(f) + len(g)], np.uint64)
    speeds = [32768, 40000, 65535, 65536, 65537, 70000, 131072]
    for qc in ([0, 1, 2, 3], [0, 2, 3], [0, 0, 3]):
        k, t1, ho = W.warp_pair_batch_tf(pf, pt, po, qc, speeds, speeds, fan)
        ek, et, eho = T.warp_pair_batch(pf, pt, po, qc, speeds, fan)
        assert np.array_equal(k, ek) and np.array_equal(t1, et) and np.array_equal(ho, eho)
    for s16 in speeds:
        for x, y in zip(W.warp_peaks_tf(f, t, s16, s16), T.warp_peaks(f, t, s16)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("fan", [1, 2, 5, 64])
def test_twin_at_the_identity_is_pair_keys(fan):
    f, t = _random_peaks(1)
    k, t1 = W.warp_pair_tf(f, t, 65536, 65536, fan)
    ok, ot1 = O.pair_keys(f, t, fan)
    assert np.array_equal(k, ok) and np.array_equal(t1, ot1)
    wf, wt = W.warp_peaks_tf(f, t, 65536, 65536)
    assert np.array_equal(wf, f) and np.array_equal(wt, t)


def test_each_axis_takes_its_own_factor():
    f, t = _random_peaks(5)
    wf, wt = W.warp_peaks_tf(f, t, 70000, 65536)                        # tempo alone: no frame merges, the order is the input's
    assert np.array_equal(wf, f) and np.array_equal(wt, (t * 70000 + 32768) >> 16)
    wf, wt = W.warp_peaks_tf(f, t, 65536, 70000)                        # pitch alone: the frames are the input's
    keep = (2 * 65536 * f + 70000) // (2 * 70000) <= 2048
    assert np.array_equal(wt, t[keep]) and np.array_equal(wf, ((2 * 65536 * f + 70000) // 140000)[keep])
    wf, wt = W.warp_peaks_tf(f, t, 65536, 60000)                        # bins spread, the upper ones leave, the order stays
    keep = (2 * 65536 * f + 60000) // 120000 <= 2048
    assert 0 < keep.sum() < len(f) and np.array_equal(wt, t[keep])


def test_ties_across_two_merged_frames_keep_the_earlier_index():
    """t16 < 65536 with f16 > 65536, the quadrant no speed reaches: frames 1 and 2 share t' = 1 and bins 2k - 1, 2k share
    f' = k at 131072, so the two frames tie on f'; the earlier index (the earlier frame) comes first."""
    assert [(x * 40000 + 32768) >> 16 for x in (0, 1, 2, 3)] == [0, 1, 1, 2]
    assert [(2 * 65536 * b + 131072) // (2 * 131072) for b in (100, 101, 102, 103)] == [50, 51, 51, 52]
    f = np.asarray([101, 103, 102, 200], np.int64)
    t = np.asarray([1, 1, 2, 2], np.int64)
    wf, wt = W.warp_peaks_tf(f, t, 40000, 131072)
    assert wt.tolist() == [1, 1, 1, 1] and wf.tolist() == [51, 51, 52, 100]      # 101 (frame 1) before 102 (frame 2)
    k, t1 = W.warp_pair_tf(f, t, 40000, 131072, 2)
    assert [int(x) >> 20 for x in k] == [51, 51, 52] and [(int(x) >> 8) & 0xFFF for x in k] == [51, 52, 100]
    # the same peaks with the tie the other way round in bin order: 102 in frame 1, 101 in frame 2 -- still frame 1 first
    wf2, _ = W.warp_peaks_tf(np.asarray([102, 101], np.int64), np.asarray([1, 2], np.int64), 40000, 131072)
    assert wf2.tolist() == [51, 51]
    # t16 >= 65536 with f16 < 65536: nothing merges, bins spread, the order is the input's without the peaks that leave
    wf, wt = W.warp_peaks_tf(np.asarray([1024, 1025, 5], np.int64), np.asarray([1, 1, 2], np.int64), 131072, 32768)
    assert wf.tolist() == [2048, 10] and wt.tolist() == [2, 4]


def test_the_score_of_a_note_clip_does_not_depend_on_length_or_call():
    a = W.notes_clip(7, 1, 3.0)
    b = W.notes_clip(7, 1, 1.5)
    assert a.dtype == np.int16 and len(a) == 3 * 44100
    assert np.array_equal(a[:len(b)], b)
    assert np.array_equal(W.notes_clip(7, 1, 1.5), b)
    assert not np.array_equal(W.notes_clip(7, 2, 1.5), b) and not np.array_equal(W.notes_clip(8, 1, 1.5), b)
    # a faster tempo moves the note boundaries and nothing else: the first note of voice 1 (32768 samples) ends sooner
    c = W.notes_clip(7, 1, 1.5, tempo=1.25)
    assert len(c) == len(b) and not np.array_equal(c, b)
    assert np.abs(a.astype(np.int64)).max() > 1000                      # notes, not only the bed
