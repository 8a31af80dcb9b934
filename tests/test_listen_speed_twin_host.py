"""CPU: the numpy twin of the listeners' peak windows (tests/listen_speed_twin.py) -- its window cuts at the edges, its
hashes against warp_pair_batch / warp_pair_batch_tf on whole clips, its horizons against shz_stream_plan -- and the
end-to-end conditions of test_gpu_listener_speeds.py met by the twin alone, before any GPU is asked.  No GPU."""
import numpy as np
import pytest

import listen_speed_cases as CS
import listen_speed_twin as LT
import speed_twin as T
import warp_twin as W


def _random_peaks(seed, frames=150, per_frame=5):
    rng = np.random.default_rng(seed)
    f, t = [], []
    for fr in range(frames):
        n = int(rng.integers(0, per_frame + 1))
        f.extend(sorted(rng.choice(2049, n, replace=False).tolist()))
        t.extend([fr] * n)
    return np.asarray(f, np.int64), np.asarray(t, np.int64)


def test_ended_streams_from_frame_0_are_the_whole_clips():
    """w0 = 0 and every stream ended: the listener's query is the whole clips' peaks"""
    peaks = [_random_peaks(3), _random_peaks(4, frames=90)]
    horizons = [150, 90]                                    # ended: every frame settled; min - window_frames < 0
    w0, win = LT.window(peaks, horizons, 107)
    assert w0 == 0
    for (f, t), (wf, wt) in zip(peaks, win):
        assert np.array_equal(wf, f) and np.array_equal(wt, t)
    pf, pt = np.concatenate([p[0] for p in peaks]), np.concatenate([p[1] for p in peaks])
    po, qc = np.asarray([0, len(peaks[0][0]), len(pf)], np.uint64), np.asarray([0, 2], np.uint32)
    lad = [60000, 65536, 67500]
    k, t1, ho = T.warp_pair_batch(pf, pt, po, qc, lad)
    for v, (hk, ht) in enumerate(LT.hashes(win, w0, lad)):
        a, b = int(ho[2 * v]), int(ho[2 * v + 2])
        assert np.array_equal(hk, k[a:b]) and np.array_equal(ht, t1[a:b])
    tempos, pitches = [65536, 60000, 70000], [67500, 65536, 62000]
    k, t1, ho = W.warp_pair_batch_tf(pf, pt, po, qc, tempos, pitches)
    for v, (hk, ht) in enumerate(LT.hashes(win, w0, tempos, pitches)):
        a, b = int(ho[2 * v]), int(ho[2 * v + 2])
        assert np.array_equal(hk, k[a:b]) and np.array_equal(ht, t1[a:b])


def test_window_cuts_at_the_edges():
    f = np.asarray([10, 20, 30, 40, 50, 60], np.int64)
    t = np.asarray([0, 92, 93, 94, 199, 230], np.int64)
    # H <= window_frames: w0 = 0, everything below H stays
    w0, win = LT.window([(f, t)], [107], 107)
    assert w0 == 0 and win[0][1].tolist() == [0, 92, 93, 94]
    w0, win = LT.window([(f, t)], [50], 107)
    assert w0 == 0 and win[0][1].tolist() == [0]
    # H = 200: w0 = 93 -- the peak at t = w0 is kept, the one at w0 - 1 dropped, the one at H - 1 kept, the one beyond waits
    w0, win = LT.window([(f, t)], [200], 107)
    assert w0 == 93 and win[0][1].tolist() == [93, 94, 199] and win[0][0].tolist() == [30, 40, 50]
    # a channel ahead of H = min: it keeps its settled peaks >= H, the other channel's cut is its own horizon
    w0, win = LT.window([(f, t), (f, t)], [200, 240], 107)
    assert w0 == 93 and win[0][1].tolist() == [93, 94, 199] and win[1][1].tolist() == [93, 94, 199, 230]
    # rebased times start at 0: nothing is added to the query offsets
    (k, t1), = LT.hashes([win[1]], w0, [65536])
    ok, ot1 = T.warp_pair(win[1][0], win[1][1].astype(np.int64) - 93, 65536)
    assert np.array_equal(k, ok) and np.array_equal(t1, ot1) and int(t1.min()) == 0
    # a listener without peaks in its window: no hashes, no answer
    exp = LT.expected([(f[:0], t[:0])], 5, {}, [65536, 67000])
    assert exp["nres"] == 0 and exp["nhash"] == 0 and exp["best"] == 0 and exp["profile"].tolist() == [0, 0]


def test_horizon_is_the_stream_plan():
    from shazam_amd import _ffi
    for hop in (2048, 1024):
        for n in (0, 1, 4095, 4096, 4097, 6143, 6144, 24575, 24576, 24577, 26624, 100000, 617400):
            for ended in (False, True):
                if n == 0 and not ended:
                    continue
                assert LT.horizon(n, ended, hop) == _ffi.stream_plan(0, n, 0, hop, ended)[3], (hop, n, ended)
    # and the listener's window is shz_listener_window
    for hs in ([0, 0], [107, 300], [108, 300], [500, 400]):
        assert LT.window([(np.zeros(0), np.zeros(0))] * 2, hs, 107)[0] == _ffi.listener_window(hs, 107)[1]


@pytest.fixture(scope="module")
def corpus():
    sg = CS.songs()
    return sg, CS.oracle_table(sg)


def test_the_twin_alone_meets_the_end_to_end_conditions(corpus):
    """A 1.03 cut of songs[5] from second 3, one channel, 8192-sample chunks: from the first push with a full window on, the
    twin's top answer is the song, at a speed within one rung of 1.03, at an offset within 2 frames of 3 s + w0 * 1.03; at
    the ladder [65536] alone -- no warp -- the song is not reported."""
    sg, table = corpus
    lad = CS.ladder()
    x = CS.cut(sg[CS.FAST_SONG], CS.FAST_SECOND, CS.FAST)
    peaks = CS.oracle_peaks(x)
    pushes = CS.full_window_pushes(len(x))
    assert len(pushes) >= 20 and pushes[-1][1]
    worst = 0.0
    for got, ended, h in pushes:
        w0, win = LT.window([peaks], [h], CS.WINDOW_FRAMES)
        assert w0 == h - CS.WINDOW_FRAMES > 0
        exp = LT.expected(win, w0, table, lad, None, CS.TOPN)
        assert exp["nres"] > 0
        top = (int(exp["sid"][0]), int(exp["delta"][0]), int(lad[exp["best"]]))
        worst = max(worst, abs(top[1] - (CS.FAST_SECOND * CS.SR / 2048 + w0 * CS.FAST)))
        assert CS.end_to_end_ok(top, w0, lad), (got, w0, top, exp["profile"].tolist())
        one = LT.expected(win, w0, table, [65536], None, CS.TOPN)
        assert not (one["nres"] and int(one["sid"][0]) == CS.FAST_SONG + 1), (got, one["profile"].tolist())
    print("pushes asserted:", len(pushes), "| worst offset error (frames):", worst)
