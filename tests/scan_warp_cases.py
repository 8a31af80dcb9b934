"""Test helpers for the scan over warp pairs (not a conftest, not collected): the fixture the GPU tests share -- four note songs
in the table, a recording of three pieces whose tempo and pitch were moved by the renderer, between noise -- the numbers the
CPU oracle and the twins measured on it, and the host recipe on device peaks."""
import numpy as np

import scan_warp_twin as SW
import speed_twin as T
import warp_twin as WT

ARRAYS = SW.ARRAYS
WINDOW, STEP = 108, 22            # round(5 s * 44100 / 2048), round(1 s * 44100 / 2048)
FIX_STEP = 43                     # the fixture's windows are 2 s apart: round(2 s * 44100 / 2048)
SR = 44100
TEMPO_RUNG, PITCH_RUNG = 2753, 79                        # the default steps of the two ladders, Q16
TEMPOS = np.asarray([54524, 57277, 60030, 62783, 65536, 68289, 71042, 73795, 76548], np.uint32)   # tempo_ladder(0.8, 1.2)
PITCHES = np.asarray([63561, 63640, 65536, 67432, 67511], np.uint32)       # the rungs of pitch_ladder() beside 0.97, 1, 1.03
# The pieces: (song index, tempo, pitch, seconds), each from the song's start, rendered by warp_twin.notes_clip's own
# arguments: a tempo-only piece, a mixed piece and a pitch-only piece.  Where the choices come from (CPU: the oracle's peaks, the
# twins' warp and cut, the reference's vote):
# - The tempo-only piece runs at 1.16, not at 1.04: the PLAIN scan still reaches 158 aligned hashes on a 5 s window of a piece
#   at tempo 1.04 -- a 108-frame window drifts by 4 frames only -- which is as much as a pitch-only piece collects, so no
#   threshold separates the populations.  The plain scan keeps a floor of 50 .. 85 on that song at any tempo, so the piece sits
#   where the floor is reached and a rung of the ladder (76548 = 1.168) lies within one rung of it.
# - That floor hardly depends on how much of the piece a window holds (18 of 108 frames still give 69), while the piece's count
#   at its own pair falls with its share.  Stage 1 of the separable search -- tempo 1 -- therefore names the tempo-only piece's
#   pitch on every window that holds a little of it, and the grid names it only while its share is large: with windows 1 s
#   apart some window always holds 1 .. 22 frames of it, and the two searches differ there.  So the windows are 2 s apart and
#   the piece is 7.95 s long: it ends at frame 214, one frame before window 5 begins, and window 4 holds 42 frames of it, where
#   both searches name it with a margin (grid 184 against 134, stage 1 75 against 55 on the CPU's own table).
# - The mixed piece follows it, at (1.10, 0.97): on the windows they share, both are weak at tempo 1 and strong at their own
#   pairs, so the two stages rank them alike.  The pitch-only piece comes last and has the mixed piece's pitch: on the windows
#   those two share stage 1 names one pitch rung whichever wins, and stage 2 then tries every tempo at it.
# - The trailing noise is 1.05 s, which keeps the recording at 25 s (537 frames).
PIECES = ((0, 1.16, 1.0, 7.95), (3, 1.10, 0.97, 7), (2, 1.0, 0.97, 7))
# Over warp_grid(TEMPOS, PITCHES), 45 pairs, window 108 / step 43 (11 windows of 537 frames), the votes of the CPU reference
# (speed_twin.aligned_votes) on the oracle's peaks of the recording against the table's rows: per window the best pair's
# index, the song, the song frame at the window's start and the aligned count
BEST = [42] * 5 + [30] * 2 + [20] * 4                    # (76548, 65536), (71042, 63561), (65536, 63561)
SID = [1] * 5 + [4] * 2 + [3] * 4
DELTA = [-50, 0, 49, 100, 150, 2, 49, -64, -21, 22, 65]
ALIGNED = [272, 351, 309, 305, 184, 204, 189, 189, 356, 460, 381]
# the largest count the plain scan / any rung of speed_ladder() reaches on each window (the same measurement)
PLAIN = [67, 85, 85, 85, 75, 7, 13, 17, 17, 17, 14]
SPEED = [67, 85, 85, 85, 75, 25, 25, 63, 89, 97, 88]
MIN_ALIGNED = 140                                        # between the two populations: at most 97 there, at least 184 here
SEGMENTS = ((1, 0, 4, (76548, 65536)), (4, 5, 6, (71042, 63561)), (3, 7, 10, (65536, 63561)))   # song, first, last, pair
# the work of the two searches over tempo_ladder(0.8, 1.2) x pitch_ladder() on the fixture (DESIGN.md 3.7i states them):
# (warped hash entries written, window entries handed to the match)
WORK_GRID = (5462226, 12281182)
WORK_SEPARABLE = (723714, 1495742)


def songs():
    return [WT.notes_clip(7, c, 20) for c in range(4)]


def recording():
    from oracle import synth
    return np.concatenate([synth.traffic_noise(5, 0, 2 * SR)] + [WT.notes_clip(7, c, sec, a, p) for c, a, p, sec in PIECES] +
                          [synth.traffic_noise(5, 1, int(1.05 * SR))])


def make_db(S, ctx, song_list):
    """Songs 1..4 in a fresh table; returns (db, key32 -> [(sid, offset)]): one set of rows for the device table and the CPU vote."""
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(song_list, ctx=ctx)
    per_song = []
    for c in range(len(song_list)):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        assert sid == c + 1
        d.set_song_fingerprinted(sid)
        per_song.append((k[int(ho[c]):int(ho[c + 1])], t1[int(ho[c]):int(ho[c + 1])]))
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    return d, T.table_of(per_song)


def flatten(S, recordings):
    chans, first = [], [0]
    for r in recordings:
        cs = [r] if (isinstance(r, np.ndarray) and r.ndim == 1) else list(r)
        chans.extend(S._as_pcm(c) for c in cs)
        first.append(len(chans))
    off = np.zeros(len(chans) + 1, np.uint64)
    if chans:
        off[1:] = np.cumsum([len(c) for c in chans])
    pcm = np.concatenate(chans) if off[-1] else np.zeros(1, np.int16)
    return chans, pcm, off, np.asarray(first, np.uint32)


def device_peaks(ctx, chans, pcm, off, first):
    """(chan_peaks, frames) for the twin's recipe: the peaks of the device extraction per recording and channel."""
    pf, pt, po = ctx.peaks(pcm, off)
    peaks, frames = [], []
    for r in range(len(first) - 1):
        cs = range(int(first[r]), int(first[r + 1]))
        peaks.append([(pf[int(po[c]):int(po[c + 1])], pt[int(po[c]):int(po[c + 1])]) for c in cs])
        frames.append(max((ctx.frames_of(len(chans[c])) for c in cs), default=0))
    return peaks, frames


def same(got, want, what="", names=ARRAYS + ("best", "profile")):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name, got[name].shape, want[name].shape)
        assert np.array_equal(got[name], want[name]), (what, name)


def check(S, db, recordings, window, step, tempos, pitches, select=None, topns=(2,), full_sorts=(False,), what=""):
    """scan_warps against the host recipe (device peaks, the twin's warp, cut and fold, Table.match), array for array and
    the two work counts; returns the last result and win_off.  select: a function (n_wins) -> (sel_off, sel_warp), or None."""
    ctx = db.ctx
    chans, pcm, off, first = flatten(S, recordings)
    peaks, frames = device_peaks(ctx, chans, pcm, off, first)
    n_wins = sum(SW.window_count(int(F), window, step) if p else 0 for p, F in zip(peaks, frames))
    sel = None if select is None else select(n_wins)
    hk, hq, hqo, hwo, work = SW.host_queries(peaks, frames, window, step, tempos.tolist(), pitches.tolist(), sel)
    for topn in topns:
        for fs_ in full_sorts:
            m = db.table.match(hk, hq, hqo, topn, full_sort=fs_)
            want = SW.fold_best(m, int(hwo[-1]), tempos.tolist(), pitches.tolist(), topn, sel)
            got, win_off, ms = ctx.scan_warps(db.table, pcm, off, first, window, step, tempos, pitches, sel, topn=topn, full_sort=fs_)
            assert np.array_equal(win_off, hwo), (what, win_off, hwo)
            same(got, want, (what, topn, fs_))
            assert got["work"] == work, (what, got["work"], work)
            assert len(ms) == 4 and all(x >= 0.0 for x in ms)
    return got, win_off
