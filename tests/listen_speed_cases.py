"""Test helpers for the listeners at a ladder (not a conftest, not collected): the corpus, the ladder and the streams the
host test and the GPU tests share, made by the oracle's synthesiser and speed_twin.speed_up alone."""
import numpy as np

import listen_speed_twin as LT
import speed_twin as T
from oracle import cpu_ref as O, synth

SR = 44100
SEED = 7
N_SONGS, SONG_S, STREAM_S = 8, 20, 14
STREAM_LEN = STREAM_S * SR
WINDOW_FRAMES = 107                     # int(5 s * 44100 / 2048), what StreamRecognizer(window_seconds=5) derives
CHUNK = 8192
TOPN = 2
STEP = 92                               # shazam_amd.speed.DEFAULT_STEP_Q16
FAST = 1.03
FAST_SONG, FAST_SECOND = 5, 3           # the 1.03 listener: songs[5] (song id 6) from second 3
PLAIN_SONG, PLAIN_SECOND = 2, 2         # the 1.0 listener: songs[2] (song id 3) from second 2


def songs():
    return [synth.music_clip(SEED, c, SONG_S * SR) for c in range(N_SONGS)]


def ladder():
    """7 rungs on the default grid (step 92 / 65536, anchored at 65536): 65536 and its neighbours, the rung nearest 1.03 and
    its neighbours, and a slow one."""
    mid = 65536 + STEP * int(round((T.q16(FAST) - 65536) / STEP))
    lad = np.asarray(sorted({65536 - 21 * STEP, 65536 - STEP, 65536, 65536 + STEP, mid - STEP, mid, mid + STEP}), np.uint32)
    assert len(lad) == 7 and abs(int(mid) - T.q16(FAST)) <= STEP // 2
    return lad


def cut(song, second: int, s: float, n: int = STREAM_LEN):
    """n samples of the song from `second` on, played s times as fast"""
    return T.speed_up(song[second * SR: second * SR + int(n * s) + 2], s)[:n]


def streams(sg):
    """The four streams of 2 listeners x 2 channels: listener 0 hears songs[5] at 1.03 (second channel: 20 dB noise),
    listener 1 songs[2] at 1.0 with 10 dB noise on its second channel."""
    fast, plain = cut(sg[FAST_SONG], FAST_SECOND, FAST), cut(sg[PLAIN_SONG], PLAIN_SECOND, 1.0)
    return [fast, synth.mix_query(fast, synth.synth_clip(5, 8, len(fast), 0, 8000), 20.0),
            plain, synth.mix_query(plain, synth.synth_clip(5, 9, len(plain), 0, 8000), 10.0)]


def oracle_peaks(x):
    """(f, t) of the signal's peaks, (t asc, f asc)"""
    _, _, f, t = O.fingerprint_keys(x)
    return np.asarray(f), np.asarray(t)


def oracle_table(sg):
    """key32 -> [(sid, offset)] of the songs, ids from 1 (speed_twin.table_of)"""
    return T.table_of([O.fingerprint_keys(x)[:2] for x in sg])


def full_window_pushes(n_samples: int, chunk: int = CHUNK, window_frames: int = WINDOW_FRAMES):
    """[(samples after the push, ended, H)] of a stream fed n_samples in chunks, ending with the last, for the pushes at
    which the window is full (H > window_frames)"""
    out = []
    for a in range(0, n_samples, chunk):
        got, ended = min(a + chunk, n_samples), a + chunk >= n_samples
        h = LT.horizon(got, ended)
        if h > window_frames:
            out.append((got, ended, h))
    return out


def end_to_end_ok(top, w0: int, lad, song_id: int = FAST_SONG + 1, second: int = FAST_SECOND, s: float = FAST):
    """The three end-to-end conditions on a listener's top answer (sid, delta, speed16): the song, the speed within one rung,
    the offset within 2 frames of where stream frame w0 lies in the song -- 1 for the vote's own rounding, 1 for the
    rounding of w0 s (the rung's own error over a 107-frame window is below 0.1 frame)."""
    sid, delta, s16 = top
    return sid == song_id and abs(int(s16) - T.q16(s)) <= STEP and abs(delta - (second * SR / 2048 + w0 * s)) <= 2


def build_db(S, ctx, sg):
    """The songs as ids 1..len(sg) in a device table, built as in test_gpu_speed_recognize.py; returns (db, key32 ->
    [(sid, offset)]): one set of rows for the device table and for the CPU vote."""
    d = S.get_database("hip")(ctx=ctx)
    k, t1, ho = S.fingerprint_batch(sg, ctx=ctx)
    per_song = []
    for c in range(len(sg)):
        sid = d.insert_song(f"song{c}", "AB" * 20, int(ho[c + 1] - ho[c]))
        assert sid == c + 1
        d.set_song_fingerprinted(sid)
        per_song.append((k[int(ho[c]):int(ho[c + 1])], t1[int(ho[c]):int(ho[c + 1])]))
    d.table.insert_clips(k, t1, ho, 1)
    d.table.finalize()
    return d, T.table_of(per_song)


class Feed:
    """n streams fed from their signals push by push: keeps every stream's position and end, gives the chunks of a push and
    the horizons after it (listen_speed_twin.horizon)."""

    def __init__(self, signals):
        self.sig, self.n = list(signals), len(signals)
        self.pos, self.ended = [0] * self.n, [False] * self.n

    def take(self, sizes, end=()):
        """sizes[i]: samples for stream i (None: nothing); end: streams that end with this chunk.  Returns (chunks, ends)."""
        chunks = []
        for i, n in enumerate(sizes):
            if n is None or self.ended[i]:
                chunks.append(None)
                continue
            c = self.sig[i][self.pos[i]:self.pos[i] + int(n)]
            self.pos[i] += len(c)
            chunks.append(c)
        ends = [i for i in end if not self.ended[i]]
        for i in ends:
            self.ended[i] = True
        return chunks, ends or None

    def horizons(self):
        return [LT.horizon(self.pos[i], self.ended[i]) for i in range(self.n)]

    def reset(self, which):
        for i in which:
            self.pos[i], self.ended[i] = 0, False
