"""GPU: shz_resample_i16 equals the numpy statement of its integer formula (tests/resample_twin.py) bit for bit -- the
product's own plans, random plans at the limits, every memory mode, chunked input -- and audio at 48, 32, 22.05 and 16 kHz
is found in a 44.1 kHz table through resample_to / fs_in / target_fs, with the results of the existing path fed with the
twin's samples."""
import numpy as np
import pytest

from resample_twin import resample_twin, song_at_rate

pytestmark = pytest.mark.gpu

PAIRS = [(8000, 44100), (11025, 44100), (16000, 44100), (22050, 44100), (32000, 44100), (48000, 44100), (96000, 44100),
         (44100, 48000)]
HOP = 2048


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _pack(clips):
    off = np.zeros(len(clips) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in clips])
    pcm = np.concatenate(clips) if off[-1] else np.zeros(1, np.int16)
    return np.ascontiguousarray(pcm, np.int16), off


def _check_batch(ctx, clips, plan, what=""):
    L, M, T, taps = plan
    pcm, off = _pack(clips)
    out, oo = ctx.resample(pcm, off, L, M, T, taps)
    assert int(oo[-1]) == len(out)
    for c, x in enumerate(clips):
        want = resample_twin(x, L, M, T, taps)
        got = out[int(oo[c]):int(oo[c + 1])]
        assert len(got) == len(want) == -(-len(x) * L // M), (what, c)
        assert np.array_equal(got, want), (what, c, len(x), int(np.flatnonzero(got != want)[0]))


# ---- 1. kernel == twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
def test_product_plans_edge_lengths(S, ctx, pair):
    plan = S.resample_plan(*pair)
    T = plan[2]
    rng = np.random.default_rng(pair[0])
    lens = [0, 1, T // 2, T, 9973, 3 * T + 17, 40000]          # 7 clips a call
    clips = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens]
    _check_batch(ctx, clips, plan, pair)
    _check_batch(ctx, clips[4:5], plan, pair)                    # 1 clip a call


@pytest.mark.parametrize("pair", PAIRS)
def test_thirty_seconds(S, ctx, pair):
    rng = np.random.default_rng(7)
    _check_batch(ctx, [rng.integers(-32768, 32768, 30 * pair[0]).astype(np.int16)], S.resample_plan(*pair), pair)


def test_thousand_clips(S, ctx):
    rng = np.random.default_rng(11)
    clips = [rng.integers(-32768, 32768, int(n)).astype(np.int16) for n in rng.integers(0, 3000, 1000)]
    _check_batch(ctx, clips, S.resample_plan(48000, 44100), "1000 clips")


# (L, M, T): odd L and M up to the limits (L, M <= 2^24, L T <= 2^24), tap tables in LDS and in global memory, tiles of one output
RANDOM_PLANS = [(1, 1, 2), (8388607, 5, 2), (3, 16777215, 32), (524287, 999983, 32), (239673, 7, 70), (147, 321, 70),
                (4095, 4093, 4096), (3, 5, 4096), (1, 3, 4096), (441, 81, 32), (35, 16777215, 4096)]


@pytest.mark.parametrize("L,M,T", RANDOM_PLANS)
def test_random_plans_full_range(ctx, L, M, T):
    """Taps over the whole int32 range, PCM at the ends of int16: sums reach 2^58 and the output saturates; clips of tiny
    amplitude keep the same sums inside int16 so that unsaturated values are compared too."""
    rng = np.random.default_rng(L * 31 + T)
    taps = rng.integers(-2 ** 31, 2 ** 31, (L, T), dtype=np.int64).astype(np.int32)
    taps[0, :] = -2 ** 31
    taps[-1, :] = 2 ** 31 - 1
    cap_n = max(1, 1_500_000 * M // L)                            # keeps a clip's outputs below 1.5 million
    lens = sorted({min(n, cap_n) for n in (0, 1, T // 2, T, 9973)})
    if T <= 70:
        lens.append(min(30 * 16000, cap_n))                       # 30 s at 16 kHz (T = 4096: test_thirty_seconds_at_4096_taps)
    clips = []
    for i, n in enumerate(lens):
        if i % 2 == 0:
            x = rng.choice(np.array([-32768, 32767], np.int16), n)
        else:
            x = rng.integers(-1, 2, n).astype(np.int16)
        clips.append(x)
    clips.append(np.full(min(2 * T + 3, cap_n), -32768, np.int16))
    _check_batch(ctx, clips, (L, M, T, taps), (L, M, T))


def test_thirty_seconds_at_4096_taps(ctx):
    """30 s at 16 kHz through a 4096-tap plan whose table sits in LDS."""
    L, M, T = 3, 5, 4096
    rng = np.random.default_rng(5)
    taps = rng.integers(-2 ** 31, 2 ** 31, (L, T), dtype=np.int64).astype(np.int32)
    x = rng.integers(-2, 3, 30 * 16000).astype(np.int16)
    x[::1000] = -32768
    _check_batch(ctx, [x], (L, M, T, taps), "30 s, T = 4096")


@pytest.mark.parametrize("pair", [(48000, 44100), (8000, 44100), (96000, 44100)])
def test_neighbours_do_not_leak(S, ctx, pair):
    plan = S.resample_plan(*pair)
    L, M, T, taps = plan
    clips = [np.full(5000, 32767, np.int16), np.zeros(3000, np.int16), np.full(5000, -32768, np.int16)]
    pcm, off = _pack(clips)
    out, oo = ctx.resample(pcm, off, L, M, T, taps)
    mid = out[int(oo[1]):int(oo[2])]
    assert len(mid) == -(-3000 * L // M) and not mid.any()
    _check_batch(ctx, clips, plan, "neighbours")


def test_memory_modes_and_capacity(S, ctx):
    from shazam_amd import _ffi
    L, M, T, taps = S.resample_plan(48000, 44100)
    rng = np.random.default_rng(3)
    clips = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (5000, 1, 12345)]
    pcm, off = _pack(clips)
    want = np.concatenate([resample_twin(x, L, M, T, taps) for x in clips])
    dpcm = ctx.alloc(pcm.nbytes)
    dpcm.upload(pcm)
    dout = ctx.alloc(len(want) * 2)
    for pcm_dev in (False, True):
        for out_dev in (False, True):
            rc, out, oo, n = ctx.resample_raw(dpcm if pcm_dev else pcm, off, L, M, T, taps, pcm_device=pcm_dev,
                                              out=dout if out_dev else None, cap=len(want))
            assert rc == _ffi.OK and n == len(want)
            got = dout.download(np.int16, len(want)) if out_dev else out
            assert np.array_equal(got, want), (pcm_dev, out_dev)
            assert [int(v) for v in oo] == [0] + np.cumsum([-(-len(x) * L // M) for x in clips]).tolist()
    # a first clip that does not start the buffer, on a 2-byte boundary
    off2 = off.copy()
    off2[0] = 3
    for pcm_dev in (False, True):
        out, oo = ctx.resample(dpcm if pcm_dev else pcm, off2, L, M, T, taps, pcm_device=pcm_dev)
        assert np.array_equal(out[:int(oo[1])], resample_twin(clips[0][3:], L, M, T, taps))
    for out_dev in (False, True):
        rc, _, _, n = ctx.resample_raw(pcm, off, L, M, T, taps, out=dout if out_dev else None, cap=len(want) - 1)
        assert rc == _ffi.E_CAPACITY and n == len(want)
    dpcm.free()
    dout.free()


def test_invalid_arguments(ctx):
    from shazam_amd import _ffi
    pcm, off = np.zeros(100, np.int16), np.array([0, 100], np.uint64)
    t = np.zeros((4, 4096), np.int32)
    for L, M, T in ((0, 1, 2), (1, 0, 2), (1, 1, 0), (1, 1, 3), (1, 1, 4098)):
        assert ctx.resample_raw(pcm, off, L, M, T, t, cap=1000)[0] == _ffi.E_INVALID, (L, M, T)
    assert ctx.resample_raw(pcm, np.array([0, 60, 50], np.uint64), 1, 1, 2, t, cap=1000)[0] == _ffi.E_INVALID
    assert ctx.resample_raw(pcm, off, 1, 1, 2, t, m_first=[5], m_end=[4], cap=1000)[0] == _ffi.E_INVALID
    assert ctx.resample_raw(pcm, off, 3, 2, 2, t, cap=1000)[0] == _ffi.OK


# ---- 2. chunked == whole ----------------------------------------------------------------------------------------------
def _chunks(n, size, rng):
    cuts, pos = [0], 0
    while pos < n:
        pos = min(n, pos + (int(rng.integers(0, 20000)) if size is None else size))
        cuts.append(pos)
    return cuts


@pytest.mark.parametrize("size,n", [(1, 700), (4095, 60000), (8192, 60000), (None, 150000)])
@pytest.mark.parametrize("pair", [(48000, 44100), (96000, 44100), (16000, 44100)])
def test_stream_resampler_equals_whole(S, ctx, pair, size, n):
    rng = np.random.default_rng(n + (size or 0))
    xs = [rng.integers(-32768, 32768, n).astype(np.int16), rng.integers(-32768, 32768, n // 2 + 3).astype(np.int16)]
    whole = S.resample_batch(xs, pair[0], pair[1], ctx=ctx)
    T = S.resample_plan(*pair)[2]
    for with_end in (True, False):
        rs = S.StreamResampler(2, pair[0], pair[1], ctx=ctx)
        cuts = _chunks(n, size, rng)
        got = [[], []]
        for a, b in zip(cuts[:-1], cuts[1:]):
            last = b == n
            out = rs.push([x[a:b] for x in xs], end=True if (last and with_end) else None)
            for i in range(2):
                got[i].append(out[i])
        for i in range(2):
            g = np.concatenate(got[i])
            if with_end:
                assert g.tobytes() == whole[i].tobytes(), (pair, size, i)
            else:   # everything whose newest input has arrived: a prefix that stops less than T / 2 inputs short of the end
                L, M = S.resample_plan(*pair)[:2]
                assert len(g) == max(0, -(-(len(xs[i]) - T // 2) * L // M))
                assert g.tobytes() == whole[i][:len(g)].tobytes(), (pair, size, i)


def test_in_base_and_output_range(S, ctx):
    L, M, T, taps = S.resample_plan(96000, 44100)
    rng = np.random.default_rng(9)
    x = rng.integers(-32768, 32768, 50000).astype(np.int16)
    whole = resample_twin(x, L, M, T, taps)
    # pieces [a, b) of the clip with the outputs whose inputs they hold; two pieces in one call
    pieces = [(0, 20000), (19000, 50000)]
    rng_m = []
    for a, b in pieces:
        m1 = 0 if a == 0 else -(-(a + T) * L // M)               # i0 - T + 1 >= a
        m2 = len(whole) if b == len(x) else max(m1, (b - T) * L // M)
        rng_m.append((m1, m2))
    pcm, off = _pack([x[a:b] for a, b in pieces])
    out, oo = ctx.resample(pcm, off, L, M, T, taps, in_base=[a for a, _ in pieces], m_first=[m for m, _ in rng_m],
                           m_end=[m for _, m in rng_m])
    for c, (m1, m2) in enumerate(rng_m):
        assert m2 > m1 and np.array_equal(out[int(oo[c]):int(oo[c + 1])], whole[m1:m2]), c
    # a buffer that does not hold all the inputs of its range: what lies outside reads as zero, as in the twin
    out, oo = ctx.resample(x[1000:3000], [0, 2000], L, M, T, taps, in_base=[1000], m_first=[300], m_end=[1800])
    assert np.array_equal(out, resample_twin(x[1000:3000], L, M, T, taps, in_base=1000, m_first=300, m_end=1800))


# ---- 3. extraction -----------------------------------------------------------------------------------------------------
def test_extraction_equals_existing_path_on_twin_samples(S, ctx):
    L, M, T, taps = S.resample_plan(48000, 44100)
    clips48 = [song_at_rate(40 + i, 48000, seconds=6.0 + i) for i in range(3)] + [np.zeros(0, np.int16)]
    want = S.fingerprint_batch([resample_twin(c, L, M, T, taps) for c in clips48], Fs=44100, ctx=ctx)
    got = S.fingerprint_batch(clips48, Fs=48000, ctx=ctx, resample_to=44100)
    assert len(want[0]) > 100
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert S.fingerprint(clips48[1], Fs=48000, resample_to=44100) == S.fingerprint(resample_twin(clips48[1], L, M, T, taps), Fs=44100)
    # another hop goes through the same path
    a = S.fingerprint_batch(clips48[:1], Fs=48000, ctx=ctx, wratio=0.75, resample_to=44100)
    b = S.fingerprint_batch([resample_twin(clips48[0], L, M, T, taps)], Fs=44100, ctx=ctx, wratio=0.75)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ---- 4. recognition ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def song_db(S, ctx):
    db = S.get_database("hip")(ctx=ctx)
    for s in range(4):
        fp = set(S.fingerprint(song_at_rate(100 + s, 44100)))
        sid = db.insert_song(f"song{s}", "AB" * 20, len(fp))
        db.insert_hashes(sid, fp)
        db.set_song_fingerprinted(sid)
    db.finalize()
    return db


@pytest.mark.parametrize("fs", [48000, 32000, 22050, 16000])
def test_recognition_across_rates(S, ctx, song_db, fs):
    """Four analytic songs at 44.1 kHz in the table, 10 s of song index 2 (song_id 3) from frame 7 sampled at fs.  The numpy
    pipeline (oracle/cpu_ref.py on the twin's samples) gave 414 of 426 hashes at 48, 32 and 22.05 kHz and 248 of 346 at 16 kHz."""
    q = song_at_rate(102, fs, seconds=10.0, t0=7 * HOP / 44100)
    raw, *_ = S.recognize(q, db=song_db, Fs=fs)
    assert not raw or raw[0]["song_id"] != 3
    L, M, T, taps = S.resample_plan(fs, 44100)
    y = resample_twin(q, L, M, T, taps)
    for fused in (False, True):
        got, *_ = S.recognize(q, db=song_db, Fs=fs, fused=fused, resample_to=44100)
        assert got and got[0]["song_id"] == 3 and got[0]["offset"] == 7
        if fs != 16000:
            assert 2 * got[0]["hashes_matched_in_input"] >= got[0]["input_total_hashes"]
        want, *_ = S.recognize(y, db=song_db, Fs=44100, fused=fused)
        assert got == want
    # two queries, one of them stereo, in one batch
    res, _ = S.recognize_batch([q, [q, q[::-1].copy()]], song_db, Fs=fs, resample_to=44100, fused=True)
    ref, _ = S.recognize_batch([y, [y, resample_twin(q[::-1], L, M, T, taps)]], song_db, Fs=44100, fused=True)
    assert res == ref and res[0][0]["song_id"] == 3


@pytest.mark.parametrize("device", [False, True])
def test_stream_recognizer_at_48k(S, ctx, song_db, device):
    q = song_at_rate(102, 48000, seconds=10.0, t0=7 * HOP / 44100)
    L, M, T, taps = S.resample_plan(48000, 44100)
    y = resample_twin(q, L, M, T, taps)
    rec = S.StreamRecognizer(song_db, 1, window_seconds=30, device=device, fs_in=48000)
    ref = S.StreamRecognizer(song_db, 1, window_seconds=30, device=device)
    pos, last = 0, None
    for a in range(0, len(q), 8192):
        end = [0] if a + 8192 >= len(q) else None
        last = rec.push([q[a:a + 8192]], end=end)
    for a in range(0, len(y), 8192):
        end = [0] if a + 8192 >= len(y) else None
        want = ref.push([y[a:a + 8192]], end=end)
    results, w0 = last[0]
    assert results and results[0]["song_id"] == 3 and results[0]["offset"] + w0 == 7
    assert last == want          # the same hashes in the window as the twin's samples give
    rec.close()
    ref.close()


def test_stream_fingerprinter_fs_in(S, ctx):
    x = song_at_rate(77, 32000, seconds=8.0)
    fp = S.StreamFingerprinter(1, ctx=ctx, fs_in=32000)
    ks, ts = [], []
    for a in range(0, len(x), 8192):
        k, t1, _ = fp.push([x[a:a + 8192]], end=[0] if a + 8192 >= len(x) else None)
        ks.append(k)
        ts.append(t1)
    fp.close()
    k, t1, _ = S.fingerprint_batch([x], Fs=32000, ctx=ctx, resample_to=44100)
    assert len(k) > 50 and np.array_equal(np.concatenate(ks), k) and np.array_equal(np.concatenate(ts), t1)


# ---- 5. ingest ---------------------------------------------------------------------------------------------------------
def test_ingest_target_fs(S, ctx, tmp_path):
    from shazam_amd import ingest
    songs = {"a48": (song_at_rate(201, 48000, seconds=20.0), 48000), "b44": (song_at_rate(202, 44100, seconds=20.0), 44100)}
    for name in songs:
        (tmp_path / f"{name}.wav").write_bytes(name.encode())      # the reader is injected: the files only carry names

    def reader(fn, limit=None):
        x, fs = songs[fn.split("/")[-1][:-4]]
        return [x], fs, fn[-7:].upper()

    db = S.get_database("hip")(ctx=ctx)
    done = ingest.fingerprint_directory(str(tmp_path), [".wav"], db, reader=reader, target_fs=44100)
    ids = {name: sid for sid, name, _ in done}
    assert set(ids) == {"a48", "b44"}
    for seed, name in ((201, "a48"), (202, "b44")):
        q = song_at_rate(seed, 44100, seconds=8.0, t0=20 * HOP / 44100)
        got, *_ = S.recognize(q, db=db)
        assert got and got[0]["song_id"] == ids[name] and got[0]["offset"] == 20, name
    # without target_fs the 48 kHz file is in the table at its own rate, and a 44.1 kHz query does not find it
    db2 = S.get_database("hip")(ctx=ctx)
    done2 = ingest.fingerprint_directory(str(tmp_path), [".wav"], db2, reader=reader)
    got, *_ = S.recognize(song_at_rate(201, 44100, seconds=8.0, t0=20 * HOP / 44100), db=db2)
    assert not got or got[0]["song_id"] != {n: s for s, n, _ in done2}["a48"]


# ---- 6. defaults -------------------------------------------------------------------------------------------------------
def test_defaults_unchanged(S, ctx, song_db):
    x = song_at_rate(102, 44100, seconds=6.0, t0=7 * HOP / 44100)
    a = S.fingerprint_batch([x], ctx=ctx)
    for kw in ({"resample_to": None}, {"resample_to": 44100}):
        for u, v in zip(a, S.fingerprint_batch([x], ctx=ctx, **kw)):
            assert np.array_equal(u, v)
    r0, *_ = S.recognize(x, db=song_db)
    r1, *_ = S.recognize(x, db=song_db, resample_to=None)
    assert r0 == r1 and r0[0]["song_id"] == 3
    assert S.fingerprint(x) == S.fingerprint(x, resample_to=None)
