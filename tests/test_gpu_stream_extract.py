"""GPU: live streams (shz_streams_*) give, push by push, exactly the hashes of fingerprint() on the whole signal -- same
keys, same t1, same order -- and give each hash as soon as the emission rule allows, no sooner and no later.

Emission rule (include/shz.h): settled peaks are those of frames < H (H = complete frames - 10, at the end
all frames); a settled peak i (time-major order) emits once fan - 1 settled peaks follow it, or once H > t_i + 200, or
when the stream ends."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAN = 5


@pytest.fixture(scope="module")
def S():
    import shazam_amd
    return shazam_amd


@pytest.fixture(scope="module")
def ctx(S):
    return S.get_context(0)


def _fixtures(golden_dir):
    """(name, pcm, Fs, golden npz, key prefix) of every extraction fixture."""
    from oracle import synth
    out = []
    g = np.load(os.path.join(golden_dir, "wav_kat.npz"))
    for fs in (22050, 44100):
        out.append((f"wav{fs}", g["pcm"], fs, g, f"fs{fs}_"))
    g = np.load(os.path.join(golden_dir, "synth_clips.npz"))
    for name in ("white_5s", "white_30s", "tonal_5s", "tonal_30s", "tonal_list_input_2s"):
        seed, clip, n, ta, na = (int(v) for v in g[f"{name}_params"])
        out.append((name, synth.synth_clip(seed, clip, n, ta, na), 44100, g, f"{name}_"))
    g = np.load(os.path.join(golden_dir, "edge_cases.npz"))
    for name in ("short_3000", "exact_4096", "ragged_6143", "two_frames_6144", "silence_20000", "square_p64",
                 "gap_250_frames", "loud_fullscale", "dc_offset"):
        out.append((name, g[f"{name}_pcm"], 44100, g, f"{name}_"))
    g = np.load(os.path.join(golden_dir, "tie_cases.npz"))
    for name, x in synth.tie_inputs().items():
        out.append((name, x, int(g[f"{name}_Fs"]), g, f"{name}_"))
    return out


def _schedules(n, seed):
    rng = np.random.default_rng(seed)
    out = {"chunk8192": list(range(0, n, 8192)) + [n]}
    b, pos = [0], 0
    while pos < n:
        pos = min(n, pos + int(rng.integers(0, 300001)))
        b.append(pos)
    out["random"] = b
    k = min(n, 12000)
    out["single_then_big"] = list(range(0, k + 1)) + list(range(k + 100000, n, 100000)) + [n]
    out["one_push"] = [0, n]
    return out


def _expected_emitted(pt, H, ending, fan=FAN):
    """Hashes the rule has released once the horizon is H: those of the first e settled peaks (pt: time-major peak
    times of the whole signal)."""
    m = int(np.searchsorted(pt, H, side="left")) if not ending else len(pt)
    if ending:
        e = m
    else:
        e = max(m - (fan - 1), int(np.searchsorted(pt, H - 200, side="left")) if H > 200 else 0, 0)
    n = 0
    for i in range(e):
        for j in range(i + 1, min(i + fan, len(pt))):
            if pt[j] - pt[i] <= 200:
                n += 1
    return n


def _stream_one(S, ctx, x, bounds, fs, pt=None, fan=FAN):
    st = S._ffi.Streams(ctx, 1, fs, 10.0, fan)
    try:
        ks, ts = [], []
        total = 0
        for i in range(len(bounds) - 1):
            ending = i == len(bounds) - 2
            k, t1, ho = st.push([x[bounds[i]:bounds[i + 1]]], end=[0] if ending else None)
            assert ho[1] == len(k)
            ks.append(k)
            ts.append(t1)
            total += len(k)
            s = st.state(0)
            assert s["samples"] == bounds[i + 1] and s["emitted"] == total
            assert s["pending"] <= fan - 1
            if pt is not None:
                assert total == _expected_emitted(pt, s["settled"], ending, fan), (i, s)
        return np.concatenate(ks), np.concatenate(ts)
    finally:
        st.close()


def test_fixtures_every_schedule_bit_exact(S, ctx, golden_dir):
    for name, x, fs, g, p in _fixtures(golden_dir):
        x = np.ascontiguousarray(x, np.int16)
        n = len(x)
        wk, wt, _, _ = ctx.fingerprint_batch(x if n else np.zeros(1, np.int16), np.array([0, n], np.uint64), fs=fs)
        hexes = S.hex_of_keys(ctx, wk) if len(wk) else []
        assert [h.encode() for h in hexes] == list(g[f"{p}hash_hex"]), name
        assert wt.tolist() == list(g[f"{p}hash_t1"]), name
        _, pt, _ = ctx.peaks(x if n else np.zeros(1, np.int16), np.array([0, n], np.uint64), fs=fs)
        pt = pt.astype(np.int64)
        for sname, b in _schedules(n, zlib.crc32(name.encode())).items():
            k, t1 = _stream_one(S, ctx, x, b, fs, pt if sname != "single_then_big" else None)
            assert np.array_equal(k, wk) and np.array_equal(t1, wt), (name, sname, len(k), len(wk))


def test_liveness_single_samples(S, ctx):
    """Liveness also while samples trickle in one at a time (the rule checked after every push)."""
    from oracle import synth
    x = synth.synth_clip(3, 1, 60000, 4000, 2000)
    _, pt, _ = ctx.peaks(x, np.array([0, len(x)], np.uint64))
    wk, wt, _, _ = ctx.fingerprint_batch(x, np.array([0, len(x)], np.uint64))
    b = list(range(0, 2048 * 12)) + list(range(2048 * 12, len(x), 777)) + [len(x)]
    k, t1 = _stream_one(S, ctx, x, b, 44100, pt.astype(np.int64))
    assert np.array_equal(k, wk) and np.array_equal(t1, wt)


def test_many_streams_mixed_rates_end_and_reuse(S, ctx):
    from oracle import synth
    rng = np.random.default_rng(42)
    n = 256
    st = S._ffi.Streams(ctx, n, 44100, 10.0, FAN)
    sig_id = 0

    def new_signal():
        nonlocal sig_id
        sig_id += 1
        ln = int(rng.integers(0, 44100 * 6))
        return synth.synth_clip(900, sig_id, ln, int(rng.integers(0, 5000)), int(rng.integers(500, 9000)))

    sigs = [new_signal() for _ in range(n)]
    pos = [0] * n
    got = [[[], []] for _ in range(n)]
    done = []            # (signal, keys, t1) of streams that ended
    reused = 0
    for rnd in range(40):
        chunks, ends = [], []
        for i in range(n):
            if sigs[i] is None or rng.random() < 0.2:    # nothing for this stream in this push
                chunks.append(None)
                continue
            step = int(rng.integers(0, 60000))
            c = sigs[i][pos[i]:pos[i] + step]
            pos[i] += len(c)
            chunks.append(c)
            if pos[i] >= len(sigs[i]) and rng.random() < 0.7:
                ends.append(i)
        k, t1, ho = st.push(chunks, end=ends)
        for i in range(n):
            got[i][0].append(k[ho[i]:ho[i + 1]])
            got[i][1].append(t1[ho[i]:ho[i + 1]])
        for i in ends:
            done.append((sigs[i], np.concatenate(got[i][0]), np.concatenate(got[i][1])))
            got[i] = [[], []]
            sigs[i] = None
        # some ended slots are reset and reused for a new signal
        free = [i for i in range(n) if sigs[i] is None]
        if free and rnd < 30:
            pick = free[: max(1, len(free) // 2)]
            st.reset(pick)
            for i in pick:
                sigs[i], pos[i] = new_signal(), 0
                reused += 1
    # end everything still open (ending with an empty chunk)
    open_ = [i for i in range(n) if sigs[i] is not None]
    k, t1, ho = st.push([None] * n, end=open_)
    for i in open_:
        got[i][0].append(k[ho[i]:ho[i + 1]])
        got[i][1].append(t1[ho[i]:ho[i + 1]])
        done.append((sigs[i][:pos[i]], np.concatenate(got[i][0]), np.concatenate(got[i][1])))
    st.close()
    assert reused > 20 and len(done) == n + reused
    clips = [d[0] for d in done]
    wk, wt, ho = S.fingerprint_batch(clips, ctx=ctx)
    for c, (_, k, t1) in enumerate(done):
        assert np.array_equal(k, wk[ho[c]:ho[c + 1]]) and np.array_equal(t1, wt[ho[c]:ho[c + 1]]), c


def test_fp64_fallback_inside_a_push(S, ctx):
    from oracle import synth
    click = np.zeros(2048 * 400, np.int16)
    click[1024::2048] = 20000          # a click per hop: hundreds of tied cells a window, redone with fp64 staging
    train = synth.tie_inputs()["click_train_30s"]
    sigs = [click, train] + [synth.synth_clip(5, i, 2048 * 300, 0, 8000) for i in range(6)]
    n = len(sigs)
    s0 = ctx.extract_stats()
    st = S._ffi.Streams(ctx, n, 44100, 10.0, FAN)
    got = [[] for _ in range(n)]
    gt = [[] for _ in range(n)]
    longest = max(len(x) for x in sigs)
    for a in range(0, longest, 88200):
        ends = [i for i in range(n) if a < len(sigs[i]) <= a + 88200]
        k, t1, ho = st.push([x[a:a + 88200] for x in sigs], end=ends)
        for i in range(n):
            got[i].append(k[ho[i]:ho[i + 1]])
            gt[i].append(t1[ho[i]:ho[i + 1]])
    st.close()
    s1 = ctx.extract_stats()
    assert s1["f64_clips"] > s0["f64_clips"]
    for i, x in enumerate(sigs):
        wk, wt, _, _ = ctx.fingerprint_batch(x, np.array([0, len(x)], np.uint64))
        assert np.array_equal(np.concatenate(got[i]), wk) and np.array_equal(np.concatenate(gt[i]), wt), i


def test_non_default_overlap_and_hop_change(S, ctx):
    from oracle import synth
    x = synth.synth_clip(8, 2, 441000, 4000, 3000)
    ctx.set_overlap(int(4096 * 0.75))
    try:
        wk, wt, _, _ = ctx.fingerprint_batch(x, np.array([0, len(x)], np.uint64))
        st = S._ffi.Streams(ctx, 1, 44100, 10.0, FAN)
        b = list(range(0, len(x), 8192)) + [len(x)]
        ks, ts = [], []
        for i in range(len(b) - 2):
            k, t1, _ = st.push([x[b[i]:b[i + 1]]])
            ks.append(k)
            ts.append(t1)
        ctx.set_overlap(2048)    # the hop changes under the stream
        with pytest.raises(S.ShzError) as e:
            st.push([x[b[-2]:]], end=[0])
        assert e.value.code == S._ffi.E_STATE
        ctx.set_overlap(int(4096 * 0.75))
        k, t1, _ = st.push([x[b[-2]:]], end=[0])
        ks.append(k)
        ts.append(t1)
        st.close()
        assert np.array_equal(np.concatenate(ks), wk) and np.array_equal(np.concatenate(ts), wt)
    finally:
        ctx.set_overlap(2048)


def test_errors_and_capacity_retry(S, ctx):
    from oracle import synth
    F = S._ffi
    x = synth.synth_clip(9, 0, 44100 * 8, 4000, 3000)
    st = F.Streams(ctx, 2, 44100, 10.0, FAN)
    ref = F.Streams(ctx, 2, 44100, 10.0, FAN)
    assert st.push_raw(x, np.array([0, 100, 50], np.uint64))[0] == F.E_INVALID   # decreasing chunk_off
    half = 44100 * 4
    chunks = [x[:half], x[:half // 2]]
    rk, rt1, rho = ref.push(chunks)
    assert len(rk) > 10
    pcm = np.concatenate(chunks)
    off = np.array([0, half, half + half // 2], np.uint64)
    rc, _, _, _, need = st.push_raw(pcm, off, cap=5)
    assert rc == F.E_CAPACITY and need == len(rk)
    assert st.state(0) == {"samples": 0, "settled": 0, "pending": 0, "emitted": 0}
    rc, k, t1, ho, cnt = st.push_raw(pcm, off, cap=need)
    assert rc == F.OK and cnt == need
    assert np.array_equal(k, rk) and np.array_equal(t1, rt1) and np.array_equal(ho, rho)
    for i in range(2):
        assert st.state(i) == ref.state(i)
    # end stream 0, push to it again
    k, t1, ho = st.push([x[half:], None], end=[0])
    with pytest.raises(S.ShzError) as e:
        st.push([x[:10], None])
    assert e.value.code == F.E_STATE
    with pytest.raises(S.ShzError) as e:
        st.push([None, None], end=[0])
    assert e.value.code == F.E_STATE
    k, t1, ho = st.push([None, x[half // 2:half]])     # an ended stream given nothing is left alone
    assert ho[1] == 0
    st.reset([0])
    assert st.state(0) == {"samples": 0, "settled": 0, "pending": 0, "emitted": 0}
    k, t1, ho = st.push([x, None], end=[0])
    wk, wt, _, _ = ctx.fingerprint_batch(x, np.array([0, len(x)], np.uint64))
    assert np.array_equal(k, wk) and np.array_equal(t1, wt)
    # fan_value is limited to 64
    with pytest.raises(S.ShzError) as e:
        F.Streams(ctx, 1, 44100, 10.0, 65)
    assert e.value.code == F.E_INVALID
    st.close()
    ref.close()


def test_device_pcm_and_device_output(S, ctx):
    F = S._ffi
    n, ln = 16, 44100 * 5
    buf = ctx.synth_pcm(77, 0, n, ln, 3000, 4000)
    pcm = buf.download(np.int16, n * ln).reshape(n, ln)
    buf.free()
    st = F.Streams(ctx, n, 44100, 10.0, FAN)
    ok, ot, dp = ctx.alloc(1 << 22), ctx.alloc(1 << 22), ctx.alloc(n * 40000 * 2)
    rng = np.random.default_rng(3)
    pos = np.zeros(n, np.int64)
    got = [[] for _ in range(n)]
    while (pos < ln).any():
        steps = np.minimum(rng.integers(0, 40000, n), ln - pos)
        chunks = [pcm[i, pos[i]:pos[i] + steps[i]] for i in range(n)]
        co = np.zeros(n + 1, np.uint64)
        co[1:] = np.cumsum(steps)
        dp.upload(np.concatenate(chunks))
        pos += steps
        ends = [i for i in range(n) if pos[i] == ln and steps[i] > 0]
        rc, _, _, ho, cnt = st.push_raw(dp.ptr, co, end=ends, pcm_device=True, out_key=ok, out_t1=ot)
        assert rc == F.OK and ho[n] == cnt
        k, t1 = ok.download(np.uint32, cnt), ot.download(np.uint32, cnt)
        for i in range(n):
            got[i].append((k[ho[i]:ho[i + 1]], t1[ho[i]:ho[i + 1]]))
    st.close()
    wk, wt, ho, _ = ctx.fingerprint_batch(pcm.reshape(-1), np.arange(n + 1, dtype=np.uint64) * ln)
    for i in range(n):
        k = np.concatenate([g[0] for g in got[i]])
        t1 = np.concatenate([g[1] for g in got[i]])
        assert np.array_equal(k, wk[ho[i]:ho[i + 1]]) and np.array_equal(t1, wt[ho[i]:ho[i + 1]]), i
    for b in (ok, ot, dp):
        b.free()


def test_long_stream(S, ctx):
    """105 minutes in 10 s chunks: more than 2^17 frames."""
    n = 44100 * 60 * 105
    buf = ctx.synth_pcm(4242, 0, 1, n, 0, 8000)
    x = buf.download(np.int16, n)
    buf.free()
    assert ctx.frames_of(n) > (1 << 17)
    wk, wt, _, _ = ctx.fingerprint_batch(x, np.array([0, n], np.uint64))
    st = S._ffi.Streams(ctx, 1, 44100, 10.0, FAN)
    ks, ts = [], []
    step = 441000
    for a in range(0, n, step):
        k, t1, _ = st.push([x[a:a + step]], end=[0] if a + step >= n else None)
        ks.append(k)
        ts.append(t1)
    st.close()
    k, t1 = np.concatenate(ks), np.concatenate(ts)
    assert len(k) == len(wk) and np.array_equal(k, wk) and np.array_equal(t1, wt)


def test_fingerprint_stream_api(S, ctx):
    from oracle import synth
    x = synth.synth_clip(12, 4, 44100 * 7, 4000, 2500)
    chunks = [x[a:a + 8192] for a in range(0, len(x), 8192)]
    parts = list(S.fingerprint_stream(chunks))
    assert len(parts) == len(chunks)
    assert [h for p in parts for h in p] == S.fingerprint(x)
    assert list(S.fingerprint_stream([])) == []
    assert [h for p in S.fingerprint_stream([x[:3000]]) for h in p] == S.fingerprint(x[:3000])
    fp = S.StreamFingerprinter(2)
    a = fp.push_hex([x[:100000], x[:5000]])
    b = fp.push_hex([x[100000:], x[5000:]], end=[0, 1])
    assert a[0] + b[0] == S.fingerprint(x) == a[1] + b[1]
    fp.close()
