"""GPU: stft_psd_kernel's walk over the clip tables.  The kernel keeps the clip of the frame it loaded last in scalar
registers (first frame, end frame, length, first sample) and reads the tables again only where a frame crosses into a later
clip; a workgroup of the chunked map walks 32 consecutive frames, one of the persistent map every (grid / 8)-th frame of
an eighth.  A frame taken from the wrong clip, or from the right clip at a stale offset, is wrong in every bin, so the
batches here put clip boundaries at every position of a 32-frame chunk and on its edges:

  * clips of 1, 2, 3, 31, 32, 33, 64 and 65 frames in four orders;
  * a run of 40 one-frame clips (several boundaries in one chunk, consecutive frames that all change clip);
  * clips shorter than one window (one zero-padded frame) between full ones;
  * clips of odd length, so that later clips start at odd samples of the packed buffer (the unaligned load shape);
  * filler in front and behind so that the batch takes the chunked map and its last chunk is partly empty.

Checked, with the rules of tests/test_gpu_stft_stage.py (TOL and its derivation are stated there):
  1. fp64 rows against the exact power (oracle.np_exact.psd_exact) in amplitude: |sqrt(got) - sqrt(want)| / sqrt(Pmax) <= TOL;
  2. fp32 rows are the fp64 rows converted, bit for bit (a zero after conversion staged as 1.0);
  3. where the exact power is >= 1.0 the fp32 key is at most one step from the key of the exact power rounded to fp32;
  4. the persistent grid gives the rows of the default map bit for bit;
  5. hashes and peaks of the default path equal those of fp64 staging (shz_set_stage_f64(1)) and of oracle.cpu_ref, in one
     pass, under a workspace limit that cuts the batch into sub-batches, and in a batch large enough for the chunked map.
The large cases compare every row with the device's numpy-arithmetic spectrogram (Context.stft_db(power=True), pinned to
the reference by tests/golden/psd_digests.json) and the first and last frame of every structured clip with the CPU oracle."""
import hashlib
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 44100
NFFT, NBINS, HOP = 4096, 2049, 2048
HOP_L = 64               # the hop of the rows test on the chunked map: 25,000 frames in 1.7 M samples
WGS_PER_CU = 3           # mirrors launch_stft (shz_extract.hip): resident workgroups per CU of the persistent grid
CHUNK_FRAMES = 32        # mirrors launch_stft: frames per workgroup of the chunked map
TOL = 64 * 7.886e-16     # tests/test_gpu_stft_stage.py: 64 x the measured disagreement of two exact fp64 transforms
TINY = 2.0 ** -100
F32, F64 = 0, 1          # SHZ_STAGE_F32, SHZ_STAGE_F64
SIZES = (1, 2, 3, 31, 32, 33, 64, 65)
ORDERS = (SIZES, SIZES[::-1], SIZES[3:] + SIZES[:3], (65, 1, 64, 2, 33, 3, 32, 31))
SHORT = (33, 2049, 4095, 1, 3000)   # samples: shorter than a window, one zero-padded frame each
FILL_SAMPLES = HOP * 643 + NFFT     # a 30 s filler clip: 644 frames


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    ctx = S.get_context(0)
    return types.SimpleNamespace(S=S, ctx=ctx, info=ctx.device_info())


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _noise(seed, n, sigma=8000.0):
    x = np.random.default_rng([20250, seed]).normal(0.0, sigma, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _frames_of(n, hop):
    return 1 if n < NFFT else (n - NFFT) // hop + 1


def _structured(hop):
    """[(clip, frames)]: the clips of the module docstring at `hop`.  A clip's samples depend on its frame count alone (the
    exact rows of a size are computed once); the extra samples behind its last frame make later clips start at odd samples."""
    pool = _noise(1, NFFT + 64 * hop + 128)
    out = []
    for o, order in enumerate(ORDERS):
        for i, f in enumerate(order):
            extra = min((o + i) % 3, hop - 1)
            out.append(pool[f:f + NFFT + (f - 1) * hop + extra])
    ones = _noise(2, 40 * 7 + NFFT + 1)
    out += [ones[7 * i:7 * i + NFFT + min(i & 1, hop - 1)] for i in range(40)]
    for i, n in enumerate(SHORT):
        out.append(pool[100 + i:100 + i + n])
        f = (3, 2, 33, 1, 31)[i]
        out.append(pool[f:f + NFFT + (f - 1) * hop])
    return [(np.ascontiguousarray(c), _frames_of(len(c), hop)) for c in out]


def _pack(clips):
    off = np.zeros(len(clips) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in clips], dtype=np.uint64)
    return np.concatenate(clips), off


def _foff(off, hop):
    f = np.zeros(len(off), np.int64)
    f[1:] = np.cumsum([_frames_of(int(off[i + 1] - off[i]), hop) for i in range(len(off) - 1)])
    return f


def _grid(info, frames=1 << 20):
    g = min(int(info["compute_units"]) * WGS_PER_CU, frames)
    return (g + 7) & ~7


# ---- references ---------------------------------------------------------------------------------------------------------
_EXACT = {}   # sha1 of a frame's samples -> its exact power row: computed once, shared, never written to


def _exact_frame(x):
    from oracle import np_exact as E
    key = hashlib.sha1(x.tobytes()).digest()
    row = _EXACT.get(key)
    if row is None:
        row = E.psd_exact(x, FS, 0)[:, 0].copy()   # (a clip shorter than the window is padded with zeros there, as mlab does)
        row.flags.writeable = False
        _EXACT[key] = row
    return row


def _exact_rows(pcm, off, hop, ids):
    foff = _foff(off, hop)
    rows = []
    for g in ids:
        c = int(np.searchsorted(foff, g, side="right")) - 1
        start = int(off[c]) + (int(g) - int(foff[c])) * hop
        rows.append(_exact_frame(pcm[start:min(start + NFFT, int(off[c + 1]))]))
    return np.stack(rows)


_REFS = {}    # sha1 of a clip -> cpu_ref's (key32, t1, peak_f, peak_t)


def _cpu_ref(x):
    from oracle import cpu_ref as O
    key = hashlib.sha1(x.tobytes()).digest()
    if key not in _REFS:
        _REFS[key] = O.fingerprint_keys(x)
    return _REFS[key]


def _key(f32):
    return np.ascontiguousarray(f32, np.float32).view(np.int32).astype(np.int64)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_rows(got64, got32, want, label):
    """rules 1-3 on frames [n][2049]; want: the exact power, zeros as zeros"""
    assert got64.shape == got32.shape == want.shape, (label, got64.shape, got32.shape, want.shape)
    assert not np.isnan(got64).any() and not np.isnan(got32).any(), f"{label}: a cell was never written"
    conv = got64.astype(np.float32)
    conv = np.where(conv == 0, np.float32(1.0), conv)
    assert _bits_equal(got32, conv), f"{label}: fp32 rows are not the fp64 rows converted"                       # 2
    pmax = want.max(axis=1)
    zero = pmax == 0     # an all-zero frame (a clip of one zero sample) is staged as exactly 1.0 in every bin
    if zero.any():
        assert (got64[zero] == 1.0).all() and (got32[zero] == 1.0).all(), f"{label}: an all-zero frame is not all 1.0"
    live = ~zero
    w1 = np.where(want == 0, 1.0, want)
    g = np.where((got64 == 1.0) & (w1 < TINY), 0.0, got64)[live]
    w = np.where((w1 == 1.0) & (got64 < TINY), 0.0, w1)[live]
    err = np.abs(np.sqrt(g) - np.sqrt(w)) / np.sqrt(pmax[live])[:, None]
    worst = float(err.max())
    f, k = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{label}: max amplitude error {worst:.3e} (TOL {TOL:.3e}) at live frame {f} bin {k}")
    assert worst <= TOL, f"{label}: amplitude error {worst:.3e} > {TOL:.3e} at live frame {f} bin {k}"          # 1
    loud = (want >= 1.0) & live[:, None]
    steps = np.abs(_key(got32) - _key(w1.astype(np.float32)))[loud]
    if steps.size:
        print(f"{label}: fp32 key steps from the exact power: max {int(steps.max())}")
        assert int(steps.max()) <= 1, f"{label}: fp32 key {int(steps.max())} steps from the exact power's"      # 3


def _check_rows_device(got64, got32, ref, label):
    """rules 1-3 against the device's exact spectrogram `ref` [n][2049] (zeros as 1.0), 4,096 frames at a time"""
    for a in range(0, len(ref), 4096):
        w = ref[a:a + 4096]
        _check_rows(got64[a:a + 4096], got32[a:a + 4096], np.where(w == 1.0, 0.0, w), f"{label} frames {a}..")


def _extract(ctx, pcm, off, f64, pcm_device=False, peaks=True):
    ctx.set_stage_f64(f64)
    try:
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, off, pcm_device=pcm_device)
        pf, pt, po = ctx.peaks(pcm, off, pcm_device=pcm_device) if peaks else (None, None, None)
    finally:
        ctx.set_stage_f64(False)
    return k, t1, ho, pf, pt, po


def _assert_clip(out, i, x, what):
    k, t1, ho, pf, pt, po = out
    rk, rt1, rf, rt = _cpu_ref(x)
    a, b = int(ho[i]), int(ho[i + 1])
    assert np.array_equal(k[a:b], rk) and np.array_equal(t1[a:b], rt1), f"{what}: hashes differ from cpu_ref"
    if pf is not None:
        a, b = int(po[i]), int(po[i + 1])
        assert np.array_equal(pf[a:b], rf) and np.array_equal(pt[a:b], rt), f"{what}: peaks differ from cpu_ref"


def _assert_same(u, v, what):
    for a, b in zip(u, v):
        assert (a is None and b is None) or np.array_equal(a, b), what


# ---- the structured batch alone: the persistent grid, one pass and sub-batches ------------------------------------------
def test_structured_batch_rows(env):
    """1,000 frames: the default map IS the persistent grid here (every workgroup strides over the frames and most of its
    frames change clip); every frame against the CPU oracle"""
    ctx = env.ctx
    clips = _structured(HOP)
    pcm, off = _pack([c for c, _ in clips])
    assert sum(int(o) & 1 for o in off[:-1]) >= 20, "clips at odd samples of the packed buffer"
    n = int(_foff(off, HOP)[-1])
    assert n == sum(f for _, f in clips) and n <= _grid(env.info) * CHUNK_FRAMES
    got64, got32 = ctx.stft_stage(pcm, off, FS, F64), ctx.stft_stage(pcm, off, FS, F32)
    assert _bits_equal(got32, ctx.stft_stage(pcm, off, FS, F32, persistent=True))                                 # 4
    assert _bits_equal(got64, ctx.stft_stage(pcm, off, FS, F64, persistent=True))
    _check_rows(got64, got32, _exact_rows(pcm, off, HOP, range(n)), "structured batch")


def test_structured_batch_hashes_one_pass_and_sub_batches(env):
    ctx = env.ctx
    clips = [c for c, _ in _structured(HOP)]
    pcm, off = _pack(clips)
    one32, one64 = _extract(ctx, pcm, off, False), _extract(ctx, pcm, off, True)
    _assert_same(one32, one64, "fp32 staging against fp64 staging")
    for i, x in enumerate(clips):
        _assert_clip(one32, i, x, f"clip {i} ({len(x)} samples)")
    # a workspace limit of 130 fp64 rows (259 fp32 rows): at least eight sub-batches, cut at other clips in the two modes
    ctx.set_workspace_limit(130 * 2056 * 8)
    try:
        sub32, sub64 = _extract(ctx, pcm, off, False), _extract(ctx, pcm, off, True)
    finally:
        ctx.set_workspace_limit(0)
    _assert_same(sub32, one32, "fp32 staging in sub-batches")
    _assert_same(sub64, one32, "fp64 staging in sub-batches")


# ---- the chunked map ------------------------------------------------------------------------------------------------------
def _chunked_layout(info, hop):
    """filler of 1,005 frames, the structured clips, filler up to grid x 32 + 45 frames: the first count that takes the
    chunked map plus a whole chunk and 13 frames of a last one"""
    clips = _structured(hop)
    total = _grid(info) * CHUNK_FRAMES + CHUNK_FRAMES + 13
    rest = total - 1005 - sum(f for _, f in clips)
    assert rest > 0
    return clips, 1005, rest, total


def test_chunked_map_rows(env):
    """grid x 32 + 45 frames at hop 64: workgroup b takes frames [32 b, 32 b + 32), the structured clips start at frame
    1,005 = 31 x 32 + 13, the last workgroup has 13 frames"""
    ctx = env.ctx
    st, fa, fb, total = _chunked_layout(env.info, HOP_L)
    pool = _noise(3, NFFT + (max(fa, fb) - 1) * HOP_L + 3)
    clips = [pool[:NFFT + (fa - 1) * HOP_L + 1]] + [c for c, _ in st] + [pool[2:2 + NFFT + (fb - 1) * HOP_L]]
    pcm, off = _pack(clips)
    ctx.set_overlap(NFFT - HOP_L)
    try:
        foff = _foff(off, HOP_L)
        assert int(foff[-1]) == total and total > _grid(env.info) * CHUNK_FRAMES and total % CHUNK_FRAMES == 13
        ref = np.ascontiguousarray(np.concatenate(ctx.stft_db(pcm, off, FS, power=True), axis=1).T)   # [total][2049], zeros as 1.0
        got64, got32 = ctx.stft_stage(pcm, off, FS, F64), ctx.stft_stage(pcm, off, FS, F32)
        assert _bits_equal(got32, ctx.stft_stage(pcm, off, FS, F32, persistent=True))                             # 4
        assert _bits_equal(got64, ctx.stft_stage(pcm, off, FS, F64, persistent=True))
    finally:
        ctx.set_overlap(NFFT - HOP)
    _check_rows_device(got64, got32, ref, "chunked map")
    # every position of a chunk is a clip's first frame somewhere
    firsts = {int(f) % CHUNK_FRAMES for f in foff[1:-1]}
    assert firsts == set(range(CHUNK_FRAMES)), sorted(set(range(CHUNK_FRAMES)) - firsts)
    ids = sorted({int(g) for c in range(1, len(clips) - 1) for g in (foff[c], foff[c + 1] - 1)} | {0, total - 1})
    _check_rows(got64[ids], got32[ids], _exact_rows(pcm, off, HOP_L, ids), "chunked map against the CPU oracle")


def test_chunked_map_hashes(env):
    """The same layout at the default hop, the PCM on the device (one extraction pass over the whole batch): filler clips
    of 644 frames made on the device, the structured clips between them at an odd sample offset"""
    ctx = env.ctx
    st = [c for c, _ in _structured(HOP)]
    st_frames = sum(_frames_of(len(c), HOP) for c in st)
    need = _grid(env.info) * CHUNK_FRAMES + CHUNK_FRAMES + 13 - st_frames
    n_fill = -(-need // 644)
    k1 = 2
    off = [i * FILL_SAMPLES for i in range(k1)] + [k1 * FILL_SAMPLES + 1]   # (one more sample: it belongs to the last filler clip)
    for x in st:
        off.append(off[-1] + len(x))
    pad = -off[-1] % 64
    off[-1] += pad                                                          # (zeros behind the last structured clip's last frame)
    start_post = off[-1]
    off += [start_post + (i + 1) * FILL_SAMPLES for i in range(n_fill - k1)]
    off = np.array(off, np.uint64)
    frames = sum(ctx.frames_of(int(off[i + 1] - off[i])) for i in range(len(off) - 1))
    assert frames == n_fill * 644 + st_frames and frames > _grid(env.info) * CHUNK_FRAMES
    assert frames <= min(1 << 20, (env.info["hbm_bytes"] // 4) // (2056 * 8)), "one sub-batch"
    ctx.set_workspace_limit(0)
    buf = ctx.alloc(int(off[-1]) * 2)
    try:
        at = lambda sample: types.SimpleNamespace(ptr=buf.ptr + 2 * int(sample))
        ctx.synth_pcm(9191, 0, k1, FILL_SAMPLES, 0, 8000, out=at(0))
        ctx.synth_pcm(9191, k1, n_fill - k1, FILL_SAMPLES, 0, 8000, out=at(start_post))
        last = st[-1]
        mid = np.concatenate([np.zeros(1, np.int16)] + st + [np.zeros(pad, np.int16)])
        buf.upload(mid, 2 * k1 * FILL_SAMPLES)
        ctx.sync()
        out32 = _extract(ctx, buf, off, False, pcm_device=True)
        out64 = _extract(ctx, buf, off, True, pcm_device=True)
    finally:
        buf.free()
    _assert_same(out32, out64, "fp32 staging against fp64 staging")
    for i, x in enumerate(st):
        if i == len(st) - 1:
            x = np.concatenate([last, np.zeros(pad, np.int16)])
            assert _frames_of(len(x), HOP) == _frames_of(len(last), HOP)
        _assert_clip(out32, k1 + i, x, f"structured clip {i} ({len(x)} samples)")
    assert int(out32[2][k1]) > 0 and int(out32[2][-1]) > int(out32[2][k1 + len(st)])
