"""GPU: the rows stft_psd_kernel stages for fp32 peak picking, read bin by bin through shz_stft_stage_host and compared with
the exact spectrogram (oracle.np_exact.psd_exact on the CPU; for the cases of thousands of frames the device's
numpy-arithmetic kernel behind Context.stft_db(power=True), which tests/golden/psd_digests.json pins to the reference bit
for bit, plus the CPU oracle on a sample of at most 64 frames).  The fast kernel is never its own reference, except in
the two equalities 2 and 5.

For every cell of every frame:
  1. the fp64 rows against the exact power, in amplitude: |sqrt(got) - sqrt(want)| / sqrt(Pmax) <= TOL, Pmax the exact
     maximum of the frame.  A cell that is exactly 1.0 on one side stands for 0 when the other side is below 2^-100
     (stage_value maps an exact zero to 1.0, and two arithmetics need not agree on which cells are exactly zero);
  2. the fp32 rows are the fp64 rows converted, bit for bit: got32 == where(f32(got64) == 0, 1, f32(got64));
  3. the premise of shz_peak32.inc: where the exact power is >= 1.0 (0 dB, the lowest threshold of the fp32 route),
     |key(got32) - key(f32(exact))| <= 1, key = the float's bits as an integer;
  4. an all-zero frame is staged as exactly 1.0 in every bin, in both kinds;
  5. the persistent grid and the default map give bit-equal rows, and so do two runs of the same call;
  6. no cell keeps the 0xFF bytes the entry fills the staging buffer with.

TOL.  Measured on the CPU (python tests/test_gpu_stft_stage.py prints it; no GPU needed): the quantity of 1 between
psd_exact and an independent fp64 transform (np.fft.rfft of the frame times np.hanning, mlab's scaling), over every
frame this file hands to psd_exact (all frames of the small cases, the sampled frames of the large ones):
    measured maximum  = 7.886e-16
    TOL = 64 x that   = 5.047e-14
64: the fast kernel is another factorisation (radix 8.8.8.4 on the packed half-length transform, split post-pass) with
fused multiply-adds, and the published error constants of radix variants differ by small factors; a wrong pairing,
twiddle or frame is wrong by eight or more orders of magnitude beyond this.  On the same frames the rfft stand-in is 0
key steps from f32(exact) on every cell of power >= 1.0; two fp64 values within TOL of each other that straddle an fp32
rounding boundary are 1 step apart, which is what 3 allows.

The frame-to-workgroup maps (launch_stft, stft_psd_kernel): grid = WGS_PER_CU x compute units workgroups, at most one
per frame, rounded up to a multiple of 8; workgroup b of the persistent map walks the eighth b & 7 of the frames from its
frame b >> 3 in steps of grid / 8; once there are more than grid x CHUNK_FRAMES frames the default is workgroup b =
frames [32 b, 32 b + 32)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 44100
NFFT, NBINS = 4096, 2049
WGS_PER_CU = 3       # mirrors WGS_PER_CU of launch_stft (shz_extract.hip): resident workgroups per CU of the persistent grid
CHUNK_FRAMES = 32    # mirrors CHUNK_FRAMES of launch_stft: frames per workgroup of the chunked map
MEASURED = 7.886e-16  # psd_exact against the rfft stand-in, see the module docstring
TOL = 64 * MEASURED
TINY = 2.0 ** -100
T0_BINS = (0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048)   # the bins thread 0 of stft_p4_rest writes
F32, F64 = 0, 1      # SHZ_STAGE_F32, SHZ_STAGE_F64


@pytest.fixture(scope="module")
def ctx():
    import shazam_amd
    return shazam_amd.get_context(0)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _noise(seed, n, sigma=8000.0):
    return _i16(np.random.default_rng([20240, seed]).normal(0.0, sigma, n))


def _unit_noise(seed, n):
    return np.random.default_rng([20241, seed]).integers(-1, 2, n).astype(np.int16)


def _len_frames(frames, hop=2048):
    return NFFT + (frames - 1) * hop


def _signals():
    """name -> int16 clip of 3 to 6 frames at hop 2048"""
    out = {"white_noise": _noise(1, _len_frames(6))}
    n3 = _len_frames(3)
    t = np.arange(n3, dtype=np.float64)
    for b in T0_BINS:
        if b == 0:
            tone = np.full(n3, 32766.0)
        elif b == 2048:
            tone = 32766.0 * (1.0 - 2.0 * (np.arange(n3) & 1))
        else:
            tone = 32767.0 * np.cos(2.0 * np.pi * b * t / NFFT)
        out[f"cosine_bin{b}"] = _i16(tone + _unit_noise(100 + b, n3))
    n4 = _len_frames(4)
    out["sine_off_bin"] = _i16(32767.0 * np.sin(2.0 * np.pi * 300.37 * np.arange(n4) / NFFT)
                               + np.random.default_rng([20242]).normal(0.0, 3.0, n4))
    out["square_period4"] = np.where((np.arange(n3) & 2) == 0, 32767, -32768).astype(np.int16)
    out["constant_min"] = np.full(n3, -32768, np.int16)
    for name, pos in (("impulse_at_0", 0), ("impulse_at_4095", 4095), ("impulse_mid_frame", 2048)):
        x = np.zeros(n3, np.int16)
        x[pos] = 32767
        out[name] = x
    out["all_zeros"] = np.zeros(n3, np.int16)
    out["unit_noise"] = _unit_noise(7, n4)
    return out


SIGNALS = _signals()
LENGTHS = (1, 2, 4095, 4096, 4097, 6143, 6144, 6145)
ODD_LENGTHS = (4097, 6145, 4099, 8193, 5001, 3, 4096)
PERSISTENT_COUNTS = (1, 3, 7, 8, 9, 15, 16, 17, 4 * 8 + 1)


def _length_clips():
    return [_noise(200 + i, n) for i, n in enumerate(LENGTHS)]


def _one_frame_clips(count):
    """clips of one frame each; every second one a sample longer, so that half of the later ones start at odd samples"""
    return [_noise(300 + i, NFFT + (i & 1)) for i in range(count)]


def _opt_batch():
    """9 frames: 5 + 1 + 3, the second and third clip at odd samples of the packed buffer"""
    return [_noise(400, _len_frames(5) + 1), _noise(401, 1001), _noise(402, _len_frames(3))]


# ---- layout and references ----------------------------------------------------------------------------------------------
def _frames_of(n, hop):
    return 1 if n < NFFT else (n - NFFT) // hop + 1   # mlab.specgram's frame count (frames_hop in shz_extract.hip)


def _pack(clips):
    off = np.zeros(len(clips) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in clips], dtype=np.uint64)
    return (np.concatenate(clips) if clips else np.zeros(0, np.int16)), off


def _frame_offsets(off, hop):
    foff = np.zeros(len(off), np.int64)
    foff[1:] = np.cumsum([_frames_of(int(off[i + 1] - off[i]), hop) for i in range(len(off) - 1)])
    return foff


_EXACT = {}   # sha1 of a frame's samples -> its exact power row: computed once, shared by every test, never written to


def _exact_frame(x):
    from oracle import np_exact as E
    key = hashlib.sha1(x.tobytes()).digest()
    row = _EXACT.get(key)
    if row is None:
        row = E.psd_exact(x, FS, 0)[:, 0].copy()   # (a clip shorter than the window is padded with zeros there, as mlab does)
        row.flags.writeable = False
        _EXACT[key] = row
    return row


def _frame_samples(pcm, off, foff, hop, g):
    c = int(np.searchsorted(foff, g, side="right")) - 1
    start = int(off[c]) + (g - int(foff[c])) * hop
    return pcm[start:min(start + NFFT, int(off[c + 1]))]


def _exact_rows(pcm, off, hop, frame_ids=None):
    """exact power (zeros as zeros) of the frames `frame_ids` (default: all) of the batch, [len(frame_ids)][2049]"""
    foff = _frame_offsets(off, hop)
    ids = range(int(foff[-1])) if frame_ids is None else frame_ids
    return np.stack([_exact_frame(_frame_samples(pcm, off, foff, hop, int(g))) for g in ids])


def _rfft_rows(frames):
    """the independent fp64 stand-in: np.fft.rfft of the windowed frames [n][4096], mlab's scaling"""
    w = np.hanning(NFFT)
    X = np.fft.rfft(frames.astype(np.float64) * w, axis=1)
    P = X.real ** 2 + X.imag ** 2
    P[:, 1:-1] *= 2.0
    return P / FS / (w ** 2).sum()


def _key(f32):
    return np.ascontiguousarray(f32, np.float32).view(np.int32).astype(np.int64)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the assertions ----------------------------------------------------------------------------------------------------
def _amp_error(got, want, pmax):
    """assertion 1's quantity per cell.  want: the exact power with zeros as 1.0; pmax[frame]: the exact maximum of the frame
    (> 0).  A cell that is exactly 1.0 on one side stands for 0 when the other side is below 2^-100."""
    g = np.where((got == 1.0) & (want < TINY), 0.0, got)
    w = np.where((want == 1.0) & (got < TINY), 0.0, want)
    return np.abs(np.sqrt(g) - np.sqrt(w)) / np.sqrt(pmax)[:, None]


def _check_cells(got64, got32, want, pmax, label):
    """assertions 1, 2, 3, 4 and 6 on frames [n][2049]; want: exact power, zeros as 1.0; pmax: exact frame maxima, 0 for an
    all-zero frame"""
    assert got64.dtype == np.float64 and got32.dtype == np.float32 and got64.shape == got32.shape == want.shape, label
    assert not np.isnan(got64).any() and not np.isnan(got32).any(), f"{label}: a cell keeps the 0xFF fill"          # 6
    assert (got64 > 0).all() and (got32 > 0).all(), f"{label}: a staged power is positive (zero is staged as 1.0)"
    conv = got64.astype(np.float32)
    conv = np.where(conv == 0, np.float32(1.0), conv)
    assert _bits_equal(got32, conv), f"{label}: fp32 rows are not the fp64 rows converted"                         # 2
    zero = pmax == 0
    if zero.any():                                                                                                 # 4
        assert (got64[zero] == 1.0).all() and (got32[zero] == 1.0).all(), f"{label}: an all-zero frame is not all 1.0"
    live = ~zero
    if live.any():
        err = _amp_error(got64[live], want[live], pmax[live])
        worst = float(err.max())
        f, k = np.unravel_index(int(err.argmax()), err.shape)
        print(f"{label}: max amplitude error {worst:.3e} (TOL {TOL:.3e}) at live frame {f} bin {k}")
        assert worst <= TOL, f"{label}: amplitude error {worst:.3e} > {TOL:.3e} at live frame {f} bin {k}"        # 1
    loud = want >= 1.0
    if zero.any():
        loud[zero] = False   # (zeros written as 1.0)
    steps = np.abs(_key(got32) - _key(want.astype(np.float32)))[loud]
    if steps.size:                                                                                                 # 3
        print(f"{label}: fp32 key steps from the exact power: max {int(steps.max())}, {int((steps > 0).sum())} of {steps.size} cells differ")
        assert int(steps.max()) <= 1, f"{label}: fp32 key {int(steps.max())} steps from the exact power's"


def _stage_all(ctx, pcm, off, label, repeat=True):
    """both kinds under the default map, and assertion 5: the persistent grid and a second run give the same bits"""
    got64 = ctx.stft_stage(pcm, off, FS, F64)
    got32 = ctx.stft_stage(pcm, off, FS, F32)
    assert _bits_equal(got32, ctx.stft_stage(pcm, off, FS, F32, persistent=True)), f"{label}: fp32 rows differ under the persistent grid"
    assert _bits_equal(got64, ctx.stft_stage(pcm, off, FS, F64, persistent=True)), f"{label}: fp64 rows differ under the persistent grid"
    if repeat:
        assert _bits_equal(got32, ctx.stft_stage(pcm, off, FS, F32)), f"{label}: two runs of the fp32 call differ"
        assert _bits_equal(got64, ctx.stft_stage(pcm, off, FS, F64)), f"{label}: two runs of the fp64 call differ"
    return got64, got32


def _check_small(ctx, clips, label, hop=2048):
    """every frame of a small batch against the CPU oracle"""
    pcm, off = _pack(clips)
    raw = _exact_rows(pcm, off, hop)
    got64, got32 = _stage_all(ctx, pcm, off, label)
    assert got64.shape == raw.shape, (label, got64.shape, raw.shape)
    _check_cells(got64, got32, np.where(raw == 0, 1.0, raw), raw.max(axis=1), label)
    return got64, got32


def _sample_frames(n, eighths, others=(), limit=64):
    """first, last, both sides of every boundary in `eighths`, then of the boundaries in `others` (the four nearest either end
    first, then evenly spread ones) until there are `limit` frames.  A boundary is the first frame of a chunk or an eighth."""
    picked = [0, n - 1]
    others = sorted({e for e in others if 0 < e < n})
    ends = others[:4] + others[-4:]
    spread = [others[i] for i in np.linspace(0, len(others) - 1, min(len(others), limit)).astype(int)] if others else []
    for e in [e for e in eighths if 0 < e < n] + ends + spread:
        for g in (e - 1, e):
            if g not in picked and len(picked) < limit:
                picked.append(g)
    return sorted(picked)


def _check_large(ctx, clips, hop, label, others):
    """thousands of frames: every cell against the device's exact spectrogram, a sample of frames against the CPU oracle.
    The caller has set the hop."""
    pcm, off = _pack(clips)
    foff = _frame_offsets(off, hop)
    n = int(foff[-1])
    ref = np.concatenate(ctx.stft_db(pcm, off, FS, power=True), axis=1)   # [2049][n], zeros as 1.0
    assert ref.shape == (NBINS, n)
    got64, got32 = _stage_all(ctx, pcm, off, label, repeat=False)
    assert got64.shape == (n, NBINS)
    for a in range(0, n, 4096):
        w = np.ascontiguousarray(ref[:, a:a + 4096].T)
        # the exact maximum of a frame, an exact zero (staged as 1.0) not taken for a power; no other power: an all-zero frame
        pmax = np.where(w == 1.0, 0.0, w).max(axis=1)
        _check_cells(got64[a:a + 4096], got32[a:a + 4096], w, pmax, f"{label} frames {a}..")
    ids = _sample_frames(n, _eighth_edges(n), others)
    assert len(ids) <= 64
    raw = _exact_rows(pcm, off, hop, ids)
    _check_cells(got64[ids], got32[ids], np.where(raw == 0, 1.0, raw), raw.max(axis=1), f"{label} against the CPU oracle")


def _grid(ctx, frames):
    """workgroups of the persistent grid, as launch_stft sizes it"""
    g = min(int(ctx.device_info()["compute_units"]) * WGS_PER_CU, frames)
    return (g + 7) & ~7


def _eighth_edges(n):
    chunk = (n + 7) >> 3
    return [e * chunk for e in range(1, 8)]


# ---- signals, lengths, load paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SIGNALS))
def test_signal(ctx, name):
    x = SIGNALS[name]
    assert 3 <= _frames_of(len(x), 2048) <= 6
    got64, _ = _check_small(ctx, [x], name)
    if name == "all_zeros":
        assert (got64 == 1.0).all()
    if name == "unit_noise":   # powers below 1.0 everywhere: assertion 3 is vacuous here and 1 carries the case
        assert _exact_rows(*_pack([x]), 2048).max() < 1.0
    if name.startswith("cosine_bin"):
        b = int(name[len("cosine_bin"):])
        assert (got64.argmax(axis=1) == b).all(), "the tone's bin holds the maximum of every frame"


def test_signals_in_one_batch(ctx):
    """every signal as a clip of one call: a frame computed from a neighbouring clip's samples shows here"""
    _check_small(ctx, list(SIGNALS.values()), "all signals")


@pytest.mark.parametrize("i", range(len(LENGTHS)), ids=[str(n) for n in LENGTHS])
def test_clip_length_alone(ctx, i):
    _check_small(ctx, [_length_clips()[i]], f"{LENGTHS[i]} samples")


def test_clip_lengths_in_one_batch(ctx):
    """all three load paths in one launch: shorter than a window, aligned, and (behind the clips of odd length) odd starts"""
    clips = _length_clips()
    got64, got32 = _check_small(ctx, clips, "lengths batch")
    pos = 0
    for c in clips:   # a clip of a batch gets the rows it gets alone
        pcm, off = _pack([c])
        f = _frames_of(len(c), 2048)
        assert _bits_equal(got64[pos:pos + f], ctx.stft_stage(pcm, off, FS, F64))
        assert _bits_equal(got32[pos:pos + f], ctx.stft_stage(pcm, off, FS, F32))
        pos += f
    assert pos == len(got64)


def test_odd_starts(ctx):
    clips = [_noise(500 + i, n) for i, n in enumerate(ODD_LENGTHS)]
    _, off = _pack(clips)
    assert sum(int(o) & 1 for o in off[:-1]) >= 3
    _check_small(ctx, clips, "odd starts")


def test_hop_4096(ctx):
    x = _noise(600, 8192 + 3)
    ctx.set_overlap(0)
    try:
        got64, _ = _check_small(ctx, [x], "hop 4096", hop=4096)
    finally:
        ctx.set_overlap(2048)
    assert len(got64) == 2


def test_hop_1(ctx):
    """hop 1: 4,100 frames that start at even and odd samples in turn (the aligned and the unaligned load path)"""
    x = _noise(601, 8192 + 3)
    ctx.set_overlap(4095)
    try:
        assert ctx.frames_of(len(x)) == 4100
        _check_large(ctx, [x], 1, "hop 1", others=range(1, 4100))
    finally:
        ctx.set_overlap(2048)


# ---- the persistent map --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", PERSISTENT_COUNTS)
def test_persistent_counts_one_clip(ctx, frames):
    _check_small(ctx, [_noise(700, _len_frames(frames))], f"{frames} frames, one clip")


@pytest.mark.parametrize("frames", PERSISTENT_COUNTS)
def test_persistent_counts_one_frame_clips(ctx, frames):
    _check_small(ctx, _one_frame_clips(frames), f"{frames} clips of one frame")


# ---- the largest persistent count and the chunked map ---------------------------------------------------------------
HOP_L = 64


def _clips_of(frames_each, total, pcm_pool):
    """clips of `frames_each` frames at hop HOP_L (a last shorter one makes up `total`), cut from the pool; lengths vary within
    the hop so that clips start at even and odd samples.  One-frame clips also come shorter than a window."""
    counts = [frames_each] * (total // frames_each) + ([total % frames_each] if total % frames_each else [])
    clips, pos = [], 0
    for i, f in enumerate(counts):
        n = _len_frames(f, HOP_L) + (i * 7) % HOP_L
        if f == 1 and i % 3:
            n = (33, 2049)[i % 3 - 1] + i % 5
        if pos + n > len(pcm_pool):
            pos = i % 11
        clips.append(pcm_pool[pos:pos + n])
        pos += n
    assert sum(_frames_of(len(c), HOP_L) for c in clips) == total
    return clips


def _large_case(ctx, total, frames_each):
    pool = _noise(800, _len_frames(total, HOP_L) + HOP_L)
    assert len(pool) < 2_000_000
    clips = [pool[:_len_frames(total, HOP_L)]] if frames_each == 0 else _clips_of(frames_each, total, pool)
    grid = _grid(ctx, total)
    chunked = total > grid * CHUNK_FRAMES
    chunks = range(CHUNK_FRAMES, total, CHUNK_FRAMES) if chunked else ()
    ctx.set_overlap(NFFT - HOP_L)
    try:
        _check_large(ctx, clips, HOP_L, f"{total} frames in clips of {frames_each or 'all'}", chunks)
    finally:
        ctx.set_overlap(2048)


def test_largest_persistent_count(ctx):
    """grid x 32 frames: the most the default still gives to the persistent grid"""
    _large_case(ctx, _grid(ctx, 1 << 20) * CHUNK_FRAMES, 0)


@pytest.mark.parametrize("frames_each", [0, 1, 31, 32, 33], ids=["one_clip", "clips_of_1", "clips_of_31", "clips_of_32", "clips_of_33"])
@pytest.mark.parametrize("extra", [1, 33])
def test_chunked_map(ctx, extra, frames_each):
    """grid x 32 + 1 frames: the first count the default cuts into chunks of 32; + 33: with a partial last chunk.  The
    persistent grid walks the same clips in steps of grid / 8 frames, across several clips at a time."""
    _large_case(ctx, _grid(ctx, 1 << 20) * CHUNK_FRAMES + extra, frames_each)


# ---- SHZ_STFT_OPT ---------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import shazam_amd
import test_gpu_stft_stage as T
ctx = shazam_amd.get_context(0)
pcm, off = T._pack(T._opt_batch())
np.savez(sys.argv[3], f64=ctx.stft_stage(pcm, off, T.FS, T.F64), f32=ctx.stft_stage(pcm, off, T.FS, T.F32),
         f32p=ctx.stft_stage(pcm, off, T.FS, T.F32, persistent=True))
"""


def test_stft_opt_switches(ctx, tmp_path):
    """SHZ_STFT_OPT = 1 (no rotation of the special wave), 2 (one frame loop for all waves), 3 (both): the switch is read once
    per process, so each value runs in a child of its own, one after the other; the rows are the parent's bit for bit."""
    clips = _opt_batch()
    got64, got32 = _check_small(ctx, clips, "opt batch")
    assert len(got64) == 9
    here = os.path.dirname(os.path.abspath(__file__))
    for opt in (1, 2, 3):
        out = str(tmp_path / f"opt{opt}.npz")
        env = dict(os.environ, SHZ_STFT_OPT=str(opt))
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(here), here, out], env=env, timeout=120,
                           capture_output=True, text=True)
        assert r.returncode == 0, (opt, r.stderr[-2000:])
        with np.load(out) as z:
            assert _bits_equal(z["f64"], got64), f"SHZ_STFT_OPT={opt}: fp64 rows differ"
            assert _bits_equal(z["f32"], got32), f"SHZ_STFT_OPT={opt}: fp32 rows differ"
            assert _bits_equal(z["f32p"], got32), f"SHZ_STFT_OPT={opt}: fp32 rows differ under the persistent grid"


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """every refusal returns its code before anything runs and leaves the context good for the next call"""
    from shazam_amd import _ffi
    L = _ffi.lib()
    x = _noise(900, _len_frames(3))
    off = np.array([0, len(x)], np.uint64)
    want32, want64 = ctx.stft_stage(x, off, FS, F32), ctx.stft_stage(x, off, FS, F64)
    out = np.empty((3, NBINS), np.float64)
    n = C.c_uint64(77)
    p = lambda a: C.c_void_p(a.ctypes.data)
    po = lambda a: a.ctypes.data_as(_ffi.u64p)

    def call(pcm=x, co=off, nc=1, fs=FS, kind=F32, flags=0, dst=out, cap=3, h=ctx.h):
        return L.shz_stft_stage_host(h, None if pcm is None else p(pcm), None if co is None else po(co), nc, fs, kind, flags,
                                     None if dst is None else p(dst), cap, C.byref(n))

    def good():
        assert _bits_equal(ctx.stft_stage(x, off, FS, F32), want32) and _bits_equal(ctx.stft_stage(x, off, FS, F64), want64)

    def refused(code, needle, **kw):
        assert call(**kw) == code, kw
        msg = (L.shz_last_error(ctx.h) or b"").decode()
        assert needle in msg, (kw, msg)
        good()

    assert call(h=None) == _ffi.E_INVALID
    refused(_ffi.E_INVALID, "pcm is NULL", pcm=None)
    refused(_ffi.E_INVALID, "out is NULL", dst=None)
    refused(_ffi.E_INVALID, "clip_off is NULL", co=None)
    refused(_ffi.E_INVALID, "unknown kind", kind=2)
    refused(_ffi.E_INVALID, "unknown kind", kind=0xFFFFFFFF)
    refused(_ffi.E_INVALID, "unknown flag", flags=2)
    refused(_ffi.E_INVALID, "unknown flag", flags=0x80000001)
    refused(_ffi.E_INVALID, "Fs must be", fs=0)
    refused(_ffi.E_INVALID, "non-decreasing", co=np.array([0, 5000, 4999], np.uint64), nc=2)
    n.value = 77
    refused(_ffi.E_INVALID, "out holds 2", cap=2)
    assert n.value == 3   # the count the caller needs
    # more than 2^20 frames: hop 1 over 4096 + 2^20 samples
    big = np.zeros(NFFT + (1 << 20), np.int16)
    ctx.set_overlap(4095)
    try:
        assert ctx.frames_of(len(big)) == (1 << 20) + 1
        assert call(pcm=big, co=np.array([0, len(big)], np.uint64), cap=1 << 21) == _ffi.E_INVALID
        assert "2^20" in (L.shz_last_error(ctx.h) or b"").decode()
    finally:
        ctx.set_overlap(2048)
    good()
    # the workspace limit: a call that does not fit in one pass is refused, not split
    ctx.set_workspace_limit(3 * NBINS * 4)
    try:
        assert call() == _ffi.E_CAPACITY
        assert "workspace limit" in (L.shz_last_error(ctx.h) or b"").decode()
    finally:
        ctx.set_workspace_limit(0)
    good()
    # no clips: OK, no rows, nothing else looked at
    n.value = 77
    assert call(pcm=None, co=None, nc=0, dst=None, cap=0) == _ffi.OK and n.value == 0
    assert L.shz_stft_stage_host(ctx.h, None, None, 0, FS, F64, 1, None, 0, None) == _ffi.OK
    good()
    # an empty clip is a clip of one all-zero frame (mlab pads), and equal offsets are in order
    rows = ctx.stft_stage(np.zeros(0, np.int16), np.array([0, 0], np.uint64), FS, F64)
    assert rows.shape == (1, NBINS) and (rows == 1.0).all()


# ---- the measurement behind TOL (CPU only): python tests/test_gpu_stft_stage.py -------------------------------------
def _measure_reference_disagreement(compute_units=256):
    """max over every frame this file hands to psd_exact of assertion 1's quantity between psd_exact and the rfft stand-in, and
    the stand-in's largest fp32 key distance from the exact power on cells >= 1.0"""
    batches = [([x], 2048) for x in SIGNALS.values()] + [(list(SIGNALS.values()), 2048)]
    batches += [([c], 2048) for c in _length_clips()] + [(_length_clips(), 2048)]
    batches += [([_noise(500 + i, n) for i, n in enumerate(ODD_LENGTHS)], 2048), ([_noise(600, 8192 + 3)], 4096), (_opt_batch(), 2048)]
    for f in PERSISTENT_COUNTS:
        batches += [([_noise(700, _len_frames(f))], 2048), (_one_frame_clips(f), 2048)]
    sampled = [([_noise(601, 8192 + 3)], 1, range(1, 4100))]
    grid = (compute_units * WGS_PER_CU + 7) & ~7
    for total in (grid * CHUNK_FRAMES, grid * CHUNK_FRAMES + 1, grid * CHUNK_FRAMES + 33):
        for each in (0, 1, 31, 32, 33):
            if total == grid * CHUNK_FRAMES and each:
                continue
            p = _noise(800, _len_frames(total, HOP_L) + HOP_L)
            clips = [p[:_len_frames(total, HOP_L)]] if each == 0 else _clips_of(each, total, p)
            sampled.append((clips, HOP_L, range(CHUNK_FRAMES, total, CHUNK_FRAMES) if total > grid * CHUNK_FRAMES else ()))
    worst, steps = 0.0, 0
    todo = [(c, h, None) for c, h in batches] + [(c, h, e) for c, h, e in sampled]
    for clips, hop, edges in todo:
        pcm, off = _pack(clips)
        foff = _frame_offsets(off, hop)
        ids = list(range(int(foff[-1]))) if edges is None else _sample_frames(int(foff[-1]), _eighth_edges(int(foff[-1])), edges)
        raw = _exact_rows(pcm, off, hop, ids)
        fr = np.zeros((len(ids), NFFT), np.int16)
        for r, g in enumerate(ids):
            s = _frame_samples(pcm, off, foff, hop, g)
            fr[r, :len(s)] = s
        alt = _rfft_rows(fr)
        pmax = raw.max(axis=1)
        live = pmax > 0
        if live.any():
            worst = max(worst, float((np.abs(np.sqrt(alt[live]) - np.sqrt(raw[live])) / np.sqrt(pmax[live])[:, None]).max()))
        loud = raw >= 1.0
        if loud.any():
            steps = max(steps, int(np.abs(_key(alt.astype(np.float32)) - _key(raw.astype(np.float32)))[loud].max()))
    return worst, steps


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    m, s = _measure_reference_disagreement()
    print(f"psd_exact against the rfft stand-in: max amplitude disagreement {m:.3e}; 64 x = {64 * m:.3e}; "
          f"fp32 key steps of the stand-in on cells >= 1.0: {s}")
