"""GPU: every route through the extraction driver against the CPU oracle (oracle.cpu_ref.fingerprint_keys).

The driver chooses per call and per sub-batch between one read-back block and three, between the one-workgroup tail and
the general tail, and between hashes and peaks; its outputs go to host arrays or to the caller's device arrays.  The
sizes below are the thresholds in the code at 44.1 kHz, hop 2048, fan 5:

  597 frames     stage_cap = 48 * frames + 4096 <= 32768: one read-back block + the one-workgroup tail
  4096 frames    the last batch of the one-workgroup tail (4096 * 40 mask words = XT_MAX_WORDS), separate blocks
  4097 frames    the general tail
  4097 frames under a workspace limit: 4 sub-batches, the offsets accumulate through xctl_advance (each sub-batch of
                 hashes is small enough for the one-workgroup tail)
  12292 frames   3 clips (first and last alike) under a workspace limit that makes each a sub-batch of more than 4096
                 frames: the general tail's hash stage over several sub-batches

Each for hashes and peaks, host and device outputs, compared clip by clip with the oracle -- never one GPU path with
another.  The last test is the splice of clips re-run with fp64 staging on DEVICE outputs, several clips at once."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = {
    "one_block_597": (100, 197, 300),
    "small_tail_4096": (1000, 1023, 1024, 1049),
    "general_tail_4097": (1000, 1023, 1024, 1050),
    "long_clips_12292": (4097, 4098, 4097),
}
WS_FRAME = 2064 * 4   # bytes of the fp32 staging array per frame: the workspace limit counts sub-batches in these
# batch -> frames per sub-batch under the limit: every clip of the batch becomes a sub-batch of its own
WS_LIMIT_FRAMES = {"general_tail_4097": 1100, "long_clips_12292": 4200}


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    from shazam_amd import _ffi
    return S.get_context(0), _ffi


@pytest.fixture(scope="module")
def oracle():
    """frames -> (key32, t1, peak_f, peak_t) of the noise clip with that many frames; computed once, read only."""
    from oracle import cpu_ref, synth
    clips, ref = {}, {}
    for c, f in enumerate(sorted({f for fs in FRAMES.values() for f in fs})):
        clips[f] = synth.synth_clip(4242, c, 2048 * (f + 1), 0, 8000)
        ref[f] = cpu_ref.fingerprint_keys(clips[f])
    return clips, ref


def _batch(oracle, name):
    clips, ref = oracle
    xs = [clips[f] for f in FRAMES[name]]
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
    return np.concatenate(xs), off, [ref[f] for f in FRAMES[name]]


def _check(kind, a, b, offs, want, what):
    """entries a / b and the per-clip offsets against the oracle, clip by clip"""
    ia, ib = (0, 1) if kind == "hashes" else (2, 3)
    pos = 0
    assert offs[0] == 0, what
    for c, w in enumerate(want):
        n = len(w[ia])
        assert offs[c + 1] - offs[c] == n, (what, c, int(offs[c + 1] - offs[c]), n)
        assert np.array_equal(a[pos:pos + n], w[ia]) and np.array_equal(b[pos:pos + n], w[ib]), (what, c)
        pos += n
    assert pos == len(a) == len(b), what


def _device_call(ctx, _ffi, kind, x, off, cap, guard=0, fill=None):
    """one raw call with device outputs: (rc, count, offsets, A[cap + guard], B[cap + guard]) downloaded whatever rc says;
    fill: A starts as this value everywhere and B as 0xDEADBEEF"""
    L = _ffi.lib()
    da = np.uint32 if kind == "hashes" else np.uint16
    A, B = ctx.alloc((cap + guard) * da().itemsize), ctx.alloc((cap + guard) * 4)
    try:
        if fill is not None:
            A.upload(np.full(cap + guard, fill, da))
            B.upload(np.full(cap + guard, 0xDEADBEEF, np.uint32))
        offs, cnt = np.zeros(len(off), np.uint64), C.c_uint64()
        if kind == "hashes":
            rc = L.shz_fingerprint_batch(ctx.h, _ffi.ptr(x), off.ctypes.data_as(_ffi.u64p), len(off) - 1, 44100, 10.0, 5,
                                         _ffi.OUT_DEVICE, _ffi.ptr(A), _ffi.ptr(B), offs.ctypes.data_as(_ffi.u64p), cap, C.byref(cnt))
        else:
            rc = L.shz_peaks(ctx.h, _ffi.ptr(x), off.ctypes.data_as(_ffi.u64p), len(off) - 1, 44100, 10.0, _ffi.OUT_DEVICE,
                             _ffi.ptr(A), _ffi.ptr(B), offs.ctypes.data_as(_ffi.u64p), cap, C.byref(cnt))
        return rc, int(cnt.value), offs, A.download(da, cap + guard), B.download(np.uint32, cap + guard)
    finally:
        A.free()
        B.free()


def _run_routes(env, oracle, name, kind, out):
    ctx, _ffi = env
    x, off, want = _batch(oracle, name)
    if out == "host":
        if kind == "hashes":
            a, b, offs, _ = ctx.fingerprint_batch(x, off)
        else:
            a, b, offs = ctx.peaks(x, off)
    else:
        total = sum(len(w[0 if kind == "hashes" else 2]) for w in want)
        rc, cnt, offs, a, b = _device_call(ctx, _ffi, kind, x, off, total + 1000)
        assert rc == 0 and cnt == total, (name, kind, rc, cnt, total)
        a, b = a[:cnt], b[:cnt]
    _check(kind, a, b, offs, want, (name, kind, out))


@pytest.mark.parametrize("out", ["host", "device"])
@pytest.mark.parametrize("kind", ["hashes", "peaks"])
@pytest.mark.parametrize("name", [n for n in FRAMES if n not in ("long_clips_12292",)])
def test_route_matches_oracle(env, oracle, name, kind, out):
    _run_routes(env, oracle, name, kind, out)


@pytest.mark.parametrize("out", ["host", "device"])
@pytest.mark.parametrize("kind", ["hashes", "peaks"])
@pytest.mark.parametrize("name", list(WS_LIMIT_FRAMES))
def test_sub_batches_accumulate_offsets(env, oracle, name, kind, out):
    """a batch cut into one sub-batch per clip by the workspace limit; the STFT launches of the call, one per sub-batch,
    say that it was"""
    ctx = env[0]
    ctx.set_workspace_limit(WS_LIMIT_FRAMES[name] * WS_FRAME)
    ctx.set_profiling(True)
    try:
        _run_routes(env, oracle, name, kind, out)
        launches = ctx.kernel_ms()["stft_psd"][1]
        assert launches == len(FRAMES[name]) >= 3, launches
    finally:
        ctx.set_profiling(False)
        ctx.set_workspace_limit(0)


def _click(frames, amp=20000, phase=1024):
    x = np.zeros(2048 * frames, np.int16)
    x[phase::2048] = amp
    return x


def _splice_batch(which):
    from oracle import synth
    xs = [synth.synth_clip(17, c, 2048 * (40 + 5 * c), 0, 8000) for c in range(9)]
    if which == "two_tone_click_sine":   # the batch of test_several_redone_clips_with_exactly_the_final_capacity
        ties = synth.tie_inputs()
        xs[1], xs[4], xs[7] = ties["two_tone_10s"][:2048 * 80], _click(60), ties["sine_1k_10s"][:2048 * 70]
    else:                                # three clicks per hop: clips 4 and 7 are re-run in ONE call
        xs[1], xs[4], xs[7] = _click(80, 15000, 512), _click(60), _click(70, 25000, 100)
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
    return np.concatenate(xs), off


# What a call answers whose device arrays hold exactly the final count: the re-run clips are parked behind the batch's
# entries before they are moved into place, so it asks for more room -- (SHZ_E_CAPACITY, the count to provide).
# The count is the park position of the clip that found no room plus its new number of entries; a park position is the
# end of what lies in the arrays so far (the fp32 pass's total, then the clips parked earlier) rounded up to 64 entries.
# First batch: the fp32 pass leaves 7,377 entries of the other clips and at most 47 of the click clip, so the click
# clip parks at 7,424 and has 241,418 hashes: 248,842 (peaks: 1,920 + 60,357).  Second batch: clip 4 parks and fits,
# clip 7 parks at 248,832 behind it with 109,286 hashes: 358,118 (peaks: 62,272 + 27,324).
# Recorded on the commit before the driver was split into stages (MI355X); the split must not change it.
SPLICE_EXACT_CAP = {
    ("two_tone_click_sine", "hashes"): (-3, 248842), ("two_tone_click_sine", "peaks"): (-3, 62277),
    ("three_clicks", "hashes"): (-3, 358118), ("three_clicks", "peaks"): (-3, 89596),
}
# Clips re-run with fp64 staging by ONE call with device outputs.  In the first batch fp32 verification settles the
# two-tone and the sine clip, and only the click clip is re-run (the host-output test named above sees two re-runs
# because its call runs twice, the first time to learn the capacity); the second batch is there so that the splice
# walks over more than one re-run clip.
SPLICE_REDONE = {"two_tone_click_sine": 1, "three_clicks": 2}


@pytest.mark.parametrize("kind", ["hashes", "peaks"])
@pytest.mark.parametrize("which", ["two_tone_click_sine", "three_clicks"])
def test_splice_of_redone_clips_on_device_outputs(env, which, kind):
    """Clips that fp32 staging cannot settle are re-run with fp64 staging and spliced into the batch's entries.  With
    device outputs: the same arrays and offsets as with host outputs, nothing written behind the capacity."""
    ctx, _ffi = env
    x, off = _splice_batch(which)
    s0 = ctx.extract_stats()
    if kind == "hashes":
        a_ref, b_ref, o_ref, _ = ctx.fingerprint_batch(x, off)
    else:
        a_ref, b_ref, o_ref = ctx.peaks(x, off)
    n_ref = len(a_ref)
    fill = 0xDEADBEEF if kind == "hashes" else 0xBEEF
    s1 = ctx.extract_stats()
    roomy = 2 * n_ref + 4096   # (room for the parked clips)
    rc, cnt, offs, a, b = _device_call(ctx, _ffi, kind, x, off, roomy, guard=64, fill=fill)
    assert rc == 0 and cnt == n_ref, (rc, cnt, n_ref)
    s2 = ctx.extract_stats()
    print("re-run clips: host call(s)", s1["f64_clips"] - s0["f64_clips"], "device call", s2["f64_clips"] - s1["f64_clips"])
    assert s2["f64_clips"] - s0["f64_clips"] >= 2                      # clips were re-run and spliced
    assert s2["f64_clips"] - s1["f64_clips"] == SPLICE_REDONE[which]   # ... this many by the device call alone
    assert np.array_equal(a[:cnt], a_ref) and np.array_equal(b[:cnt], b_ref) and np.array_equal(offs, o_ref)
    assert np.all(a[roomy:] == fill) and np.all(b[roomy:] == 0xDEADBEEF)
    # capacity == the count
    rc, cnt, offs, a, b = _device_call(ctx, _ffi, kind, x, off, n_ref, guard=64, fill=fill)
    print("exact capacity:", which, kind, "n_ref", n_ref, "rc", rc, "count", cnt)
    assert np.all(a[n_ref:] == fill) and np.all(b[n_ref:] == 0xDEADBEEF)
    assert (rc, cnt) == SPLICE_EXACT_CAP[which, kind]
