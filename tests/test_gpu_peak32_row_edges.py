"""GPU: the rows peak_pick32 loads at the edges of a segment.  The kernel issues the seven row loads of every group
without a branch: a row past the last one of its segment is a re-read of the last row, a lane outside the spectrum reads
column 0, and both are replaced by -inf where the group is consumed.  A re-read row that is NOT replaced shows as a lost
peak (the edge row's maximum is no longer alone in its window) or as a duplicated one, so every clip length that puts
the segment's end at another place of the 7-row groups and the 21-row blocks is here:

  * every length from 1 to 45 frames (every residue mod 7 and mod 21; segments shorter than the 10-frame halo);
  * 251, 252, 253, 272, 273, 274 frames (the 252-frame segment edge, plus and minus the halo) and 671, 672, 673 (the long one);
  * seeded noise; tones that only the LAST frame of a clip holds, and tones that only the FIRST holds, in bins 5, 107, 1024
    and 2043 (the first and the last frequency slab, a slab edge, the middle): the maxima of the windows that
    reach the clip's edge lie in the edge row;
  * oracle.tie_geometry tiles tied across two of the last ten frames of a clip (exact, and one count apart, the second
    copy in the very last frame); their seeds top bins 0..9 and 2039..2048.

Peaks and hashes of the default path (fp32 staging) must equal fp64 staging (shz_set_stage_f64(1)) and the CPU statement
(oracle.cpu_ref; for the tie clips tie_geometry.reference, which is cpu_ref on the exact spectrogram), bit for bit and
in order, in batches of all three segment regimes (42-, 252- and 672-frame segments).  Which regime a batch is in cannot
be read back from the library: `seg_regime` restates upload_meta's rule and the test fails if a batch lands elsewhere."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NFFT, HOP = 4096, 2048
FILL_FRAMES = 644
FILL_SAMPLES = HOP * (FILL_FRAMES - 1) + NFFT
SHORT = tuple(range(1, 46))
MIDDLE = (251, 252, 253, 272, 273, 274)
LONG = (671, 672, 673)
TONE_BINS = (5, 107, 1024, 2043)
EDGE_LENGTHS = (1, 2, 7, 12, 21, 30, 45, 252, 273, 672)   # clips with tones in their first and in their last frame


def seg_regime(frames: int, compute_units: int, f64: bool) -> int:
    """upload_meta (csrc/shz_extract.hip): the segment length of ONE sub-batch of `frames` frames.  fp32 staging: 20 slabs,
    6 workgroups per CU; fp64 staging: 9 slabs, 3 per CU."""
    n_slabs, wg_per_cu = (9, 3) if f64 else (20, 6)
    slots = compute_units * wg_per_cu
    if frames * n_slabs // 672 >= 4 * slots:
        return 672
    if frames * n_slabs // 252 * 8 < slots:
        return 42
    return 252


def _len(frames, extra=0):
    return NFFT + (frames - 1) * HOP + extra


def _edge_tones(frames, first, seed):
    """noise (amplitude 1,500) with tones of 5,000 counts in 2,048 samples that only the clip's first / last frame holds"""
    from oracle import synth
    x = synth.synth_clip(seed, frames, _len(frames), 0, 1500).astype(np.float64)
    n = np.arange(HOP, dtype=np.float64)
    tone = sum(5000.0 * np.cos(2.0 * np.pi * b * n / NFFT + 0.3 * i) for i, b in enumerate(TONE_BINS))
    if frames == 1:
        x[:HOP] += tone                      # (one frame: first and last)
    elif first:
        x[:HOP] += tone
    else:
        x[-HOP:] += tone
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def env():
    """every clip and its reference, made once and shared (read-only)"""
    import shazam_amd as S
    from shazam_amd import _ffi
    from oracle import cpu_ref as O, synth, tie_geometry as G
    ctx = S.get_context(0)
    fused = _ffi.numpy_product_is_fused()
    clips = {}
    for f in SHORT + MIDDLE + LONG:
        clips[f"noise{f}"] = synth.synth_clip(606, f, _len(f, f % 2), 0, 8000)
    for f in EDGE_LENGTHS:
        clips[f"last{f}"] = _edge_tones(f, False, 707)
        clips[f"first{f}"] = _edge_tones(f, True, 708)
    # ties across two of the last ten frames: frames 22 and 27 of 30 (equal copies), frames 25 and 29 of 30 (one count on the
    # copy in the last frame), and the same in a clip of 273 frames (the last frames of a second 252-frame segment)
    ties = {"tie_exact30": G.build_clip(30, [(22, G.EDGE_SEEDS[0], ("exact",), [27])], bg_clip=1),
            "tie_step30": G.build_clip(30, [(25, G.EDGE_SEEDS[1], ("step", 240), [29])], bg_clip=2),
            "tie_step273": G.build_clip(273, [(266, G.EDGE_SEEDS[2], ("step", 200), [272])], bg_clip=3, extra=0)}
    refs = {}
    for name, x in clips.items():
        k, t1, f, t = O.fingerprint_keys(x)
        refs[name] = (f, t, k, t1)
    for name, x in ties.items():
        refs[name] = G.reference(x, fused=fused)[:4]
        clips[name] = x
    for x in clips.values():
        x.flags.writeable = False
    return types.SimpleNamespace(ctx=ctx, clips=clips, refs=refs, info=ctx.device_info(), O=O)


def test_the_inputs_hold_what_they_are_for(env):
    """counted on the references alone: the edge rows hold peaks in the first and in the last slab, the tie clips hold tied
    peaks in their last ten frames"""
    for f in EDGE_LENGTHS:
        for kind, row in (("last", f - 1), ("first", 0)):
            pf, pt = env.refs[f"{kind}{f}"][:2]
            at = set(pf[pt == row].tolist())
            assert at & set(range(0, 11)) and at & set(range(2038, 2049)), (kind, f, sorted(at))
    pf, pt = env.refs["tie_exact30"][:2]
    both = set(pf[pt == 22].tolist()) & set(pf[pt == 27].tolist())
    assert len(both) >= 20 and min(both) < 10 and max(both) > 2038, sorted(both)
    for name, last in (("tie_step30", 29), ("tie_step273", 272)):
        pf, pt = env.refs[name][:2]
        assert (pt == last).sum() >= 10, name


def _extract(ctx, pcm, off, f64, pcm_device=False):
    ctx.set_stage_f64(f64)
    try:
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, off, pcm_device=pcm_device)
        pf, pt, po = ctx.peaks(pcm, off, pcm_device=pcm_device)
    finally:
        ctx.set_stage_f64(False)
    return k, t1, ho, pf, pt, po


def _assert_clip(out, i, ref, what):
    k, t1, ho, pf, pt, po = out
    rf, rt, rk, rt1 = ref
    a, b = int(po[i]), int(po[i + 1])
    got, want = list(zip(pt[a:b].tolist(), pf[a:b].tolist())), list(zip(rt.tolist(), rf.tolist()))
    if got != want:
        only_dev, only_ref = sorted(set(got) - set(want)), sorted(set(want) - set(got))
        raise AssertionError(f"{what}: peaks differ: {len(got)} on the device, {len(want)} in the reference; (frame, bin) "
                             f"only on the device {only_dev[:8]}, only in the reference {only_ref[:8]}, "
                             f"twice on the device {len(got) - len(set(got))}")
    a, b = int(ho[i]), int(ho[i + 1])
    assert np.array_equal(k[a:b], rk) and np.array_equal(t1[a:b], rt1), f"{what}: hashes differ"


def _run_batch(env, names, regime, n_fill=0):
    """the clips `names`, each at the sample offset the lengths in front of it give (odd ones among them), behind n_fill / 2
    and in front of n_fill - n_fill / 2 filler clips made on the device; the PCM lives on the device, so the call is one
    extraction pass over the whole batch"""
    ctx, cus = env.ctx, env.info["compute_units"]
    k1 = n_fill // 2
    xs = [env.clips[n] for n in names]
    off = [i * FILL_SAMPLES for i in range(k1 + 1)]
    for x in xs:
        off.append(off[-1] + len(x))
    pad = -off[-1] % 64   # zeros up to a multiple of 64 samples: they belong to the last clip and lie behind its last frame
    assert ctx.frames_of(len(xs[-1]) + pad) == ctx.frames_of(len(xs[-1]))
    off[-1] += pad
    start_post = off[-1]
    off += [start_post + (i + 1) * FILL_SAMPLES for i in range(n_fill - k1)]
    off = np.array(off, np.uint64)
    assert sum(int(o) & 1 for o in off[k1:k1 + len(xs)]) >= min(len(xs) // 4, 3), "some clips start at odd samples"
    frames = sum(ctx.frames_of(int(off[i + 1] - off[i])) for i in range(len(off) - 1))
    for f64 in (False, True):
        assert seg_regime(frames, cus, f64) == regime, (frames, cus, f64, regime)
    assert frames <= min(1 << 20, (env.info["hbm_bytes"] // 4) // (2056 * 8)), "one sub-batch"
    ctx.set_workspace_limit(0)
    buf = ctx.alloc(int(off[-1]) * 2)
    try:
        at = lambda sample: types.SimpleNamespace(ptr=buf.ptr + 2 * int(sample))
        if k1:
            ctx.synth_pcm(9292, 0, k1, FILL_SAMPLES, 0, 8000, out=at(0))
        if n_fill - k1:
            ctx.synth_pcm(9292, k1, n_fill - k1, FILL_SAMPLES, 0, 8000, out=at(start_post))
        buf.upload(np.concatenate(xs + [np.zeros(pad, np.int16)]), 2 * k1 * FILL_SAMPLES)
        ctx.sync()
        s0 = ctx.extract_stats()
        out32 = _extract(ctx, buf, off, False, pcm_device=True)
        s1 = ctx.extract_stats()
        out64 = _extract(ctx, buf, off, True, pcm_device=True)
    finally:
        buf.free()
    # the fp32 picker itself answered: no whole pass and no clip was redone with fp64 staging
    assert s1["f64_passes"] == s0["f64_passes"] and s1["f64_clips"] == s0["f64_clips"], (s0, s1)
    for i, n in enumerate(names):
        _assert_clip(out32, k1 + i, env.refs[n], (n, regime, "fp32 staging"))
        _assert_clip(out64, k1 + i, env.refs[n], (n, regime, "fp64 staging"))
    for u, v in zip(out32, out64):   # (the filler is not compared with the CPU; the two staging modes must agree on it)
        assert np.array_equal(u, v), regime


def _fill_for(env, names, want):
    """the smallest even number of filler clips that puts the batch into the `want` regime in both staging modes (+ 8 for
    the long regime, as a margin)"""
    own = sum(env.ctx.frames_of(len(env.clips[n])) for n in names)
    cus = env.info["compute_units"]
    for n in range(0, 4000, 2):
        f = own + n * FILL_FRAMES
        if seg_regime(f, cus, False) == want and seg_regime(f, cus, True) == want:
            return n + (8 if want == 672 else 0)
    pytest.fail(f"no batch size reaches {want}-frame segments in both staging modes on {cus} compute units")


def _edge_names(lengths):
    return [f"{k}{f}" for f in EDGE_LENGTHS if f in lengths for k in ("last", "first")]


def test_short_segments(env):
    """1 to 45 frames, segments of 42: clips of 43 to 45 frames have a second segment of 1 to 3 frames inside the halo of
    the first"""
    names = [f"noise{f}" for f in SHORT] + _edge_names(SHORT) + ["tie_exact30", "tie_step30"]
    _run_batch(env, names, 42, _fill_for(env, names, 42))


def test_middle_segments(env):
    """everything in one batch of 252-frame segments: 251 to 274 frames end a segment, or begin a second one, within the
    halo; 671 to 673 frames are two segments and 167 to 169 frames of a third"""
    names = list(env.clips)
    _run_batch(env, names, 252, _fill_for(env, names, 252))


def test_long_segments(env):
    """a batch of the benchmark's size or larger, segments of 672: 671 to 673 frames end the segment, or begin a second one,
    within the halo"""
    names = [f"noise{f}" for f in MIDDLE + LONG] + _edge_names((252, 273, 672)) + ["tie_step273"] + [f"noise{f}" for f in (1, 9, 10, 11, 45)]
    _run_batch(env, names, 672, _fill_for(env, names, 672))
