"""GPU: the block rule of peak_pick32 (csrc/shz_peak32.inc) on ties BUILT from PCM and placed at every edge of its blocks.

The kernel gives the 21x21 window test only to cells that come within two fp32 key steps of the maximum of a block that
their window contains whole: the 7 rows of the cell's time block (blocks are counted from the segment's first frame,
and 42, 252 and 672 are multiples of 7, so a frame's place in its block is t mod 7) by the 21 columns round the cell, and
the time block before (rows 0..3 of a block) or after (rows 3..6).  A decided row takes its window from the rows of five
blocks.  One wave owns a slab of 44 bins (47 slabs); the seams are at the multiples of 44.  A wrong block rule loses a
tied cell (the partner's block hid it) or keeps a beaten one, so the inputs are near-ties whose two or three cells lie

  * in one time block, in neighbouring blocks with the first cell at every place t mod 7, two blocks apart;
  * 1 to 11 frames apart (at 11 the cells do not see each other), equal or one count apart (0..4 key steps);
  * three in a row over three blocks;
  * in a clip's first and last ten frames, and on either side of a segment boundary (frames 42, 252, 672);
  * in ONE row, 2..12 bins apart: the zero-odd-samples tile of oracle.tie_geometry (bins 1024 - j and 1024 + j, j = 1..6),
    and the same idea with every eighth sample kept (`_tile8`): the spectrum repeats every 512 bins and is symmetric about
    every multiple of 256, so one frame holds the pair 256 m - j, 256 m + j for m = 1, 3, 5, 7: inside a slab for most of
    them, and round bin 1280 on either side of the slab seam 1276 from j = 5 on (at j = 6, 12 bins, the two cells no
    longer see each other: both are peaks);
  * tones in bins 0..10 and 2038..2048 that only a clip's first or last frame holds.

Every clip is judged by oracle.tie_geometry.reference (here with the frames' exact spectra cached across clips: the clips
share one background), peaks and hashes bit for bit and in order, with fp32 and with fp64 staging, in one batch of each
segment regime (42, 252, 672: `seg_regime` restates upload_meta's rule, and the test fails if a batch lands elsewhere).
The first test asserts, on the CPU alone, that each clip holds the tie it is meant to hold."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NFFT, HOP, NBINS = 4096, 2048, 2049
BH, OW = 7, 44                  # rows of a time block, bins of a slab (shz_peak32.inc: P32_BH, P32_OW)
FILL_FRAMES = 644
FILL_SAMPLES = HOP * (FILL_FRAMES - 1) + NFFT
CLIP_FRAMES = 64
TONE_BINS = (2, 10, 2038, 2046)
# symmetric tiles (zero odd samples) that top bins 1004..1044 at 1024 +- j: j -> (seed, odd sample of the one count)
SYM = {1: (7017, 121), 2: (7001, 41), 3: (7019, 41), 4: (7088, 61), 5: (7083, 41), 6: (7048, 41)}
# tiles with every eighth sample kept that top bins 236..276 at 256 +- j (and so 1260..1300 at 1280 +- j): j -> seed
TILE8 = {1: 11016, 2: 11005, 3: 11001, 4: 11018, 5: 11003, 6: 11021}
TILE8_AMP = 16000               # an eighth of the samples: 9 dB less power than a full tile of the same amplitude
C8 = 1280                       # the centre 256 m next to a slab seam: 1276 = 29 * 44


def seg_regime(frames: int, compute_units: int, f64: bool) -> int:
    """upload_meta (csrc/shz_extract.hip): the segment length of ONE sub-batch of `frames` frames.  fp32 staging: the
    rule's 20 slabs and 6 workgroups per CU; fp64 staging: 9 slabs, 3 per CU."""
    n_slabs, wg_per_cu = (9, 3) if f64 else (20, 6)
    slots = compute_units * wg_per_cu
    if frames * n_slabs // 672 >= 4 * slots:
        return 672
    if frames * n_slabs // 252 * 8 < slots:
        return 42
    return 252


def _pair_plan():
    """(t mod 7 of the first cell, frame distance, exact): every distance 1..11 equal and one count apart, a pair in
    neighbouring blocks from every place of the block, pairs inside one block"""
    plan = [((2 * dt + 3 * v) % BH, dt, v == 0) for dt in range(1, 12) for v in (0, 1)]
    plan += [(p, BH, p % 2 == 0) for p in range(BH)]
    plan += [(0, 3, True), (1, 5, False), (2, 2, True), (4, 2, False)]
    return plan


def _plan(G):
    """name -> (frames, items, background): items as oracle.tie_geometry takes them; background "noise" (the same for
    every clip) or "zero" (the long clips: only the tiles' frames cost a transform)"""
    seeds = iter(G.EDGE_SEEDS)
    clips, cur, a, n = {}, [], 11, 0

    def flush():
        nonlocal cur, a
        if cur:
            clips[f"pairs{len(clips)}"] = (CLIP_FRAMES, cur, "noise")
        cur, a = [], 11

    for p, dt, exact in _pair_plan():
        while a % BH != p:
            a += 1
        if a + dt > 52:
            flush()
            while a % BH != p:
                a += 1
        if dt == 1:
            mode = ("period", 1) if exact else ("period", 1, G.PERIOD_STEP_SAMPLES[n % 4])
            cur.append((a, next(seeds), mode, []))
        else:
            cur.append((a, next(seeds), ("exact",) if exact else ("step", G.STEP_SAMPLES[n % 4]), [a + dt]))
        a += dt + 13
        n += 1
    flush()
    s = lambda: next(seeds)
    # a clip's first and last ten frames
    clips["edge0"] = (40, [(0, s(), ("exact",), [6]), (33, s(), ("step", 240), [39])], "noise")
    clips["edge1"] = (40, [(3, s(), ("step", 200), [9]), (31, s(), ("exact",), [38])], "noise")
    clips["edge2"] = (40, [(4, s(), ("exact",), [9, 14]), (27, s(), ("last", 200), [32, 37])], "noise")
    clips["edge3"] = (22, [(9, s(), ("exact",), [20])], "noise")      # 11 apart: rows 9 and 20 of 22
    # three in a row over three blocks
    clips["chain0"] = (40, [(6, s(), ("exact",), [11, 16])], "noise")
    clips["chain1"] = (40, [(13, s(), ("last", 200), [18, 23])], "noise")
    # on either side of frame 42 (a segment boundary of the 42-frame regime)
    clips["b42a"] = (CLIP_FRAMES, [(38, s(), ("exact",), [44])], "noise")
    clips["b42b"] = (CLIP_FRAMES, [(40, s(), ("step", 280), [43])], "noise")
    clips["b42c"] = (CLIP_FRAMES, [(39, s(), ("exact",), [44, 49])], "noise")
    clips["b42d"] = (CLIP_FRAMES, [(41, s(), ("period", 1, 500), [])], "noise")
    # ... of frames 252 and 672
    for B in (252, 672):
        clips[f"b{B}a"] = (B + 24, [(B - 4, s(), ("exact",), [B + 3])], "zero")
        clips[f"b{B}b"] = (B + 24, [(B - 1, s(), ("step", 160), [B + 1])], "zero")
        clips[f"b{B}c"] = (B + 24, [(B - 3, s(), ("last", 200), [B + 2, B + 7])], "zero")
    # ties inside one row
    clips["row0"] = (CLIP_FRAMES, [(5 + 15 * q, SYM[j][0], ("sym", SYM[j][1]), []) for q, j in enumerate((1, 2, 3, 4))], "noise")
    clips["row1"] = (CLIP_FRAMES, [(5 + 15 * q, SYM[j][0], m, []) for q, (j, m) in enumerate(
        ((5, ("sym", SYM[5][1])), (6, ("sym", SYM[6][1])), (6, ("symfix", ())), (4, ("symfix", ()))))], "noise")
    return clips


# row8 clips: (frame, j, sample of the one count or None)
ROW8 = {"row8a": [(5, 5, None), (20, 5, 251), (35, 5, 201), (50, 5, 401)],     # at bin 1280: 0, 2, 3, 1 key steps apart
        "row8b": [(5, 6, None), (20, 4, 401), (35, 4, 251), (50, 3, 201)]}


def _tile8(G, j, n):
    t = G.tile(TILE8[j], TILE8_AMP).copy()
    keep = np.zeros(NFFT, bool)
    keep[::8] = True
    t[~keep] = 0
    if n is not None:
        assert n % 8
        t[n] += 1
    return t


def _edge_tones(synth, frames, first, seed):
    """noise (amplitude 1,500) with tones of 5,000 counts in 2,048 samples that only the clip's first / last frame holds"""
    x = synth.synth_clip(seed, frames, NFFT + (frames - 1) * HOP, 0, 1500).astype(np.float64)
    n = np.arange(HOP, dtype=np.float64)
    tone = sum(5000.0 * np.cos(2.0 * np.pi * b * n / NFFT + 0.3 * i) for i, b in enumerate(TONE_BINS))
    if first:
        x[:HOP] += tone
    else:
        x[-HOP:] += tone
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _build(G, frames, items, bg):
    if bg == "noise":
        return G.build_clip(frames, items, bg_clip=0)
    x = np.zeros(HOP * (frames - 1) + NFFT + 1, np.int16)
    for it in items:
        G._put(x, it)
    return x


def _without_partner(item):
    a, seed, mode, frames = item
    if not frames:                   # a period stretch: nothing to take away
        return item
    return (a, seed, ("exact",) if mode[0] in ("step", "last") else mode, list(frames[:-1]))


@pytest.fixture(scope="module")
def env():
    """every clip and its reference, made once and shared (read-only)"""
    import shazam_amd as S
    from shazam_amd import _ffi
    from oracle import cpu_ref as O, np_exact as E, synth, tie_geometry as G
    ctx = S.get_context(0)
    fused = _ffi.numpy_product_is_fused()
    cache = {}

    def reference(x):
        """tie_geometry.reference with the exact spectrum of a frame kept across clips"""
        fr = np.lib.stride_tricks.sliding_window_view(x, NFFT)[::HOP]
        P = np.empty((NBINS, fr.shape[0]))
        for f, row in enumerate(fr):
            key = row.tobytes()
            if key not in cache:
                cache[key] = E.psd_exact(row, 44100, HOP, NFFT, fused)[:, 0].copy()
            P[:, f] = cache[key]
        pf, pt = O.sort_peaks(*O.peaks_2d(G.db_exact(P), 10.0))
        k, t1 = O.pair_keys(pf, pt, 5)
        return pf, pt, k, t1, P

    plan = _plan(G)
    clips = {name: _build(G, *spec) for name, spec in plan.items()}
    for name, tiles in ROW8.items():
        x = G.build_clip(CLIP_FRAMES, [], bg_clip=0)
        for a, j, n in tiles:
            x[HOP * a:HOP * a + NFFT] = _tile8(G, j, n)
        clips[name] = x
    clips["tones_first"] = _edge_tones(synth, 22, True, 708)
    clips["tones_last"] = _edge_tones(synth, 22, False, 707)
    refs = {name: reference(x) for name, x in clips.items()}
    # the same clips without the last copy of every pair or chain (the long clips and the period stretches excepted)
    alone = {}
    for name, (frames, items, bg) in plan.items():
        if bg == "noise" and any(it[3] for it in items):
            alone[name] = reference(_build(G, frames, [_without_partner(it) for it in items], bg))
    for x in clips.values():
        x.flags.writeable = False
    return types.SimpleNamespace(ctx=ctx, clips=clips, refs=refs, alone=alone, plan=plan, info=ctx.device_info(), G=G,
                                 reference=reference, fused=fused)


def _bins_at(ref, t):
    return set(ref[0][ref[1] == t].tolist())


def test_the_inputs_hold_what_they_are_for(env):
    """on the references alone"""
    G = env.G
    x = env.clips["chain0"]
    for u, v in zip(env.reference(x), G.reference(x, fused=env.fused)):
        assert np.array_equal(u, v), "the cached reference is tie_geometry.reference"
    wins = {name: G.decisive_windows(ref[4]) for name, ref in env.refs.items()}
    rel_seen, dt_seen, place_seen = set(), set(), set()
    for name, (frames, items, bg) in env.plan.items():
        for it in items:
            fr = G.item_frames(it)
            if len(fr) < 2:
                continue
            # ties across frames: windows whose two nearest cells are this item's, in one bin, within 4 key steps
            tied = [w for w in wins[name] if w[0] == w[3] and w[1] in fr and w[4] in fr and w[1] != w[4]]
            a, b, dt = fr[0], fr[-1], fr[1] - fr[0]
            far = len(fr) == 2 and dt == 11
            if far:
                assert not tied, (name, it)          # the cells do not see each other
            else:
                assert len(tied) >= 5 and dt in {abs(w[1] - w[4]) for w in tied} <= {dt, 2 * dt}, (name, it, len(tied))
            if not far and (it[2][0] in ("step", "last") or len(it[2]) > 2):
                assert any(1 <= w[2] <= 4 for w in tied), (name, it, "no pair one to four key steps apart")
            if name in env.alone and it[3]:
                with_, without = env.refs[name], env.alone[name]
                held = _bins_at(without, a)          # peaks of the first copy's frame when the last copy is not there
                if far or it[2][0] == "exact":       # out of sight, or equal powers: both stay peaks
                    assert len(held & _bins_at(with_, a) & _bins_at(with_, b)) >= 5, (name, it)
                else:                                # one count apart: the partner takes bins from the first copy
                    assert len((held - _bins_at(with_, a)) & _bins_at(with_, b)) >= 1, (name, it)
            if name.startswith("pairs"):
                rel_seen.add(((a % BH + dt) // BH, a % BH))
                dt_seen.add((dt, it[2][0] in ("exact",) or it[2] == ("period", 1)))
            if len(fr) == 3:
                assert len({t // BH for t in fr}) == 3, (name, it)
            place_seen.add(("first10", a < 10))
            place_seen.add(("last10", b >= frames - 10))
            for B in (42, 252, 672):
                place_seen.add((B, a < B <= b))
    assert {(1, p) for p in range(BH)} <= rel_seen and any(r == 0 for r, _ in rel_seen) and any(r == 2 for r, _ in rel_seen)
    assert {(dt, e) for dt in range(1, 12) for e in (True, False)} <= dt_seen, sorted(dt_seen)
    assert {("first10", True), ("last10", True), (42, True), (252, True), (672, True)} <= place_seen
    # ties inside a row: zero-odd-samples tiles, j = 1..6.  Up to j = 5 the two cells share their windows: the pair is the
    # window's two largest; at j = 6 (12 bins) neither sees the other and both are peaks
    def in_row(name, a, lo, hi):
        got = {(min(w[0], w[3]), max(w[0], w[3])) for w in wins[name] if w[1] == a and w[4] == a}
        if hi - lo <= 10:
            assert (lo, hi) in got, (name, a, lo, hi, sorted(got))
        else:
            assert (lo, hi) not in got and {lo, hi} <= _bins_at(env.refs[name], a), (name, a, lo, hi)

    js = []
    for name in ("row0", "row1"):
        for a, seed, mode, _ in env.plan[name][1]:
            j = [j for j, (sd, _) in SYM.items() if sd == seed][0]
            in_row(name, a, 1024 - j, 1024 + j)
            js.append(j)
    assert set(js) == set(range(1, 7)), js
    # ... every eighth sample kept: the pair round bin 1280 lies inside slab 29 up to j = 4, on either side of its first
    # bin 1276 from j = 5 on
    for name, tiles in ROW8.items():
        for a, j, n in tiles:
            in_row(name, a, C8 - j, C8 + j)
            assert ((C8 - j) // OW != (C8 + j) // OW) == (j >= 5)
    assert {j for tiles in ROW8.values() for _, j, _ in tiles} >= {4, 5, 6}
    # tones in the first and in the last frame, in the first and in the last eleven bins
    for name, row in (("tones_first", 0), ("tones_last", 21)):
        at = _bins_at(env.refs[name], row)
        assert at & set(range(0, 11)) and at & set(range(2038, 2049)), (name, sorted(at))


def _extract(ctx, pcm, off, f64):
    ctx.set_stage_f64(f64)
    try:
        k, t1, ho, _ = ctx.fingerprint_batch(pcm, off, pcm_device=True)
        pf, pt, po = ctx.peaks(pcm, off, pcm_device=True)
    finally:
        ctx.set_stage_f64(False)
    return k, t1, ho, pf, pt, po


def _assert_clip(out, i, ref, what):
    k, t1, ho, pf, pt, po = out
    rf, rt, rk, rt1 = ref[:4]
    a, b = int(po[i]), int(po[i + 1])
    got, want = list(zip(pt[a:b].tolist(), pf[a:b].tolist())), list(zip(rt.tolist(), rf.tolist()))
    if got != want:
        only_dev, only_ref = sorted(set(got) - set(want)), sorted(set(want) - set(got))
        raise AssertionError(f"{what}: peaks differ: {len(got)} on the device, {len(want)} in the reference; (frame, bin) "
                             f"only on the device {only_dev[:8]}, only in the reference {only_ref[:8]}, "
                             f"twice on the device {len(got) - len(set(got))}")
    a, b = int(ho[i]), int(ho[i + 1])
    assert np.array_equal(k[a:b], rk) and np.array_equal(t1[a:b], rt1), f"{what}: hashes differ"


def _run_batch(env, regime, max_frames=1 << 20):
    """every clip of at most max_frames frames, each at the sample offset the lengths in front of it give, behind one half
    and in front of the other half of the filler clips (made on the device) that put the batch into `regime` in both
    staging modes"""
    ctx, cus = env.ctx, env.info["compute_units"]
    names = [n for n, x in env.clips.items() if ctx.frames_of(len(x)) <= max_frames]
    xs = [env.clips[n] for n in names]
    own = sum(ctx.frames_of(len(x)) for x in xs)
    for n_fill in range(0, 4000, 2):
        f = own + n_fill * FILL_FRAMES
        if seg_regime(f, cus, False) == regime and seg_regime(f, cus, True) == regime:
            break
    else:
        pytest.fail(f"no batch size reaches {regime}-frame segments in both staging modes on {cus} compute units")
    n_fill += 8 if regime == 672 else 0
    k1 = n_fill // 2
    off = [i * FILL_SAMPLES for i in range(k1 + 1)]
    for x in xs:
        off.append(off[-1] + len(x))
    pad = -off[-1] % 64   # zeros up to a multiple of 64 samples: they belong to the last clip and lie behind its last frame
    assert ctx.frames_of(len(xs[-1]) + pad) == ctx.frames_of(len(xs[-1]))
    off[-1] += pad
    start_post = off[-1]
    off += [start_post + (i + 1) * FILL_SAMPLES for i in range(n_fill - k1)]
    off = np.array(off, np.uint64)
    frames = sum(ctx.frames_of(int(off[i + 1] - off[i])) for i in range(len(off) - 1))
    for f64 in (False, True):
        assert seg_regime(frames, cus, f64) == regime, (frames, cus, f64, regime)
    assert frames <= min(1 << 20, (env.info["hbm_bytes"] // 4) // (2056 * 8)), "one sub-batch"
    ctx.set_workspace_limit(0)
    buf = ctx.alloc(int(off[-1]) * 2)
    try:
        at = lambda sample: types.SimpleNamespace(ptr=buf.ptr + 2 * int(sample))
        if k1:
            ctx.synth_pcm(9393, 0, k1, FILL_SAMPLES, 0, 8000, out=at(0))
        if n_fill - k1:
            ctx.synth_pcm(9393, k1, n_fill - k1, FILL_SAMPLES, 0, 8000, out=at(start_post))
        buf.upload(np.concatenate(xs + [np.zeros(pad, np.int16)]), 2 * k1 * FILL_SAMPLES)
        ctx.sync()
        s0 = ctx.extract_stats()
        out32 = _extract(ctx, buf, off, False)
        s1 = ctx.extract_stats()
        out64 = _extract(ctx, buf, off, True)
    finally:
        buf.free()
    # the fp32 picker itself answered: no whole pass and no clip was redone with fp64 staging
    assert s1["f64_passes"] == s0["f64_passes"] and s1["f64_clips"] == s0["f64_clips"], (s0, s1)
    # ... and it listed cells: the near-ties went through peak_verify
    assert s1["undecided"] > s0["undecided"], (s0, s1)
    for i, n in enumerate(names):
        _assert_clip(out32, k1 + i, env.refs[n], (n, regime, "fp32 staging"))
        _assert_clip(out64, k1 + i, env.refs[n], (n, regime, "fp64 staging"))
    for u, v in zip(out32, out64):   # (the filler is not compared with the CPU; the two staging modes must agree on it)
        assert np.array_equal(u, v), regime


def test_short_segments(env):
    """segments of 42 frames: frame 42 of the 64-frame clips begins a segment, and the blocks start again there.  (Only a
    batch of fewer than 2,400 frames is cut this way: the six long clips stay out)"""
    _run_batch(env, 42, CLIP_FRAMES)


def test_middle_segments(env):
    """segments of 252 frames"""
    _run_batch(env, 252)


def test_long_segments(env):
    """a batch of the benchmark's size, segments of 672 frames"""
    _run_batch(env, 672)
