"""GPU: fp32 peak picking (peak_pick32 + peak_verify, csrc/shz_peak32.inc) on near-ties BUILT from PCM and placed at every
edge of the picker's geometry, judged by the CPU statement of the operation -- not by the other GPU path.

Inputs (oracle/tie_geometry.py): a 4,096-sample noise tile written at two frame-aligned positions ties all 2,049 bins of
the two frames; the second copy is exact, carries one extra count on one sample (fp32 keys 0..4 steps apart, fp64 powers
>= 1e-13 apart), is reversed in time, or has alternating signs (bin f -> 2048 - f).  Placed at every frame distance
1..11, at every phase of the 21-frame van Herk block, at frames 0..9 and the last ten of a clip, at the last frame of one
clip against the first of the next, in chains of 3 / 8 / 21 tied cells, and across frames 42, 84, 252, 504, 672 -- the
multiples of the three segment lengths `upload_meta` (csrc/shz_extract.hip) cuts clips into.  One more kind ties two
cells of ONE row (a tile with zero odd samples has |X[1024 - j]| = |X[1024 + j]|): with a count on an odd sample the two
share an fp32 key and differ in dB; with searched counts on even samples they share the dB value and lie on opposite
sides of an fp32 rounding boundary.

Reference (tie_geometry.reference): np_exact.psd_exact -> the correctly rounded dB of the library's host function
shz_db_values -> cpu_ref.peaks_2d / sort_peaks / pair_keys.  Peaks and hashes of every crafted clip must equal it bit for
bit, in order, with fp32 staging and with fp64 staging, alone and inside batches of all three segment regimes.

Which regime a batch is in cannot be read back from the library; `seg_regime` restates the rule of `upload_meta` from
the device's compute-unit count and the test FAILS if a batch does not land where it is meant to."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL_SAMPLES = 2048 * 643 + 4096          # a 30 s filler clip: 644 frames
FILL_FRAMES = 644


def seg_regime(frames: int, compute_units: int, f64: bool) -> int:
    """Segment length peak picking uses for ONE sub-batch of `frames` frames: upload_meta, csrc/shz_extract.hip
    (`seg_len = frames * n_slabs / 672 >= 4 * slots ? 672 : frames * n_slabs / 252 * 8 < slots ? 42 : 252`, integer
    division; slots = compute units * workgroups per CU).  fp32 staging: 20 slabs of 105 bins (MG_F32), 12 / P32_NW = 6
    workgroups per CU; fp64 staging: 9 slabs of 228 bins (MG_F64), 3 per CU (the call in extract_enqueue)."""
    n_slabs, wg_per_cu = (9, 3) if f64 else (20, 6)
    slots = compute_units * wg_per_cu
    if frames * n_slabs // 672 >= 4 * slots:
        return 672
    if frames * n_slabs // 252 * 8 < slots:
        return 42
    return 252


def one_sub_batch(frames: int, hbm_bytes: int) -> bool:
    """plan_sub_batches: a call is cut where frames * bytes per staged frame exceed the workspace limit (a quarter of the
    device memory unless set otherwise) or 2^20 frames.  fp64 rows are the larger: DB_STRIDE * 8 bytes."""
    return frames <= min(1 << 20, (hbm_bytes // 4) // (2056 * 8))


@pytest.fixture(scope="module")
def env():
    import shazam_amd as S
    from shazam_amd import _ffi
    from oracle import tie_geometry as G
    ctx = S.get_context(0)
    fused = _ffi.numpy_product_is_fused()
    names, pcm, plan = G.crafted_clips()
    refs = [G.reference(x, fused=fused) for x in pcm]
    return types.SimpleNamespace(S=S, ctx=ctx, G=G, fused=fused, names=names, pcm=pcm, plan=plan, refs=refs,
                                 info=ctx.device_info())


@pytest.fixture
def default_workspace(env):
    """The regime arithmetic assumes the default workspace limit (a quarter of the device memory); the library has no
    getter, so whoever changed it on the shared context loses that setting for the rest of the session -- as they would
    with any other test that sets it."""
    env.ctx.set_workspace_limit(0)
    yield
    env.ctx.set_workspace_limit(0)


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
    rf, rt, rk, rt1, _ = ref
    a, b = int(po[i]), int(po[i + 1])
    got, want = list(zip(pt[a:b].tolist(), pf[a:b].tolist())), list(zip(rt.tolist(), rf.tolist()))
    if got != want:
        only_dev, only_ref = sorted(set(got) - set(want)), sorted(set(want) - set(got))
        raise AssertionError(f"{what}: peaks differ: {len(got)} on the device, {len(want)} in the reference; (frame, bin) "
                             f"only on the device {only_dev[:8]}, only in the reference {only_ref[:8]}")
    a, b = int(ho[i]), int(ho[i + 1])
    assert np.array_equal(k[a:b], rk) and np.array_equal(t1[a:b], rt1), f"{what}: hashes differ"


def test_the_built_ties_cover_the_geometry(env):
    """Counted from the reference's spectrogram alone (the same conditions as tests/test_tie_geometry_ref.py asserts on
    the CPU): >= 5 decisive windows per key-step class 0..4 for every position class of the maximum's bin, for every
    frame distance 1..10 and for every segment boundary."""
    G = env.G
    by_pos, by_dt, by_b = G.coverage([G.decisive_windows(r[4]) for r in env.refs])
    for step in range(5):
        for c in G.BIN_CLASSES:
            assert by_pos.get((step, c), 0) >= 5, (step, c, by_pos.get((step, c), 0))
        for dt in range(1, 11):
            assert by_dt.get((step, dt), 0) >= 5, (step, dt)
        for B in G.BOUNDARIES:
            assert by_b.get((step, B), 0) >= 5, (step, B)
    # ties inside one row: two cells of a frame with the same fp32 key and different dB values
    i = env.names.index("inrow")
    A = G.db_exact(env.refs[i][4])
    assert sum(1 for (f, t, s, f2, t2) in G.decisive_windows(env.refs[i][4])
               if t2 == t and f + f2 == 2048 and s == 0 and A[f, t] != A[f2, t]) >= 10
    # ... and two cells of a row with ONE dB value whose fp32 keys differ by a step (both are peaks)
    i = env.names.index("straddle")
    assert len(G.straddling_pairs(env.plan[i][2], env.refs[i])) >= 8


@pytest.mark.parametrize("f64", [False, True], ids=["fp32_staging", "fp64_staging"])
def test_every_clip_alone(env, f64):
    """One clip per call: 42-frame segments (every boundary of BOUNDARIES is a segment boundary here)."""
    ctx = env.ctx
    for i, (name, x) in enumerate(zip(env.names, env.pcm)):
        frames = env.plan[i][1]
        assert seg_regime(frames, env.info["compute_units"], f64) == 42, (name, frames, env.info)
        s0 = ctx.extract_stats()
        out = _extract(ctx, x, np.array([0, len(x)], np.uint64), f64)
        s1 = ctx.extract_stats()
        _assert_clip(out, 0, env.refs[i], (name, "alone", "fp64" if f64 else "fp32"))
        # the fp32 picker itself answered: no whole-pass fallback, no clip redone with fp64 staging
        assert s1["f64_passes"] == s0["f64_passes"] and s1["f64_clips"] == s0["f64_clips"], (name, s0, s1)


def test_chains_are_settled_by_the_verification_kernel(env):
    """3, 8 and 21 tied cells per bin in one window stay below PV_MAX_NEAR = 32: peak_verify decides them on fp64 values
    (decided_f64 rises) and neither the per-clip fp64 pass nor the whole-pass fallback is taken.  chain*: equal cells, all
    peaks; chain*p: the last copy carries one count, so among 3 / 8 / 21 cells within two key steps the kernel has to find
    the ONE maximum (or the n - 1 equal ones): the reference has peaks and non-peaks among them, counted here."""
    ctx, G = env.ctx, env.G
    for name in ("chain3p", "chain8p", "chain21p"):
        i = env.names.index(name)
        mixed, _ = G.chain_mixed_bins(env.plan[i][2][0], env.refs[i])
        assert len(mixed) >= 5, (name, mixed)
    for name in ("chain3", "chain8", "chain21", "chain3p", "chain8p", "chain21p"):
        i = env.names.index(name)
        x = env.pcm[i]
        s0 = ctx.extract_stats()
        out = _extract(ctx, x, np.array([0, len(x)], np.uint64), False)
        s1 = ctx.extract_stats()
        _assert_clip(out, 0, env.refs[i], name)
        assert s1["decided_f64"] > s0["decided_f64"], (name, s0, s1)
        assert s1["f64_clips"] == s0["f64_clips"] and s1["f64_passes"] == s0["f64_passes"], (name, s0, s1)


def test_more_than_32_tied_cells_take_the_per_clip_fp64_pass(env):
    """A click per hop: flat spectra, hundreds of cells within two key steps of every window's maximum.  The clip is
    marked and redone with fp64 staging (f64_clips rises), its neighbours in the batch stand, all equal the reference."""
    ctx, G = env.ctx, env.G
    click = G.click_per_hop(40)
    ia, ib = env.names.index("edge0"), env.names.index("edge1")
    xs = [env.pcm[ia], click, env.pcm[ib]]
    refs = [env.refs[ia], G.reference(click, fused=env.fused), env.refs[ib]]
    assert len(refs[1][0]) > 0
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)
    x = np.concatenate(xs)
    s0 = ctx.extract_stats()
    out = _extract(ctx, x, off, False)
    s1 = ctx.extract_stats()
    assert s1["f64_clips"] > s0["f64_clips"], (s0, s1)
    assert s1["f64_passes"] == s0["f64_passes"], (s0, s1)
    out64 = _extract(ctx, x, off, True)
    for i in range(3):
        _assert_clip(out, i, refs[i], ("click batch fp32", i))
        _assert_clip(out64, i, refs[i], ("click batch fp64", i))


def _filler_count(env, want: int) -> int:
    """The smallest number of 644-frame filler clips that puts the batch (filler + every crafted clip) into the `want`
    regime with fp32 AND with fp64 staging, plus a margin of 8 clips for the long regime."""
    crafted = sum(p[1] for p in env.plan)
    cus = env.info["compute_units"]
    for n in range(2, 4000, 2):
        f = crafted + n * FILL_FRAMES
        if seg_regime(f, cus, False) == want and seg_regime(f, cus, True) == want:
            return n + (8 if want == 672 else 0)
    pytest.fail(f"no batch size reaches {want}-frame segments in both staging modes on {cus} compute units")


@pytest.mark.parametrize("regime", [252, 672])
def test_inside_batches_of_the_longer_segment_regimes(env, default_workspace, regime):
    """The crafted clips, packed at odd sample offsets, between device-made noise clips (ctx.synth_pcm) before and after
    them: a batch of a middle size (252-frame segments: frames 252 and 504 are boundaries, 42 / 84 / 672 are not) and one
    of the benchmark's size or larger (672-frame segments: only frame 672 is).  The PCM lives on the device, so the call
    is one extraction pass over the whole batch (host PCM would be cut into upload chunks of 16-64 MB)."""
    ctx, cus = env.ctx, env.info["compute_units"]
    n_fill = _filler_count(env, regime)
    k1 = n_fill // 2
    # layout in samples: k1 filler clips, ONE more sample (so the crafted clips start at an odd offset; it belongs to the
    # last filler clip), the crafted clips, zeros up to a multiple of 64 (they belong to the last crafted clip and lie
    # behind its last frame), n_fill - k1 filler clips
    off = [i * FILL_SAMPLES for i in range(k1)] + [k1 * FILL_SAMPLES + 1]
    for x in env.pcm:
        off.append(off[-1] + len(x))
    pad = -off[-1] % 64
    off[-1] += pad
    start_post = off[-1]
    off += [start_post + (i + 1) * FILL_SAMPLES for i in range(n_fill - k1)]
    off = np.array(off, np.uint64)
    assert int(off[k1]) % 2 == 1 and sum(int(o) % 2 for o in off[k1:k1 + len(env.pcm)]) >= len(env.pcm) // 3
    frames = sum(ctx.frames_of(int(off[i + 1] - off[i])) for i in range(len(off) - 1))
    assert frames == n_fill * FILL_FRAMES + sum(p[1] for p in env.plan)
    for f64 in (False, True):
        assert seg_regime(frames, cus, f64) == regime, (frames, cus, f64)
    assert one_sub_batch(frames, env.info["hbm_bytes"]), (frames, env.info)
    buf = ctx.alloc(int(off[-1]) * 2)
    try:
        at = lambda sample: types.SimpleNamespace(ptr=buf.ptr + 2 * int(sample))
        ctx.synth_pcm(9090, 0, k1, FILL_SAMPLES, 0, 8000, out=at(0))
        ctx.synth_pcm(9090, k1, n_fill - k1, FILL_SAMPLES, 0, 8000, out=at(start_post))
        mid = np.concatenate([np.zeros(1, np.int16)] + list(env.pcm) + [np.zeros(pad, np.int16)])
        buf.upload(mid, 2 * k1 * FILL_SAMPLES)
        ctx.sync()
        s0 = ctx.extract_stats()
        out32 = _extract(ctx, buf, off, False, pcm_device=True)
        s1 = ctx.extract_stats()
        assert s1["f64_passes"] == s0["f64_passes"] and s1["f64_clips"] == s0["f64_clips"], (s0, s1)
        out64 = _extract(ctx, buf, off, True, pcm_device=True)
    finally:
        buf.free()
    for i, name in enumerate(env.names):
        _assert_clip(out32, k1 + i, env.refs[i], (name, regime, "fp32"))
        _assert_clip(out64, k1 + i, env.refs[i], (name, regime, "fp64"))
    # the filler is not compared with the CPU; the two staging modes must still agree on it
    for u, v in zip(out32, out64):
        assert np.array_equal(u, v), regime
    assert int(out32[5][k1]) > 0 and int(out32[5][-1]) > int(out32[5][k1 + len(env.names)])
