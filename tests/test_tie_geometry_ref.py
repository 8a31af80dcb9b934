"""CPU: the judge of tests/test_gpu_peak_ties_geometry.py is pinned before any GPU is asked.

(1) `tie_geometry.reference` (np_exact.psd_exact -> the host's correctly rounded dB, shz_db_values -> cpu_ref.peaks_2d /
    sort_peaks / pair_keys) reproduces the reference's own peaks and hashes on the committed near-tie fixtures
    (tests/golden/tie_cases.npz) and agrees with the numpy oracle on the two-identical-frames clips of
    tests/test_gpu_extract_fuzz.py.
(2) The builder's inputs hold the ties they are meant to hold: counted from the reference's spectrogram alone, at least
    5 decisive windows (maximum with a second cell within 4 fp32 key steps) for every key-step class 0..4 in every
    position class of the picker's geometry, at every frame distance 1..10 and across every segment boundary; nothing at
    distance 11; every phase of the 21-frame block; every clip edge.  A later change to the builder cannot quietly empty
    a class."""
import os

import numpy as np
import pytest

from oracle import cpu_ref as O, np_exact as E, synth, tie_geometry as G


@pytest.fixture(scope="module")
def crafted():
    names, pcm, plan = G.crafted_clips()
    P = [G.psd_exact_frames(x) for x in pcm]
    return names, pcm, plan, P


def test_frame_cache_is_psd_exact():
    x = np.concatenate([G.tile(1007), G.tile(1007), synth.synth_clip(3, 1, 5000, 2000, 900)])
    assert np.array_equal(G.psd_exact_frames(x), E.psd_exact(x, 44100, 2048))
    assert np.array_equal(G.psd_exact_frames(x[:1000]), E.psd_exact(x[:1000], 44100, 2048))


@pytest.mark.parametrize("name", ["sine_1k_10s", "two_tone_10s", "dc_12000_5s", "chirp_200_4000_10s", "tonal_noiseless_10s",
                                  "sparse_clicks_5s", "click_train_30s"])
def test_reference_reproduces_the_tie_goldens(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "tie_cases.npz"))
    x = synth.tie_inputs()[name]
    f, t, k, t1, _ = G.reference(x)          # (the fixtures' host forms conj(z) * z with an FMA: fused)
    assert set(zip(f.tolist(), t.tolist())) == set(zip(g[f"{name}_peaks_f"].tolist(), g[f"{name}_peaks_t"].tolist()))
    assert O.sha1_hex20(k) == [bytes(h).decode() for h in g[f"{name}_hash_hex"]]
    assert t1.tolist() == g[f"{name}_hash_t1"].tolist()


def test_reference_on_two_identical_frames():
    """The exact two-cell ties of test_gpu_extract_fuzz.py: noise far from any dB rounding, so numpy's logarithm gives the
    same answer and the oracle's fingerprint is the yardstick; the tied cells are peaks in pairs."""
    n_pairs = 0
    for c in range(6):
        x = synth.synth_clip(515, c, 2048 * 70, 0, 6000).copy()
        a, b = 10 + c, 15 + c
        x[2048 * b:2048 * b + 4096] = x[2048 * a:2048 * a + 4096]
        f, t, k, t1, _ = G.reference(x)
        ok, ot1, of, ot = O.fingerprint_keys(x)
        assert np.array_equal(f, of) and np.array_equal(t, ot) and np.array_equal(k, ok) and np.array_equal(t1, ot1), c
        pk = set(zip(f.tolist(), t.tolist()))
        n_pairs += sum(1 for (ff, tt) in pk if tt == a and (ff, b) in pk)
    assert n_pairs >= 3


def test_builder_places_what_it_says(crafted):
    names, pcm, plan, P = crafted
    phases, dts = set(), set()
    straddle = {B: 0 for B in G.BOUNDARIES}
    for (name, nf, items), x, p in zip(plan, pcm, P):
        assert p.shape == (G.NBINS, nf) and len(x) % 2 == 1, name
        for it in items:
            fr = G.item_frames(it)
            if name.startswith("long"):
                phases.add(fr[0] % 21)
                dts.add(fr[-1] - fr[0])
                for B in G.BOUNDARIES:
                    if fr[0] < B <= fr[-1]:
                        assert B - 10 <= fr[0] and fr[-1] <= B + 9, (name, it)
                        straddle[B] += 1
            if it[2][0] in ("exact", "period") and len(it[2]) == 2 or it[2] == ("exact",):
                for b in fr[1:]:          # exact copies: every bin of the two frames ties bit for bit
                    assert np.array_equal(p[:, fr[0]], p[:, b]), (name, it)
    assert phases == set(range(21)) and dts >= set(range(1, 12))
    assert all(v >= 4 for v in straddle.values()), straddle
    edge = [pl for pl in plan if pl[0].startswith("edge")]
    assert {it[0] for _, _, its in edge for it in its[:1]} == set(range(10))
    assert {G.item_frames(its[1])[-1] for _, nf, its in edge} == set(range(52 - 10, 52))
    # last frame of cross{j} == first frame of cross{j + 1} (even j + 1), one count apart for odd j + 1
    for j in range(7):
        a, b = P[names.index(f"cross{j}")][:, -1], P[names.index(f"cross{j + 1}")][:, 0]
        assert np.array_equal(a, b) == ((j + 1) % 2 == 0)
        assert np.allclose(a, b, rtol=1e-3)


def test_coverage_of_the_built_ties(crafted):
    names, pcm, plan, P = crafted
    wins = [G.decisive_windows(p) for p in P]
    by_pos, by_dt, by_b = G.coverage(wins)
    for step in range(5):
        for c in G.BIN_CLASSES:
            assert by_pos.get((step, c), 0) >= 5, (step, c, by_pos.get((step, c), 0))
        for dt in range(1, 11):
            assert by_dt.get((step, dt), 0) >= 5, (step, dt, by_dt.get((step, dt), 0))
        for B in G.BOUNDARIES:
            assert by_b.get((step, B), 0) >= 5, (step, B, by_b.get((step, B), 0))
    # dt = 11 is outside the window: the cells of a perturbed pair never meet, so where the tile tops its window BOTH
    # the larger and the smaller cell are peaks of the reference
    both = 0
    for (name, nf, items), x in zip(plan, pcm):
        for it in items:
            fr = G.item_frames(it)
            if name.startswith("long") and fr[-1] - fr[0] == 11 and it[2][0] == "step":
                f, t, _, _, p = G.reference(x)
                pk = set(zip(f.tolist(), t.tolist()))
                both += sum(1 for b in range(G.NBINS) if (b, fr[0]) in pk and (b, fr[1]) in pk and p[b, fr[0]] != p[b, fr[1]])
    assert both >= 20, both
    # clip edges: decisive windows centred in frames 0..9 and in the last ten frames; none between clips
    early = sum(1 for n, w in zip(names, wins) if n.startswith("edge") for (_, t, _, _, _) in w if t < 10)
    late = sum(1 for n, w in zip(names, wins) if n.startswith("edge") for (_, t, _, _, _) in w if t >= 52 - 10)
    assert early >= 100 and late >= 100, (early, late)
    assert all(len(w) == 0 for n, w in zip(names, wins) if n.startswith("cross"))
    # chains: 3, 8, 21 cells of one bin within the top key step of one window
    for name, n in (("chain3", 3), ("chain8", 8), ("chain21", 21)):
        p = P[names.index(name)]
        K = np.float32(p).view(np.int32)
        f, t = max(((f, t) for (f, t, s, _, _) in wins[names.index(name)] if s == 0), key=lambda c: p[c])
        assert int((K[f] >= K[f, t] - 2).sum()) == n, (name, f, t)      # n tied cells in that bin, within 21 frames
        first = plan[names.index(name)][2][0][0]
        assert set(np.where(K[f] >= K[f, t] - 2)[0]) <= set(range(first, first + 21))
    # perturbed chains: bins whose 3 / 8 / 21 cells sit within two key steps and are peaks only in part
    for name in ("chain3p", "chain8p", "chain21p"):
        i = names.index(name)
        mixed, _ = G.chain_mixed_bins(plan[i][2][0], G.reference(pcm[i]))
        assert len(mixed) >= 5, (name, mixed)
    # reversed tile: the same bin a few fp64 ulp apart; alternating signs: bin 1024 - j against 1024 + j, j = 0..5
    rev = wins[names.index("rev")]
    assert sum(1 for (f, t, s, f2, t2) in rev if s <= 1 and f2 == f and t2 != t) >= 50
    alt = wins[names.index("alt")]
    got = {(f2 - f) for (f, t, s, f2, t2) in alt if s <= 1 and f + f2 == 2048 and t2 != t}
    assert {abs(d) for d in got} >= {0, 2, 4, 6, 8, 10}, got
    p = P[names.index("alt")]
    a, b = G.item_frames(plan[names.index("alt")][2][6])          # j = 6: df = 12, the cells do not meet ...
    assert abs(p[1018, a] / p[1030, b] - 1) < 1e-9                 # ... though they hold the same power
    f, t, _, _, _ = G.reference(pcm[names.index("alt")])
    assert (1018, a) in set(zip(f.tolist(), t.tolist())) and (1030, b) in set(zip(f.tolist(), t.tolist()))


def test_ties_inside_a_row(crafted):
    """("sym", n) frames: bins 1024 - j and 1024 + j of ONE frame hold the same fp32 key while their dB values differ, so
    exactly one of the two is a peak -- what a picker that trusts a shared row maximum gets wrong."""
    names, pcm, plan, P = crafted
    i = names.index("inrow")
    A = G.db_exact(P[i])
    same_key = [(f, t, f2) for (f, t, s, f2, t2) in G.decisive_windows(P[i])
                if t2 == t and f + f2 == 2048 and s == 0 and A[f, t] != A[f2, t]]
    assert len(same_key) >= 10, same_key                   # both cells of >= 5 pairs
    pk = set(zip(*[v.tolist() for v in G.reference(pcm[i])[:2]]))
    for f, t, f2 in same_key:
        assert ((f, t) in pk) != ((f2, t) in pk), (f, t, f2)


def test_dB_ties_across_an_fp32_rounding_boundary(crafted):
    """("symfix", S) frames: two cells of one row a few fp64 ulp apart -- one dB value, both peaks -- whose fp32 keys differ
    by one step.  A picker that drops cells one key step below their row's maximum loses the lower one."""
    names, pcm, plan, P = crafted
    i = names.index("straddle")
    assert len(G.straddling_pairs(plan[i][2], G.reference(pcm[i]))) >= 8


def test_click_per_hop_goes_over_the_verification_limit():
    """Every cell of a click-per-hop clip is within two key steps of its window's maximum: far more than PV_MAX_NEAR = 32."""
    p = G.psd_exact_frames(G.click_per_hop(40))
    K = np.float32(p).view(np.int32).astype(np.int64)
    w = K[1000:1021, 10:31]
    assert int((w >= w.max() - 2).sum()) > 32
