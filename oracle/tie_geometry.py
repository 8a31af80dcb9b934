"""TEST INFRASTRUCTURE (oracle): near-ties between spectrogram cells BUILT from PCM, placed at every edge of the fp32
peak picker's geometry, and the CPU statement of what the peaks and hashes of such input are.

Only tests import this (see ``oracle/__init__.py``).

**Construction.**  A *tile* is 4,096 samples of ``synth.synth_clip`` noise.  Written at the frame-aligned positions
``2048 a`` and ``2048 b`` it makes all 2,049 bins of frames a and b tie exactly; every bin that is a window maximum is
then a decisive two-cell tie.  The second copy is varied (``second_copy``):

    ("exact",)    the tile itself: equal powers, key step 0
    ("step", n)   one count added to sample n: the fp32 keys of the two cells differ by 0..4 steps (and more) depending on
                  the bin, while the fp64 powers differ by >= 1e-13 relative -- the reference's answer hangs on no rounding
    ("rev",)      the tile reversed in time (numpy's Hann window is symmetric): same bin, powers equal up to the
                  transform's rounding -- the regime where the correctly rounded logarithm decides
    ("alt",)      the tile times (-1)^n: bin f moves to 2048 - f, so cells (a, 1024 - j) and (b, 1024 + j) nearly tie
    ("symfix", S) the same symmetric tile with counts on the even samples S: see STRADDLE
    ("sym", n)    ONE frame, ties inside a row: with its odd samples zero the tile's spectrum is symmetric about bin 1024,
                  |X[1024 - j]| = |X[1024 + j]|; one count on the odd sample n separates the two cells by 0..4 key steps

``dt = 1`` and chains of copies on consecutive frames cannot be built from whole tiles (frames overlap by half): there
the material is a stretch of period 2,048 (``("period", k)``: k + 1 identical consecutive frames).

**Reference.**  ``reference(x)``: ``np_exact.psd_exact`` (numpy's arithmetic bit for bit), the library's host function
``shz_db_values`` (the correctly rounded 10 log10, checked against ``decimal`` in tests/test_log10_host.py) with zero power
as ``cpu_ref.log_db`` treats it, ``cpu_ref.peaks_2d`` / ``sort_peaks`` / ``pair_keys``.  numpy's log10 is not used.

**Coverage.**  ``decisive_windows`` counts, from the reference's spectrogram alone, the windows whose maximum has a second
cell within 4 fp32 key steps, by key-step class, by position of the maximum's bin in the picker's geometry
(``bin_class``), by frame distance and by the segment boundary the two cells straddle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import cpu_ref as O, np_exact as E, synth

NFFT, HOP, NBINS = 4096, 2048, 2049
SLAB = 105                      # bins per peak_pick32 slab (61 * 2 waves - 17)
BOUNDARIES = (42, 84, 252, 504, 672)   # multiples of the three segment lengths 42 / 252 / 672 (upload_meta)
TILE_AMP, BG_AMP = 6000, 1500   # tiles 12 dB above the background: most tile bins that top their row top their window
LONG_FRAMES = 760
STEP_SAMPLES = (160, 200, 240, 280)
PERIOD_STEP_SAMPLES = (400, 500, 650, 800)   # (a period-2048 stretch has four times the power in its even bins)

# Tile seeds (synth_clip(seed, 0, 4096, 0, TILE_AMP)) whose spectrum tops bins 0..19 inside 0..9 AND bins 2029..2048
# inside 2039..2048, so that every pair built from them has a decisive window in the first and in the last ten bins
# (the first 120 seeds from 1000 on with that property, by np.fft on the Hann-windowed tile; pinned here so that the
# inputs do not depend on the searching host's FFT).
EDGE_SEEDS = (
    1007, 1023, 1029, 1048, 1050, 1052, 1054, 1055, 1056, 1057, 1060, 1067, 1068, 1078, 1093, 1095, 1103, 1104,
    1105, 1110, 1118, 1123, 1124, 1125, 1126, 1129, 1132, 1138, 1139, 1145, 1149, 1152, 1156, 1159, 1164, 1168,
    1169, 1177, 1178, 1180, 1183, 1187, 1189, 1192, 1194, 1196, 1200, 1201, 1202, 1205, 1210, 1211, 1213, 1214,
    1215, 1217, 1226, 1228, 1229, 1237, 1240, 1251, 1252, 1254, 1256, 1260, 1262, 1264, 1266, 1275, 1278, 1280,
    1284, 1287, 1290, 1291, 1297, 1305, 1307, 1309, 1313, 1316, 1321, 1323, 1324, 1331, 1332, 1337, 1346, 1349,
    1350, 1352, 1356, 1359, 1368, 1370, 1372, 1379, 1380, 1381, 1382, 1390, 1391, 1393, 1400, 1403, 1408, 1410,
    1415, 1423, 1425, 1426, 1429, 1430, 1434, 1435, 1437, 1438, 1443, 1448,
)
# (tile seed, sample n) pairs for which the ONE-COUNT perturbation puts the tile's top cell of bins 0..9 (even entries)
# or of bins 2039..2048 (odd entries) exactly 4, 3, 2, 1 fp32 key steps apart, in turn: the first and the last ten bins hold
# one decisive window per pair, so their key-step classes are filled by choice, not by luck (seeds from 2000 on, n tried in
# 160, 200, .., 320, key steps by np_exact.psd_exact; the tests count what the reference finds, whatever this table promises).
TARGETED = (
    (2205, 240), (2151, 200), (2000, 160), (2156, 200), (2013, 160), (2052, 160), (2003, 160), (2027, 160),
    (2213, 240), (2165, 240), (2110, 160), (2168, 240), (2030, 160), (2057, 160), (2019, 160), (2040, 160),
    (2214, 240), (2190, 320), (2146, 200), (2176, 200), (2033, 160), (2114, 200), (2021, 160), (2048, 160),
    (2216, 240), (2225, 280), (2148, 280), (2189, 240), (2080, 160), (2120, 200), (2022, 160), (2065, 160),
    (2221, 280), (2238, 280), (2167, 240), (2197, 200), (2098, 160), (2122, 160), (2026, 160), (2070, 160),
    (2223, 280), (2240, 320), (2169, 240), (2201, 280), (2109, 240), (2123, 200), (2034, 160), (2082, 160),
    (2244, 240), (2256, 280), (2171, 240), (2208, 240), (2112, 200), (2133, 160), (2035, 160), (2085, 160),
    (2247, 240), (2266, 240), (2184, 280), (2210, 240), (2117, 160), (2135, 200), (2037, 160), (2106, 160),
)
# Tile seeds whose spectrum tops bins 1004..1044 at bin 1024 - j, j = 0..6 (the ("alt",) pairs: df = 2 j) and whose pair
# is decisive in the clip plan() builds (the spill of a tile into the half-covered neighbour frames can outrank it): the
# first such seed from 5000 on for each j, picked by hand with decisive_windows
ALT_SEEDS = (5095, 5045, 5059, 5116, 5016, 5076, 5018)


# (tile seed, odd sample n) of the ("sym", n) frames: the symmetric tile tops bins 1004..1044 at 1024 +- j, 1 <= j <= 5
# (the first 24 such seeds from 7000 on, n in turn)
SYM_SEEDS = (
    (7001, 41), (7008, 61), (7009, 81), (7017, 121), (7019, 41), (7025, 61), (7029, 81), (7036, 121),
    (7044, 41), (7045, 61), (7053, 81), (7058, 121), (7062, 41), (7074, 61), (7076, 81), (7079, 121),
    (7083, 41), (7088, 61), (7092, 81), (7105, 121), (7106, 41), (7107, 61), (7113, 81), (7114, 121),
)


# (tile seed, even samples) of the ("symfix", samples) frames.  The symmetric tile's cells 1024 - j and 1024 + j differ by
# the transform's rounding only (a few fp64 ulp: one dB value, both are peaks); a count on an EVEN sample keeps the
# symmetry and moves both powers together.  These sets put the pair on opposite sides of an fp32 rounding boundary: the
# fp32 keys differ by ONE step although the dB values tie -- fact (a) of shz_peak32.inc, the case the classes "within one
# step of the row maximum" (e >= 1) and key_near(.., 1) exist for.  Found by a CPU search: for a seed whose symmetric
# tile tops bins 1004..1044 at 1024 +- j, all 2^24 subsets of 24 even samples (n0 + 74 k) by one-bin DFT updates in
# long double, kept where the power lies within 1.5e-14 of a rounding boundary (about one subset in 5e6), each confirmed
# with np_exact.psd_exact and shz_db_values: one candidate in ~200 straddles.  Three processes, ten minutes.
STRADDLE = (
    (7001, (612, 686, 834, 982, 1056, 1130, 1278, 1574, 1648, 1796, 1870, 1944, 2092, 2314)),
    (7001, (758, 832, 980, 1054, 1276, 1424, 1646, 2238, 2386, 2460)),
    (7001, (776, 850, 924, 1072, 1146, 1368, 1442, 1590, 1664, 1812, 2330, 2404, 2478)),
    (8007, (636, 710, 784, 858, 932, 1006, 1080, 1154, 1228, 1376, 1450, 1524, 1746, 1820, 1968, 2338)),
    (8007, (664, 738, 812, 960, 1330, 1404, 1626, 1700, 1774, 1922, 1996, 2144, 2218, 2292)),
    (8007, (718, 1088, 1236, 1458, 1532, 1606, 1680, 2124, 2272, 2346, 2420)),
    (8007, (798, 1020, 1094, 1316, 1390, 1464, 1612, 1686, 2130, 2278, 2352, 2426)),
    (8007, (798, 1020, 1094, 1316, 1390, 1464, 1612, 1686, 2130, 2278, 2352, 2426)),
    (9001, (1258, 1332, 1406, 1554, 1628, 1702, 1998, 2146, 2220, 2294, 2442)),
    (9001, (884, 1106, 1402, 1476, 1698, 1920, 2142, 2364, 2438, 2512)),
    (9001, (1258, 1332, 1406, 1554, 1628, 1702, 1998, 2146, 2220, 2294, 2442)),
)


def tile(seed: int, amp: int = TILE_AMP) -> np.ndarray:
    return synth.synth_clip(seed, 0, NFFT, 0, amp)


def second_copy(t: np.ndarray, mode: tuple) -> np.ndarray:
    kind = mode[0]
    if kind == "exact":
        return t.copy()
    if kind == "step":
        u = t.copy()
        u[mode[1]] += 1
        return u
    if kind == "rev":
        return t[::-1].copy()
    if kind == "alt":
        u = t.copy()
        u[1::2] = -u[1::2]
        return u
    if kind == "sym":                # not a copy: the tile itself, odd samples zero, one count on the odd sample n
        u = t.copy()
        u[1::2] = 0
        u[mode[1]] += 1
        return u
    if kind == "symfix":             # the symmetric tile with one count on each of the (even) samples mode[1]
        u = t.copy()
        u[1::2] = 0
        u[list(mode[1])] += 1
        return u
    raise ValueError(mode)


# ---------------------------------------------------------------------------------------------------------- the plan
# An item = (first frame a, tile seed, mode, dt or chain frames).  Items of one clip keep >= 13 frames between the last
# full-tile frame of one and the first of the next: their cells never share a window.
def _put(x, item):
    a, seed, mode, frames = item
    t = tile(seed)
    if mode[0] == "period":          # frames a .. a + k identical: period 2,048 over (k + 2) * 2048 samples
        k = mode[1]
        h = t[:HOP]
        x[HOP * a:HOP * (a + k + 2)] = np.tile(h, k + 2)
        if len(mode) > 2:            # one count on a sample only the LAST frame covers, at window position 4095 - n
            x[HOP * (a + k) + NFFT - 1 - mode[2]] += 1
        return
    x[HOP * a:HOP * a + NFFT] = second_copy(t, mode) if mode[0] in ("sym", "symfix") else t
    for b in frames:
        if mode[0] == "last":        # a chain of exact copies whose LAST copy carries the count
            x[HOP * b:HOP * b + NFFT] = second_copy(t, ("step", mode[1])) if b == frames[-1] else t
        else:
            x[HOP * b:HOP * b + NFFT] = second_copy(t, mode)


def item_frames(item):
    """the frames that hold a full copy"""
    a, _, mode, frames = item
    if mode[0] == "period":
        return list(range(a, a + mode[1] + 1))
    return [a] + list(frames)


def build_clip(n_frames: int, items, bg_clip: int, extra: int = 1, bg_seed: int = 4242) -> np.ndarray:
    """Background noise of n_frames frames (+ `extra` samples, so that the next clip of a packed batch starts at an odd
    sample offset) with the items written into it."""
    x = synth.synth_clip(bg_seed, bg_clip, HOP * (n_frames - 1) + NFFT + extra, 0, BG_AMP).copy()
    last = -100
    for it in sorted(items, key=lambda i: i[0]):
        fr = item_frames(it)
        assert fr[0] - last >= 13 or last < 0, (it, last)
        assert 0 <= fr[0] and fr[-1] < n_frames, it
        _put(x, it)
        last = fr[-1]
    assert O.frame_count(len(x)) == n_frames
    return x


def plan():
    """Every crafted clip as (name, n_frames, items).  Deterministic."""
    seeds, targeted = iter(EDGE_SEEDS), iter(TARGETED)

    def pair(a, dt, exact, n=None):
        if exact:
            return (a, next(seeds), ("exact",), [a + dt])
        if n is not None:
            return (a, next(seeds), ("step", n), [a + dt])
        t = next(targeted, None)
        if t is None:
            return (a, next(seeds), ("step", STEP_SAMPLES[a % 4]), [a + dt])
        return (a, t[0], ("step", t[1]), [a + dt])

    clips = []
    # --- long clips: pairs straddling the segment boundaries, and the dt sweep (1..11: exact, then four perturbed rounds, then one more of dt 2..10 with a larger perturbation)
    # with the first frame of the items walking through every phase of the 21-frame van Herk block
    sweep = [(dt, m) for m in range(5) for dt in range(1, 12)] + [(1, m) for m in range(1, 5)] + [(dt, 5) for dt in range(2, 11)]
    si = 0
    for c in range(4):
        items, zones = [], []
        for i, B in enumerate(BOUNDARIES):
            a = B - 1 - (3 * c + 2 * i) % 9
            dt = min(max(B - a, 2) + (c + i) % 3, 10)
            items.append(pair(a, dt, (c + i) % 4 == 0, (240, 280, 320, 300)[(c + i) % 4]))
            zones.append((a - 13, a + dt + 13))
        a = 1
        while si < len(sweep):
            dt, m = sweep[si]
            while a % 21 != (5 * si) % 21 or any(a <= z[1] and a + dt >= z[0] for z in zones):
                a += 1
            if a + dt + 2 >= LONG_FRAMES:
                break
            if dt == 1:
                items.append((a, next(seeds), ("period", 1) if m == 0 else ("period", 1, PERIOD_STEP_SAMPLES[(m + si) % 4]), []))
            else:
                items.append(pair(a, dt, m == 0, 300 if m == 5 else None))
            si += 1
            a += dt + 13
        clips.append((f"long{c}", LONG_FRAMES, items))
    assert si == len(sweep), si
    # --- a at frames 0..9, b in the last ten frames (clipped windows)
    for j in range(10):
        dt = 2 + j % 9
        clips.append((f"edge{j}", 52, [pair(j, dt, j % 5 == 0), pair(52 - 1 - j - dt, dt, j % 5 == 2)]))
    # --- the last frame of clip c against the first frame of clip c + 1: the same tile, no cell may see the other
    prev = None
    for j in range(8):
        s = next(seeds)
        items = [(13, s, ("exact",), [])]
        if prev is not None:
            items.append((0, prev, ("exact",), []))        # frame 0 = clip j - 1's last frame (cross_patch perturbs some)
        clips.append((f"cross{j}", 14, items))
        prev = s
    # --- chains of 3, 8 and 21 tied cells per bin inside one window
    clips.append(("chain3", 40, [(12, next(seeds), ("exact",), [17, 22])]))
    clips.append(("chain8", 40, [(14, next(seeds), ("period", 7), [])]))
    clips.append(("chain21", 60, [(18, next(seeds), ("period", 20), [])]))
    # ... and the same with one count on the last copy: cells within a key step or two whose fp64 powers DIFFER, so the
    # verification kernel has to find the one maximum among 3 / 8 / 21 recomputed cells (some members are peaks, some not)
    clips.append(("chain3p", 40, [(12, next(seeds), ("last", 200), [17, 22])]))
    clips.append(("chain8p", 40, [(14, next(seeds), ("period", 7, 250), [])]))
    clips.append(("chain21p", 60, [(18, next(seeds), ("period", 20, 250), [])]))
    # --- ulp-level ties: reversed tile (same bin), alternating-sign tile (bin f -> 2048 - f; j = 6 is just outside)
    items = [(5 + 24 * q, next(seeds), ("rev",), [5 + 24 * q + 2 + (3 * q) % 9]) for q in range(6)]
    clips.append(("rev", 160, items))
    items = [(5 + 24 * j, ALT_SEEDS[j], ("alt",), [5 + 24 * j + 2 + (2 * j) % 9]) for j in range(7)]
    clips.append(("alt", 180, items))
    # --- ties inside one row: bins 1024 - j and 1024 + j of one frame
    items = [(3 + 15 * q, sd, ("sym", n), []) for q, (sd, n) in enumerate(SYM_SEEDS)]
    clips.append(("inrow", 3 + 15 * len(SYM_SEEDS), items))
    # --- ... a few fp64 ulp apart, on opposite sides of an fp32 rounding boundary
    items = [(3 + 15 * q, sd, ("symfix", samples), []) for q, (sd, samples) in enumerate(STRADDLE)]
    clips.append(("straddle", 3 + 15 * len(STRADDLE), items))
    return clips


def cross_patch(clips_pcm, names):
    """cross{j}: one count on a sample of clip j's FIRST frame for odd j, so that the pair (clip j - 1 last frame, clip j
    first frame) is a perturbed tie as well as an exact one."""
    for x, n in zip(clips_pcm, names):
        if n.startswith("cross") and int(n[5:]) % 2 == 1:
            x[STEP_SAMPLES[int(n[5:]) % 4]] += 1


def crafted_clips():
    """(names, [pcm], plan)"""
    p = plan()
    pcm = [build_clip(nf, items, bg_clip=i) for i, (_, nf, items) in enumerate(p)]
    names = [n for n, _, _ in p]
    cross_patch(pcm, names)
    return names, pcm, p


def click_per_hop(n_frames: int = 40) -> np.ndarray:
    """A click every hop: flat spectra, every cell of a window within the top fp32 steps -- far more than PV_MAX_NEAR."""
    x = np.zeros(HOP * (n_frames - 1) + NFFT, np.int16)
    x[::HOP] = 20000
    return x


# ---------------------------------------------------------------------------------------------------- the reference
def db_exact(P: np.ndarray) -> np.ndarray:
    """10 log10(P), correctly rounded (the library's HOST function shz_db_values); zero power -> 0.0 (cpu_ref.log_db)."""
    from shazam_amd import _ffi
    P = np.ascontiguousarray(P, np.float64)
    nz = P != 0
    v = np.ascontiguousarray(P[nz])
    out = np.empty_like(v)
    if v.size:
        assert _ffi.lib().shz_db_values(v.ctypes.data_as(C.c_void_p), v.size, out.ctypes.data_as(C.c_void_p)) == 0
    A = np.zeros_like(P)
    A[nz] = out
    return A


def psd_exact_frames(x, fused: bool = True) -> np.ndarray:
    """np_exact.psd_exact(x, 44100, 2048), frame by frame; frames with the same 4,096 samples (the copies of a tile) are
    transformed once."""
    x = np.asarray(x)
    if len(x) < NFFT:
        return E.psd_exact(x, 44100, HOP, NFFT, fused)
    frames = np.lib.stride_tricks.sliding_window_view(x, NFFT)[::HOP]
    out, seen = np.empty((NBINS, frames.shape[0])), {}
    for f, fr in enumerate(frames):
        key = fr.tobytes()
        if key not in seen:
            seen[key] = f
            out[:, f] = E.psd_exact(fr, 44100, HOP, NFFT, fused)[:, 0]
        else:
            out[:, f] = out[:, seen[key]]
    return out


def reference(x, amp_min: float = 10.0, fan_value: int = 5, fused: bool = True):
    """(peak_f, peak_t, key32, t1, P): what the reference computes for one clip, with no rounding left to chance."""
    P = psd_exact_frames(x, fused)
    A = db_exact(P)
    f, t = O.sort_peaks(*O.peaks_2d(A, amp_min))
    k, t1 = O.pair_keys(f, t, fan_value)
    return f, t, k, t1, P


# ------------------------------------------------------------------------------------------------------- coverage
BIN_CLASSES = ("first10", "last10", "slab_edge", "wave_seam", "elsewhere")


def bin_class(f: int) -> str:
    """Where bin f sits in peak_pick32's geometry: slabs of 105 bins, two waves per slab; wave 1's first output column is
    slab bin 51, and the output columns 41..61 are those whose 21-bin window spans it."""
    if f < 10:
        return "first10"
    if f >= NBINS - 10:
        return "last10"
    m = f % SLAB
    if m < 10 or m >= SLAB - 10:
        return "slab_edge"
    if 41 <= m <= 61:
        return "wave_seam"
    return "elsewhere"


def decisive_windows(P: np.ndarray, amp_min_power: float = 10.0):
    """Windows (centre cells) that hold their 21x21 window's largest fp32 key, clear 10 dB, and have a second cell within
    4 key steps: list of (f, t, step, f2, t2), (f2, t2) the nearest-in-key other cell (ties: the first in frame order)."""
    K = np.float32(P).view(np.int32).astype(np.float64)     # (keys are below 2^31: exact in fp64)
    M = O._running_max(O._running_max(K, 10, 0), 10, 1)
    out = []
    for f, t in zip(*np.where((K == M) & (P > amp_min_power))):
        f0, t0 = max(f - 10, 0), max(t - 10, 0)
        w = K[f0:f + 11, t0:t + 11].copy()
        w[f - f0, t - t0] = -1
        j = int(np.argmax(w.T))                # frame-major: the earliest frame among equals
        t2, f2 = divmod(j, w.shape[0])
        step = int(K[f, t] - w[f2, t2])
        if step <= 4:
            out.append((int(f), int(t), step, int(f2 + f0), int(t2 + t0)))
    return out


def coverage(windows_per_clip):
    """Counts for the conditions the tests assert: {(step, bin class)}, {(step, dt)}, {(step, boundary)}."""
    by_pos, by_dt, by_b = {}, {}, {}
    for wins in windows_per_clip:
        for f, t, step, f2, t2 in wins:
            by_pos[(step, bin_class(f))] = by_pos.get((step, bin_class(f)), 0) + 1
            if f2 == f and t2 != t:
                by_dt[(step, abs(t2 - t))] = by_dt.get((step, abs(t2 - t)), 0) + 1
                for B in BOUNDARIES:
                    if min(t, t2) < B <= max(t, t2):
                        by_b[(step, B)] = by_b.get((step, B), 0) + 1
    return by_pos, by_dt, by_b


def chain_mixed_bins(item, ref):
    """Bins of a chain item in which all the chain's cells lie within two fp32 key steps of their maximum (one window of
    peak_verify holds them all) while the reference makes some of them peaks and some not: (mixed bins, all-peak bins)."""
    f, t, _, _, P = ref
    fr = item_frames(item)
    K = np.float32(P[:, fr]).view(np.int32).astype(np.int64)
    pk = np.zeros(P.shape, bool)
    pk[f, t] = True
    n_pk = pk[:, fr].sum(1)
    near = (K.max(1) - K.min(1)) <= 2
    return np.where(near & (n_pk > 0) & (n_pk < len(fr)))[0].tolist(), np.where(near & (n_pk == len(fr)))[0].tolist()


def straddling_pairs(plan_items, ref):
    """Items of the "straddle" clip whose cells 1024 - j and 1024 + j hold fp32 keys ONE step apart and are both peaks of
    the reference: [(frame, lower-key bin, higher-key bin)]."""
    f, t, _, _, P = ref
    pk = set(zip(f.tolist(), t.tolist()))
    K = np.float32(P).view(np.int32)
    out = []
    for it in plan_items:
        a = it[0]
        j = abs(1004 + int(np.argmax(P[1004:1045, a])) - 1024)
        lo, hi = sorted((1024 - j, 1024 + j), key=lambda b: K[b, a])
        if j and int(K[hi, a]) - int(K[lo, a]) == 1 and (lo, a) in pk and (hi, a) in pk:
            out.append((a, lo, hi))
    return out
