"""Built inputs for the k-way run merge of the bulk build (shz_build.hip: kw_*_kernel, seal_rows, kway_merge,
collapse_runs, flush_runs) and a numpy model of its PLAN.  Not collected by pytest; used by test_kway_plan_model.py
(no GPU) and test_gpu_kway_built.py.

The definition of a table is `expected`: np.unique over the packed 64-bit rows.  All arithmetic is integer arithmetic,
nothing here has a tolerance.  The model (`plan_model`, `thread_regions`) never decides whether a table is right: it
tells a built case whether it reaches the path it was built for."""
from types import SimpleNamespace

import numpy as np

# ---- constants copied from shz_build.hip: when the plan changes, the guards of the built cases fail and point here ----
KW_MAXK = 32              # runs one merge takes
KW_THREADS = 256          # threads of kw_tile_kernel
KW_TILE_SMALL = 1024      # nominal tile rows for kp2 <= KW_SMALL_MAX_KP2 ...
KW_TILE_LARGE = 2048      # ... and above
KW_SMALL_MAX_KP2 = 16
KW_BUF_TILES = 3          # the LDS buffer holds KW_BUF_TILES x TILE rows
KW_PIECE_DIV = 8          # nominal <= piece_rows / KW_PIECE_DIV (but >= kp2)
SEG_ROWS_DEFAULT = 1 << 31   # shz_table's seg_limit when set_segment_rows was not called
MAX_SEGS = 32             # SHZ_MAX_SEGS

OB = 12                   # offset bits of the built cases (every case holds one offset 2^OB - 1, so the table derives OB)


# ---- packed rows <-> columns ----
def pack(k, s, o, ob=OB):
    """(key, sid, off) columns -> packed uint64 rows of the run layout: key << 32 | sid << ob | off (sb = 32 - ob)"""
    k, s, o = (np.asarray(a, np.uint64) for a in (k, s, o))
    assert (s < (1 << (32 - ob))).all() and (o < (1 << ob)).all() and (k < (1 << 32)).all()
    return (k << np.uint64(32)) | (s << np.uint64(ob)) | o


def rows_of(values, ob=OB):
    """packed uint64 rows -> (key, sid, off) uint32 columns"""
    v = np.asarray(values, np.uint64)
    return ((v >> np.uint64(32)).astype(np.uint32), ((v & np.uint64(0xFFFFFFFF)) >> np.uint64(ob)).astype(np.uint32),
            (v & np.uint64((1 << ob) - 1)).astype(np.uint32))


def sealed(cols, ob=OB):
    """what seal_rows leaves of one run: its packed rows, sorted, each once"""
    return np.unique(pack(*cols, ob))


def expected(runs, ob=OB):
    """THE definition: the table of the runs (columns of every run) = np.unique over the packed rows of all of them.
    Returns the three uint32 columns in table order."""
    runs = [r for r in runs if len(r[0])]
    if not runs:
        return rows_of(np.empty(0, np.uint64), ob)
    return rows_of(np.unique(np.concatenate([pack(*r, ob) for r in runs])), ob)


def staged(runs):
    """the runs as one block of staged rows + the block sizes finalize_runs takes"""
    k, s, o = (np.concatenate([np.asarray(r[i], np.uint32) for r in runs]) for i in range(3))
    return k, s, o, [len(r[0]) for r in runs]


def holds_layout(runs, ob=OB):
    """the table derives ob from the largest offset it sees: some row must hold 2^ob - 1 (and every sid fit 32 - ob bits)"""
    o = np.concatenate([np.asarray(r[2], np.uint64) for r in runs])
    s = np.concatenate([np.asarray(r[1], np.uint64) for r in runs])
    return int(o.max()) == (1 << ob) - 1 and int(s.max()) < (1 << (32 - ob))


# ---- the plan of kway_merge, in numpy ----
def plan_model(runs, piece_rows=SEG_ROWS_DEFAULT):
    """runs: the SEALED runs (sorted packed uint64, `sealed`), empty ones make no run, at most KW_MAXK.
    -> kp2, tile, nominal, M, c, samples (sorted), ntiles, bounds[ntiles + 1, k], shares[ntiles, k], tile_rows[ntiles]"""
    runs = [np.asarray(r, np.uint64) for r in runs if len(r)]
    k = len(runs)
    assert 1 <= k <= KW_MAXK
    kp2 = 1
    while kp2 < k:
        kp2 <<= 1
    tile = KW_TILE_SMALL if kp2 <= KW_SMALL_MAX_KP2 else KW_TILE_LARGE
    nominal = min(tile, max(kp2, piece_rows // KW_PIECE_DIV))
    M, c = max(1, nominal // kp2), kp2
    samples = np.sort(np.concatenate([r[::M] for r in runs]))          # ceil(n / M) samples a run
    ntiles = -(-len(samples) // c)
    bounds = np.zeros((ntiles + 1, k), np.int64)
    split = samples[c::c][:ntiles - 1]                                  # tile t >= 1 starts at the value samples[t * c]
    for r, run in enumerate(runs):
        bounds[1:ntiles, r] = np.searchsorted(run, split, side="left")  # every copy of a value goes to one tile
        bounds[ntiles, r] = len(run)
    shares = np.diff(bounds, axis=0)
    return SimpleNamespace(k=k, kp2=kp2, tile=tile, nominal=nominal, M=M, c=c, samples=samples, ntiles=ntiles, split=split,
                           bounds=bounds, shares=shares, tile_rows=shares.sum(1), buf_rows=KW_BUF_TILES * tile)


def thread_regions(plan):
    """per tile: the largest number of (non-empty) merge regions of the FIRST round -- runs (0, 1), (2, 3), ... -- that the
    output range [tid * per, tid * per + per) of one thread touches (the pieces of kw_tile_kernel's `while (g < g1)`)"""
    out = np.zeros(plan.ntiles, np.int64)
    for t in range(plan.ntiles):
        s_off = np.r_[0, np.cumsum(plan.shares[t])]
        total = min(int(s_off[-1]), plan.buf_rows)
        if total == 0:
            continue
        edges = np.unique(np.minimum(np.r_[s_off[0:plan.k:2], s_off[plan.k]], total))   # ends of the non-empty regions
        per = -(-total // KW_THREADS)
        g0 = np.minimum(np.arange(KW_THREADS) * per, total)
        g1 = np.minimum(g0 + per, total)
        live = g1 > g0
        first = np.searchsorted(edges, g0[live], side="right") - 1
        last = np.searchsorted(edges, g1[live] - 1, side="right") - 1
        out[t] = int((last - first + 1).max())
    return out


def fill(plan):
    """rows of the fullest tile, in units of the nominal tile"""
    return float(plan.tile_rows.max()) / plan.tile


def splitter_ties(plan):
    """per splitter: how many samples hold its value"""
    return np.array([int((plan.samples == v).sum()) for v in plan.split], np.int64)


# ---- rows ----
def _keys(rng, m, key_vals):
    return (rng.integers(0, key_vals, m).astype(np.uint64) << np.uint64(8)) | rng.integers(0, 4, m).astype(np.uint64)


def draw(rng, n, sid_lo, sid_hi, ob=OB, key_vals=1 << 16, keys=None, top=False, avoid=None):
    """n DISTINCT rows (packed, in random order): keys of `key_vals` bucket values x 4 (or drawn from `keys`), sids in
    [sid_lo, sid_hi), any offset.  top: the first row's offset is 2^ob - 1.  avoid: packed rows that must not come up."""
    mask = np.uint64((1 << ob) - 1)
    v = np.empty(0, np.uint64)
    while True:
        m = 2 * (n - len(v)) + 8
        k = _keys(rng, m, key_vals) if keys is None else np.asarray(keys, np.uint64)[rng.integers(0, len(keys), m)]
        new = pack(k, rng.integers(sid_lo, sid_hi, m), rng.integers(0, 1 << ob, m), ob)
        v = np.unique(np.concatenate([v, new]))
        if avoid is not None:
            v = np.setdiff1d(v, avoid)
        if len(v) < n:
            continue
        v = rng.permutation(v)[:n]
        if top and n:
            v[0] |= mask
        if len(np.unique(v)) == n and (avoid is None or not np.isin(v, avoid).any()):
            return v
        v = np.unique(v)[:max(n - 4, 0)]


def mixed(rng, n, src, sid_lo, sid_hi, share=0.5, **kw):
    """n distinct rows in random order, about `share` of them rows of `src` (rows repeated across runs), the others new"""
    m = min(int(round(n * share)), len(src), n)
    if n == 1:
        m = int(rng.integers(0, 2)) if len(src) else 0
    old = rng.choice(src, m, replace=False) if m else np.empty(0, np.uint64)
    new = draw(rng, n - m, sid_lo, sid_hi, avoid=src, **kw)
    return rng.permutation(np.concatenate([old, new]).astype(np.uint64))


def _cols(runs, ob=OB):
    return [rows_of(v, ob) for v in runs]


def run_sizes(seed, k, lo=200, hi=3000):
    """unequal run lengths (the collapse beyond KW_MAXK runs picks the smallest)"""
    return [int(x) for x in np.random.default_rng(1000 + seed).integers(lo, hi, k)]


def random_runs(seed, sizes, dedup, ob=OB, key_vals=1 << 16):
    """runs of random distinct rows.  dedup False: run r owns the song ids [1 + 4 r, 5 + 4 r) -- no row can repeat, the
    merge does not look for duplicates.  True: every run draws from the same ids and about a third of a run's rows are
    rows of the run before it and of run 0."""
    rng = np.random.default_rng(seed)
    runs = []
    for r, n in enumerate(sizes):
        top = n > 0 and not any(len(x) for x in runs)
        if not dedup:
            v = draw(rng, n, 1 + 4 * r, 5 + 4 * r, ob, key_vals, top=top)
        elif not any(len(x) for x in runs) or n == 0:
            v = draw(rng, n, 1, 40, ob, key_vals, top=top)
        else:
            src = np.unique(np.concatenate([runs[-1], next(x for x in runs if len(x))]))
            v = mixed(rng, n, src, 1, 40, share=0.35, ob=ob, key_vals=key_vals)
        runs.append(v)
    if not any(((v & np.uint64((1 << ob) - 1)) == (1 << ob) - 1).any() for v in runs if len(v)):
        raise AssertionError("no row with the top offset")
    return _cols(runs, ob)


def skewed_runs(seed, big_pos, dedup, k=32, big=60000, small=96, ob=OB):
    """one run of `big` rows at position big_pos beside k - 1 runs of `small` rows, all over the same key range: a tile
    holds a few rows of every small run, and a thread's outputs cross several merge regions"""
    rng = np.random.default_rng(seed)
    kv = 1 << 20
    main = draw(rng, big, 1, 5, ob, kv, top=True)
    runs = []
    for r in range(k):
        if r == big_pos:
            runs.append(main)
        elif dedup:
            runs.append(mixed(rng, small, main, 1, 5, share=0.5, ob=ob, key_vals=kv))
        else:
            runs.append(draw(rng, small, 8 + 4 * r, 12 + 4 * r, ob, kv))
    return _cols(runs, ob)


def comb_runs(k, dedup, periods=3, seed=0, ob=OB):
    """The comb: full tiles.  k a power of two (c = k samples a tile, stride M = tile / k).  In every period of the key
    space run 0 puts c M keys inside a window; every other run puts one key just below the window and M - 1 keys inside
    it.  Run 0 starts with M keys below everything, so that the first sample inside the first window starts a tile: that
    tile holds the window, c M + (k - 1)(M - 1) rows.  Order is carried by the key (one row a key and run); the offset
    is a function of the key.  dedup False: a run's sid is its own.  True: all share sid 1 and the other runs' window
    keys are partly run 0's (duplicates inside the full tile)."""
    assert k & (k - 1) == 0 and 2 <= k <= KW_MAXK
    rng = np.random.default_rng(seed)
    tile = KW_TILE_SMALL if k <= KW_SMALL_MAX_KP2 else KW_TILE_LARGE
    M, c = tile // k, k
    span = k + 2 * c * M + 64
    mask = (1 << ob) - 1
    keys = [[np.arange(M, dtype=np.uint64)] if r == 0 else [] for r in range(k)]
    for p in range(periods):
        base = (p + 1) * span
        keys[0].append(base + k + 2 * np.arange(c * M, dtype=np.uint64))
        for r in range(1, k):
            slots = rng.choice(np.arange(1, 2 * c * M), M - 1, replace=False).astype(np.uint64)
            keys[r].append(np.r_[np.uint64(base + r), base + k + slots].astype(np.uint64))
    runs = []
    for r in range(k):
        key = rng.permutation(np.concatenate(keys[r]).astype(np.uint64))
        off = np.where(key == 0, mask, (key * np.uint64(40503) >> np.uint64(3)) & np.uint64(mask))
        sid = np.full(len(key), 1 if dedup else r + 1, np.uint64)
        runs.append((key.astype(np.uint32), sid.astype(np.uint32), off.astype(np.uint32)))
    return runs


def comb_full_tile_rows(k):
    tile = KW_TILE_SMALL if k <= KW_SMALL_MAX_KP2 else KW_TILE_LARGE
    M = tile // k
    return k * M + (k - 1) * (M - 1)


def disjoint_runs(seed, k, descending, dedup, ob=OB):
    """run r holds only keys of range r (descending: of range k - 1 - r, run 0 the largest keys); unequal lengths"""
    rng = np.random.default_rng(seed)
    runs = []
    for r, n in enumerate(run_sizes(seed, k)):
        j = k - 1 - r if descending else r
        pool = (np.uint64(j) << np.uint64(16)) | np.arange(1 << 12, dtype=np.uint64)
        lo, hi = (1, 40) if dedup else (1 + 4 * r, 5 + 4 * r)
        runs.append(draw(rng, n, lo, hi, ob, keys=pool, top=r == 0))
    return _cols(runs, ob)


def same_rows_runs(seed, k, n=3000, ob=OB):
    """every run holds the same rows (each in its own order): the table is one copy, all k samples tie at every splitter"""
    rng = np.random.default_rng(seed)
    v = draw(rng, n, 1, 40, ob, top=True)
    return _cols([rng.permutation(v) for _ in range(k)], ob)


def same_pairs_runs(seed, k, n=3000, ob=OB):
    """every run holds the same (key, offset) pairs under its own song id: nothing is dropped, groups of k neighbours
    differ in the sid bits only"""
    rng = np.random.default_rng(seed)
    key = rng.choice(1 << 24, n, replace=False).astype(np.uint32) << np.uint32(2)     # one pair a key
    off = rng.integers(0, 1 << ob, n).astype(np.uint32)
    off[0] = (1 << ob) - 1
    runs = []
    for r in range(k):
        p = rng.permutation(len(key))
        runs.append((key[p], np.full(len(p), r + 1, np.uint32), off[p]))
    return runs


def one_key_runs(seed, k, dedup, key=0x00ABCDEF, ob=OB):
    """one key for all rows of all runs: order and ties sit in the sid and offset bits alone"""
    rng = np.random.default_rng(seed)
    runs = []
    for r, n in enumerate(run_sizes(seed, k, 200, 1500)):
        if not dedup:
            runs.append(draw(rng, n, 1 + 4 * r, 5 + 4 * r, ob, keys=[key], top=r == 0))
        elif r == 0:
            runs.append(draw(rng, n, 1, 40, ob, keys=[key], top=True))
        else:
            runs.append(mixed(rng, n, np.unique(np.concatenate(runs)), 1, 40, share=0.4, ob=ob, keys=[key]))
    return _cols(runs, ob)


def stride_runs(seed, M, dedup, more=0, big=5000, ob=OB):
    """runs of 1, M - 1, M, M + 1, 2 M and 2 M + 1 rows (kw_sample_kernel takes ceil(n / M) samples) and `more` runs of 150,
    beside one run of `big` rows.  The lengths are the sealed ones: a run's rows are distinct."""
    rng = np.random.default_rng(seed)
    lens = [1, M - 1, M, M + 1, 2 * M, 2 * M + 1] + [150] * more
    main = draw(rng, big, 1, 40, ob, top=True)
    runs = [mixed(rng, n, main, 1, 40, share=0.5, ob=ob) if dedup else draw(rng, n, 50 + 4 * r, 54 + 4 * r, ob)
            for r, n in enumerate(lens)]
    at = int(rng.integers(0, len(runs) + 1))
    runs.insert(at, main)
    return _cols(runs, ob), lens[:at] + [big] + lens[at:]


def single_row_runs(seed, singles, big, dedup, ob=OB):
    """`singles` runs of one row each, beside one run of `big` rows if big"""
    rng = np.random.default_rng(seed)
    main = draw(rng, max(big, 1), 1, 40, ob, top=True)
    runs = []
    for r in range(singles):
        if dedup:      # every third single row is a row of the large run, or the single row before it
            src = main if big else (runs[-1] if runs else main)
            runs.append(src[rng.integers(0, len(src), 1)] if r % 3 == 1 else draw(rng, 1, 1, 40, ob))
        else:
            runs.append(draw(rng, 1, 50 + r, 51 + r, ob))
    if big:
        runs.insert(int(rng.integers(0, singles + 1)), main)
    else:
        runs[0] = main[:1]
        if dedup:
            runs[1] = main[:1].copy()
    return _cols(runs, ob)


def range_end_runs(seed, ob=OB):
    """the two ends of the packed 64-bit range -- row (0, 0, 0) and the row whose packed value is 2^64 - 1 -- in
    different runs (0 and 1) and together in one (2), among other rows"""
    rng = np.random.default_rng(seed)
    lo, hi = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    body = [draw(rng, n, 0, 1 << (32 - ob), ob, key_vals=1 << 24) for n in (700, 1300, 400)]
    runs = [np.r_[lo, body[0]], np.r_[body[1], hi], np.r_[hi, body[2], lo, body[0][:50]]]
    return _cols([rng.permutation(v.astype(np.uint64)) for v in runs], ob)


def ordered_rows(seed, n, ob=OB, keys=(7 << 8, 9 << 8, (9 << 8) | 1)):
    """n distinct rows ordered by (song id, offset) -- the order ingest produces -- over three keys: the table's order
    inside a key is then the order the rows arrive in"""
    rng = np.random.default_rng(seed)
    lo = np.sort(rng.choice(np.arange(1 << ob, 40 << ob), n - 1, replace=False)).astype(np.uint64)
    lo = np.r_[lo, np.uint64((41 << ob) | ((1 << ob) - 1))]          # the last row holds the top offset
    key = np.asarray(keys, np.uint64)[rng.integers(0, len(keys), n)]
    return key, lo >> np.uint64(ob), lo & np.uint64((1 << ob) - 1)


def inverted_rows(seed, n, at, ob=OB):
    """ordered_rows with ONE inversion: rows at and at + 1 swapped, both under one key (so that only the full sort, not
    the stable sort on the key bits, puts them right)"""
    key, sid, off = ordered_rows(seed, n, ob)
    key[at + 1] = key[at]
    for a in (sid, off):
        a[at], a[at + 1] = a[at + 1], a[at]
    return key.astype(np.uint32), sid.astype(np.uint32), off.astype(np.uint32)


def descending_key_rows(seed, n, ob=OB):
    """ordered rows whose neighbours share (song id, offset) under descending keys: pairs (2 i, 2 i + 1) hold one
    (sid, off) with keys 9 << 8 and 7 << 8.  No row sorts before its predecessor by (sid, off): not an inversion."""
    key, sid, off = ordered_rows(seed, n // 2, ob)
    sid, off = np.repeat(sid, 2), np.repeat(off, 2)
    key = np.tile(np.array([9 << 8, 7 << 8], np.uint64), n // 2)
    return key.astype(np.uint32), sid.astype(np.uint32), off.astype(np.uint32)


def old_random_runs(seed, k, per=5000, ob=OB):
    """what the older tests feed the merge: k equal runs of uniformly random rows (test_gpu_merge_runs._rows)"""
    rng = np.random.default_rng(seed)
    runs = []
    for _ in range(k):
        key = rng.integers(0, 1 << 22, per).astype(np.uint32) << np.uint32(8) | rng.integers(0, 6, per).astype(np.uint32)
        runs.append((key, rng.integers(1, 300, per).astype(np.uint32), rng.integers(0, 4000, per).astype(np.uint32)))
    return runs
