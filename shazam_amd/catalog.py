"""The catalogue's own question: "which of my tracks are the same recording?" (csrc/shz_catalog.hip).

Everything else here answers "which song is this audio?".  A catalogue of 10^5 to 10^6 tracks holds re-uploads, the album
and the single cut, tracks inside compilations and sets, radio edits inside full versions.  The reference has no answer
beyond deleting files by hand; INSERT IGNORE protects only against the same file_sha1.  The table already holds what is
needed: a song's rows are a ready-made query.  shz_table_song_hashes gathers the rows of listed songs on the device,
shz_match_songs matches them against the rest of the table in the same call, and find_duplicates() walks a catalogue in
batches and folds the answers of both directions into one record per pair of songs.

A pair (a, b), a < b, is reported with delta = off_b - off_a (b's frame under a's frame 0), the aligned count, both row
counts and both coverages aligned / rows.  "same": both songs are covered; "a_in_b" / "b_in_a": one is (an excerpt inside a
longer track); "overlap": neither, but enough rows align.  The clusters of "same" are what delete_songs() wants.

Altered copies: a re-upload pitched up 3 %, a 25/24 video transfer, a rip from a drifting deck shares no
hash with its original.  With speeds= / tempos= / pitches= / warps= (the ladders of speed.py) every listed song's rows are
warped on the device at every rung (shz_match_songs_warps: a row is two peaks, both are moved and the key is formed again)
and matched; fold_pairs_warps keeps, per pair, the strongest observation over both sides and all rungs, and says which
song's rows were warped by which factors.  Votes are counted in ONE delta bin: a rung that misses the true factor by m
spreads a song of T frames over about T m bins, so long tracks want a finer ladder than short ones.

Where an altered copy overlaps its original: with extents="fit" the found pairs go through one more library
call (shz_match_songs_warps_extents: every pair's warped song is a JOB at the one warp the pair was found at, its candidate
the other song around the pair's delta), and pair_extents_warps turns the result into the span in both songs' own frames,
the rows aligned there and tempo_fit, the factor the copy really runs at between the rungs."""
from __future__ import annotations

import numpy as np

from ._ffi import takes_delta_tol

# Detection thresholds, set between the two distributions scripts/catalog_bench.py measured on the music-like synthetic
# corpus (10 s songs of about 3,180 rows): among 51,000 songs no unrelated pair aligned more than 59 rows or
# covered more than 0.027 of its smaller song; no planted copy or excerpt aligned fewer than 1,474 rows or covered less than
# 0.867 of its smaller song.  0.8 rather than the middle: "same" is what delete_songs() acts on, and an excerpt that lacks a
# fifth of the longer track should stay "a_in_b" / "b_in_a".  Not measured: re-encoded or noisy copies, tracks of minutes.
MIN_ALIGNED = 200
MIN_COVERAGE = 0.8
BATCH_ROWS = 1 << 22     # rows of the listed songs handed to one shz_match_songs call (with a ladder: rows x warps)
# Thresholds of the warped search, set between the two distributions scripts/catalog_speed_bench.py measured on an MI355X
# (4,000 music-like 10 s songs of about 3,190 rows, 80 copies resampled to speeds within +-5 %, the default
# ladder of 71 rungs, the best of every pair over ALL rungs and both sides): no unrelated pair aligned more than 54 rows or
# covered more than 0.018 of its smaller song; a planted copy ON a rung aligned at least 415 rows (coverage >= 0.131 of either
# song), one HALF A STEP (0.07 %) beside a rung at least 154 (coverage >= 0.046).  A warped copy is never covered like an exact
# one (resampling moves peaks), so "same" here means 0.03 of both songs, not 0.8.  The CPU oracle's figures for the 3-rung
# catalogue of tests/test_gpu_find_duplicates_warps.py agree: unrelated <= 22, planted >= 426, coverage >= 0.13 on the warped
# side.  A ladder gives every unrelated pair n_warps chances and both counts grow with the track: not measured on tracks of
# minutes, on ladders of hundreds of rungs, on codec or phase-vocoder output.
MIN_ALIGNED_WARPED = 100
MIN_COVERAGE_WARPED = 0.03

PAIR_FIELDS = (("a", np.uint32), ("b", np.uint32), ("delta", np.int64), ("aligned", np.uint32), ("rows_a", np.uint64),
               ("rows_b", np.uint64), ("coverage_a", np.float64), ("coverage_b", np.float64), ("relation", "U7"))
EXTENT_PAIR_FIELDS = PAIR_FIELDS + (("a_first", np.uint32), ("a_last", np.uint32), ("b_first", np.uint32), ("b_last", np.uint32))
WARP_PAIR_FIELDS = PAIR_FIELDS + (("tempo_q16", np.uint32), ("pitch_q16", np.uint32), ("warped", "U1"), ("aligned_plain", np.uint32))
WARP_EXTENT_PAIR_FIELDS = WARP_PAIR_FIELDS + (("a_first", np.uint32), ("a_last", np.uint32), ("b_first", np.uint32), ("b_last", np.uint32),
                                              ("count", np.uint32), ("warped_first", np.uint32), ("warped_last", np.uint32),
                                              ("tempo_fit", np.float64), ("drift_bins", np.uint32))
S_ONE = 65536


def _table_of(db_or_table):
    """(table, db or None): a HipFingerprintDB is finalized first; a sharded one has no song gather."""
    db = db_or_table if hasattr(db_or_table, "table") else None
    table = db.table if db is not None else db_or_table
    if not hasattr(table, "h"):
        raise NotImplementedError("the catalogue calls take the unsharded table (shards=1)")
    if db is not None:
        db.finalize()
    return table, db


def _ladder_of(speeds, tempos, pitches, warps):
    """None without a ladder keyword, else (t16, f16, row): the pair list as speed.recognize_speeds / recognize_warps read
    their arguments -- speeds= is the diagonal, tempos= with pitches= their product (warp_grid, tempo-major; a missing one
    is [65536]), warps=(t16, f16) an explicit pair list; row: pairs of one grid row (library calls take whole rows)."""
    from .speed import _check_speeds, warp_grid
    if speeds is None and tempos is None and pitches is None and warps is None:
        return None
    if speeds is not None:
        if tempos is not None or pitches is not None or warps is not None:
            raise TypeError("speeds= is one factor for both axes: it excludes tempos=, pitches= and warps=")
        sp = _check_speeds(speeds)
        return sp, sp.copy(), 1
    if warps is not None:
        if tempos is not None or pitches is not None:
            raise TypeError("warps= is an explicit pair list: it excludes tempos= and pitches=")
        t16, f16 = _check_speeds(warps[0], "warps[0]"), _check_speeds(warps[1], "warps[1]")
        if len(t16) != len(f16):
            raise ValueError("warps=(t16, f16): two lists of one length")
        return t16, f16, 1
    tl = np.asarray([S_ONE], np.uint32) if tempos is None else _check_speeds(tempos, "tempos")
    pl = np.asarray([S_ONE], np.uint32) if pitches is None else _check_speeds(pitches, "pitches")
    return (*warp_grid(tl, pl), max(len(pl), 1))


def _match_songs_warps(table, sids, t16, f16, row, topn, full_sort=False, timings=False):
    """Table.match_songs_warps over the whole pair list: lists longer than one library call (1,024 warps) go in chunks of
    whole rows and are put side by side along the warp axis.  timings: "ms" is summed over the chunks."""
    from .speed import warp_chunks
    parts = [table.match_songs_warps(sids, t16[a:b], f16[a:b], topn=topn, full_sort=full_sort, timings=timings)
             for a, b in warp_chunks(len(t16), row)]
    if not parts:
        raise ValueError("the ladder is empty")
    out = {f: np.concatenate([p[f] for p in parts], axis=1) for f in ("sid", "delta", "aligned", "dedup", "nres", "nhash", "npairs")}
    out["rows"] = parts[0]["rows"]
    if timings:
        out["ms"] = tuple(np.sum([p["ms"] for p in parts], axis=0).tolist())
    return out


@takes_delta_tol(lambda *a, **k: (lambda x: x.ctx)(k["db_or_table"] if "db_or_table" in k else a[0]))
def match_songs(db_or_table, sids, topn: int = 5, full_sort: bool = False, speeds=None, tempos=None, pitches=None,
                warps=None) -> dict:
    """Every listed song matched against the rest of the table in one library call (shz_match_songs): the arrays of
    Table.match with one query per listed song and the song itself left out (sid, delta, aligned, dedup [n, topn]; nres,
    nhash, npairs [n]), plus rows [n], the songs' row counts.  delta is the found song's frame under the listed song's
    frame 0.
    With a ladder (speeds= / tempos= + pitches= / warps=, Q16 as in speed.py) every song's rows are warped at every pair
    first (shz_match_songs_warps): the arrays gain a warp axis behind the song axis ([n, n_warps, topn] / [n, n_warps]),
    "tempo_q16" / "pitch_q16" [n_warps] name the pairs, rows stay the unwarped counts, nhash is the distinct warped rows
    and delta is the found song's frame under the listed song's WARPED frame 0.
    delta_tol= (keyword): the vote tolerance in offset bins while the call runs (Context.tolerance); None: the context's.
    A song filter is taken from the context: run the call inside `with ctx.songs(only=...)` / `ctx.songs(exclude=...)` to match
    within / without a set of songs (every variant, every listed song uses the one set).
    The key cap is taken from the context too: run the call inside `with ctx.key_cap(rows):` to leave out the keys that hold
    more than `rows` table rows (Context.key_cap)."""
    table, _ = _table_of(db_or_table)
    lad = _ladder_of(speeds, tempos, pitches, warps)
    if lad is None:
        return table.match_songs(sids, topn=topn, full_sort=full_sort)
    t16, f16, row = lad
    out = _match_songs_warps(table, sids, t16, f16, row, topn, full_sort)
    out["tempo_q16"], out["pitch_q16"] = t16, f16
    return out


def _clusters(a: np.ndarray, b: np.ndarray) -> list:
    """Connected components of the edges (a[i], b[i]), each sorted by id, in the order of their smallest ids."""
    if len(a) == 0:
        return []
    ids = np.unique(np.concatenate([a, b]))
    ia, ib = np.searchsorted(ids, a), np.searchsorted(ids, b)
    label = np.arange(len(ids))
    while True:   # every node takes the smallest label among its neighbours until nothing moves
        low = np.minimum(label[ia], label[ib])
        new = label.copy()
        np.minimum.at(new, ia, low)
        np.minimum.at(new, ib, low)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    order = np.argsort(label, kind="stable")
    cuts = np.flatnonzero(np.diff(label[order])) + 1
    return [[int(x) for x in ids[g]] for g in np.split(order, cuts)]


def fold_pairs(sids, sid, delta, aligned, nres, song_ids, song_rows, min_aligned, min_coverage) -> dict:
    """The answers of match_songs folded into one record per unordered pair of songs -- plain numpy, no GPU.

    sids [n]: the listed songs; sid / delta / aligned [n, topn], nres [n]: what match_songs said about each (several
    batches: concatenated).  song_ids / song_rows: the row count of every song that occurs, listed or found.
    Returns {"pairs": structured array of PAIR_FIELDS ordered by (a, b), "clusters": list of id lists}.
    A pair both of whose songs were listed is seen from both sides: a's side is kept (the sides agree on the aligned
    count, not necessarily on which of two tied deltas they name).  Seen from b, delta changes its sign.  Pairs with
    aligned < min_aligned are dropped; coverage >= min_coverage counts as covered."""
    sids = np.asarray(sids, np.int64).reshape(-1)
    nres = np.asarray(nres, np.int64).reshape(-1)
    n = len(sids)
    if n == 0:
        return {"pairs": np.zeros(0, np.dtype(list(PAIR_FIELDS))), "clusters": []}
    sid = np.asarray(sid, np.int64).reshape(n, -1)
    delta = np.asarray(delta, np.int64).reshape(n, -1)
    aligned = np.asarray(aligned, np.int64).reshape(n, -1)
    valid = np.arange(sid.shape[1])[None, :] < nres[:, None]
    me = np.broadcast_to(sids[:, None], sid.shape)[valid]
    other, d, al = sid[valid], delta[valid], aligned[valid]
    keep = (al >= min_aligned) & (me != other)
    me, other, d, al = me[keep], other[keep], d[keep], al[keep]
    mine = me < other                               # the listed song is a: its side, delta as reported
    a, b = np.where(mine, me, other), np.where(mine, other, me)
    d = np.where(mine, d, -d)
    order = np.lexsort((~mine, b, a))               # per (a, b): a's side first
    a, b, d, al = a[order], b[order], d[order], al[order]
    first = np.ones(len(a), bool)
    first[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    a, b, d, al = a[first], b[first], d[first], al[first]
    ids = np.asarray(song_ids, np.int64).reshape(-1)
    rows = np.asarray(song_rows, np.uint64).reshape(-1)
    by = np.argsort(ids, kind="stable")
    ids, rows = ids[by], rows[by]

    def rows_of(x):
        at = np.searchsorted(ids, x)
        if len(x) and (at.max(initial=0) >= len(ids) or not np.array_equal(ids[at], x)):
            raise ValueError("fold_pairs: a song without a row count")
        return rows[at] if len(x) else np.zeros(0, np.uint64)

    pairs = np.zeros(len(a), np.dtype(list(PAIR_FIELDS)))
    pairs["a"], pairs["b"], pairs["delta"], pairs["aligned"] = a, b, d, al
    pairs["rows_a"], pairs["rows_b"] = rows_of(a), rows_of(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        pairs["coverage_a"] = al / pairs["rows_a"].astype(np.float64)
        pairs["coverage_b"] = al / pairs["rows_b"].astype(np.float64)
    ca, cb = pairs["coverage_a"] >= min_coverage, pairs["coverage_b"] >= min_coverage
    pairs["relation"] = np.where(ca & cb, "same", np.where(ca, "a_in_b", np.where(cb, "b_in_a", "overlap")))
    same = pairs["relation"] == "same"
    return {"pairs": pairs, "clusters": _clusters(pairs["a"][same], pairs["b"][same])}


def _rows_lookup(song_ids, song_rows, who):
    ids = np.asarray(song_ids, np.int64).reshape(-1)
    rows = np.asarray(song_rows, np.uint64).reshape(-1)
    by = np.argsort(ids, kind="stable")
    ids, rows = ids[by], rows[by]

    def rows_of(x):
        at = np.searchsorted(ids, x)
        if len(x) and (at.max(initial=0) >= len(ids) or not np.array_equal(ids[at], x)):
            raise ValueError(f"{who}: a song without a row count")
        return rows[at] if len(x) else np.zeros(0, np.uint64)

    return rows_of


def fold_pairs_warps(sids, tempo_q16, pitch_q16, sid, delta, aligned, nres, song_ids, song_rows,
                     min_aligned=MIN_ALIGNED_WARPED, min_coverage=MIN_COVERAGE_WARPED) -> dict:
    """The answers of match_songs at a ladder folded into one record per unordered pair of songs -- plain numpy, no GPU.

    sids [n]: the listed songs; tempo_q16 / pitch_q16 [K]: the warps; sid / delta / aligned [n, K, topn], nres [n, K]: what
    match_songs said about every (song, warp).  song_ids / song_rows: the plain row count of every song that occurs.
    Returns {"pairs": structured array of WARP_PAIR_FIELDS ordered by (a, b), "clusters": list of id lists}.
    Every (listed song, warp, rank) is an OBSERVATION of the pair it names.  Per pair a < b the kept observation is the one
    with the greatest aligned count over both sides and all warps; ties go to the smaller |t16 - 65536| + |f16 - 65536|, then
    to a's side, then to the lower warp index.  tempo_q16 / pitch_q16 are that observation's warp and warped says whose rows
    it warped ("a" or "b": that song runs t16 / 65536 times as fast and sounds f16 / 65536 times as high as the other).
    delta is as that side reported it -- the other song's frame under the warped song's WARPED frame 0 -- with the sign
    turned when the side is b.  aligned_plain: the pair's greatest count at the warp (65536, 65536) if the ladder holds
    it, else 0 -- what the plain find_duplicates would have seen.  Coverages are aligned / rows with the PLAIN row counts.
    Pairs with aligned < min_aligned are dropped; relations and clusters as in fold_pairs."""
    dt = np.dtype(list(WARP_PAIR_FIELDS))
    sids = np.asarray(sids, np.int64).reshape(-1)
    t16, f16 = np.asarray(tempo_q16, np.int64).reshape(-1), np.asarray(pitch_q16, np.int64).reshape(-1)
    n, K = len(sids), len(t16)
    if len(f16) != K:
        raise ValueError("tempo_q16 and pitch_q16 are two lists of one length")
    if n == 0 or K == 0:
        return {"pairs": np.zeros(0, dt), "clusters": []}
    sid = np.asarray(sid, np.int64).reshape(n, K, -1)
    delta = np.asarray(delta, np.int64).reshape(n, K, -1)
    aligned = np.asarray(aligned, np.int64).reshape(n, K, -1)
    nres = np.asarray(nres, np.int64).reshape(n, K)
    valid = np.arange(sid.shape[2])[None, None, :] < nres[:, :, None]
    me = np.broadcast_to(sids[:, None, None], sid.shape)[valid]
    v = np.broadcast_to(np.arange(K)[None, :, None], sid.shape)[valid]
    other, d, al = sid[valid], delta[valid], aligned[valid]
    keep = me != other
    me, v, other, d, al = me[keep], v[keep], other[keep], d[keep], al[keep]
    mine = me < other                               # the listed (warped) song is a: its side, delta as reported
    a, b = np.where(mine, me, other), np.where(mine, other, me)
    d = np.where(mine, d, -d)
    dist = np.abs(t16 - S_ONE) + np.abs(f16 - S_ONE)
    plain = np.where(dist[v] == 0, al, 0)
    order = np.lexsort((v, ~mine, dist[v], -al, b, a))   # per (a, b): the kept observation first
    a, b, d, al, v, mine, plain = a[order], b[order], d[order], al[order], v[order], mine[order], plain[order]
    first = np.ones(len(a), bool)
    first[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    start = np.flatnonzero(first)
    plain = np.maximum.reduceat(plain, start) if len(start) else plain[:0]
    a, b, d, al, v, mine = a[first], b[first], d[first], al[first], v[first], mine[first]
    ok = al >= min_aligned
    a, b, d, al, v, mine, plain = a[ok], b[ok], d[ok], al[ok], v[ok], mine[ok], plain[ok]
    rows_of = _rows_lookup(song_ids, song_rows, "fold_pairs_warps")
    pairs = np.zeros(len(a), dt)
    pairs["a"], pairs["b"], pairs["delta"], pairs["aligned"] = a, b, d, al
    pairs["rows_a"], pairs["rows_b"] = rows_of(a), rows_of(b)
    pairs["tempo_q16"], pairs["pitch_q16"] = t16[v], f16[v]
    pairs["warped"] = np.where(mine, "a", "b")
    pairs["aligned_plain"] = plain
    with np.errstate(divide="ignore", invalid="ignore"):
        pairs["coverage_a"] = al / pairs["rows_a"].astype(np.float64)
        pairs["coverage_b"] = al / pairs["rows_b"].astype(np.float64)
    ca, cb = pairs["coverage_a"] >= min_coverage, pairs["coverage_b"] >= min_coverage
    pairs["relation"] = np.where(ca & cb, "same", np.where(ca, "a_in_b", np.where(cb, "b_in_a", "overlap")))
    same = pairs["relation"] == "same"
    return {"pairs": pairs, "clusters": _clusters(pairs["a"][same], pairs["b"][same])}


def _batches(rows, live, budget):
    """the live songs cut into the longest runs within the budget of rows, one song at least"""
    parts, lo = [], 0
    cum = np.cumsum(rows[live])
    while lo < len(live):
        base = cum[lo - 1] if lo else 0
        hi = max(lo + 1, int(np.searchsorted(cum, base + int(budget), "right")))
        parts.append(live[lo:hi])
        lo = hi
    return parts


def pair_extents(table, pairs, tol: int = 0, batch_rows: int = BATCH_ROWS) -> np.ndarray:
    """The records of fold_pairs with the position of every pair in both songs (EXTENT_PAIR_FIELDS): a_first .. a_last are the
    frames of song a, b_first .. b_last those of song b, between which the rows aligned at delta (+- tol) lie.  One
    Table.match_songs_extents call per batch of a songs (at most batch_rows rows): the a songs are the queries, (b, delta -
    tol, delta + tol) their candidates."""
    out = np.zeros(len(pairs), np.dtype(list(EXTENT_PAIR_FIELDS)))
    for f, _ in PAIR_FIELDS:
        out[f] = pairs[f]
    if len(pairs) == 0:
        return out
    a_ids, first, per = np.unique(pairs["a"], return_index=True, return_counts=True)   # (pairs are ordered by (a, b))
    slot = np.arange(len(pairs)) - np.repeat(first, per)
    row_off, _, _ = table.song_hashes(a_ids, counts_only=True)
    rows = np.diff(row_off.astype(np.int64))
    for part in _batches(rows, np.arange(len(a_ids)), batch_rows):
        for c0 in range(0, int(per[part].max()), 64):        # (a song with more than 64 partners: 64 a call)
            ncand = int(min(64, per[part].max() - c0))
            cs, lo, hi = (np.zeros((len(part), ncand), t) for t in (np.uint32, np.int32, np.int32))
            sel = np.flatnonzero(np.isin(pairs["a"], a_ids[part]) & (slot >= c0) & (slot < c0 + ncand))
            at = np.searchsorted(a_ids[part], pairs["a"][sel])
            cs[at, slot[sel] - c0] = pairs["b"][sel]
            lo[at, slot[sel] - c0] = pairs["delta"][sel] - int(tol)
            hi[at, slot[sel] - c0] = pairs["delta"][sel] + int(tol)
            ext = table.match_songs_extents(a_ids[part], cs, lo, hi, cand_n=np.clip(per[part] - c0, 0, ncand).astype(np.uint32),
                                            hist=False)
            for f, g in (("a_first", "q_first"), ("a_last", "q_last"), ("b_first", "t_first"), ("b_last", "t_last")):
                out[f][sel] = ext[g][at, slot[sel] - c0]
    return out


def warp_drift_bins(max_off: int, tempo_q16, tol: int = 0) -> int:
    """drift_bins=None of pair_extents_warps: speed.default_drift_bins' formula, ceil(t_max h / 65536), with t_max = the image
    of the table's largest offset max_off under the largest tempo rung among tempo_q16 and h = half the largest gap between
    neighbouring DISTINCT rungs among tempo_q16 (0 for one rung), clamped so that a candidate's 2 (tol + drift) + 1 bins stay
    within the 4,096 the moments allow.  Derivation as there: a copy of true tempo a found at rung r puts its aligned rows on
    the line d = t' (a / r - 1) + c; the found rung is the nearest, |a - r| <= h / 65536, and over the warped frames 0 ..
    t_max the line moves by at most t_max h / 65536 bins; the pair's delta is one bin ON that line."""
    rungs = np.unique(np.asarray(tempo_q16, np.int64))
    if len(rungs) < 2:
        return 0
    gap = int(np.max(np.diff(rungs)))                                 # 2 h
    t_max = (int(max_off) * int(rungs[-1]) + 32768) >> 16
    drift = -((-t_max * gap) // (2 * S_ONE))
    return max(0, min(drift, (4096 - 1) // 2 - int(tol)))


def _pair_extents_warps(table, pairs, tol, drift_bins, batch_rows, timings=False):
    """pair_extents_warps, and the (gather, warp, extent) device times of its library calls, summed (zeros without timings)"""
    from .extent import line_fit, own_frames, tempo_of
    out = np.zeros(len(pairs), np.dtype(list(WARP_EXTENT_PAIR_FIELDS)))
    for f, _ in WARP_PAIR_FIELDS:
        out[f] = pairs[f]
    out["tempo_fit"] = np.nan
    ms = np.zeros(3)
    if len(pairs) == 0:
        return out, tuple(ms.tolist())
    tol = int(tol)
    if drift_bins is None:
        from .shard import table_maxima
        drift_bins = warp_drift_bins(table_maxima(table)[1], pairs["tempo_q16"], tol)
    drift_bins = int(drift_bins)
    if tol < 0 or drift_bins < 0:
        raise ValueError("tol and drift_bins must be >= 0")
    out["drift_bins"] = drift_bins
    side_a = pairs["warped"] == "a"
    warped = np.where(side_a, pairs["a"], pairs["b"]).astype(np.uint32)      # the job's song: its rows are warped
    other = np.where(side_a, pairs["b"], pairs["a"]).astype(np.uint32)       # the job's one candidate
    d = np.where(side_a, pairs["delta"], -pairs["delta"]).astype(np.int64)   # (fold_pairs_warps turned b's sign: turned back)
    w = tol + drift_bins
    ids, inv = np.unique(warped, return_inverse=True)
    row_off, _, _ = table.song_hashes(ids, counts_only=True)
    rows = np.diff(np.asarray(row_off).astype(np.int64))[inv]                # rows of every job
    for part in _batches(rows, np.arange(len(pairs)), batch_rows):
        ext = table.match_songs_warps_extents(warped[part], pairs["tempo_q16"][part], pairs["pitch_q16"][part], other[part],
                                              (d[part] - w).astype(np.int32), (d[part] + w).astype(np.int32), hist=False,
                                              timings=timings)
        if timings:
            ms += np.asarray(ext["ms"])
        for i, p in enumerate(part):
            n = int(ext["count"][i, 0])
            out["count"][p] = n
            if n == 0:
                continue
            t16, qf, ql = int(pairs["tempo_q16"][p]), int(ext["q_first"][i, 0]), int(ext["q_last"][i, 0])
            own = own_frames(qf, ql, t16)
            there = (int(ext["t_first"][i, 0]), int(ext["t_last"][i, 0]))
            mine, theirs = (("a_first", "a_last"), ("b_first", "b_last")) if side_a[p] else (("b_first", "b_last"), ("a_first", "a_last"))
            out[mine[0]][p], out[mine[1]][p] = own
            out[theirs[0]][p], out[theirs[1]][p] = there
            out["warped_first"][p], out["warped_last"][p] = qf, ql
            fit = line_fit(n, ext["sum_q"][i, 0], ext["sum_u"][i, 0], ext["sum_qq"][i, 0], ext["sum_qu"][i, 0], int(d[p]) - w)
            if fit is not None:
                out["tempo_fit"][p] = float(tempo_of(t16, fit[0]))
    return out, tuple(ms.tolist())


def pair_extents_warps(table, pairs, tol: int = 0, drift_bins: int = None, batch_rows: int = BATCH_ROWS) -> np.ndarray:
    """The records of fold_pairs_warps with the position of every pair in both songs and a tempo fit (WARP_EXTENT_PAIR_FIELDS;
    DESIGN.md 3.7o).  One JOB per pair -- the pair's warped song at its (tempo_q16, pitch_q16) -- with one candidate, the other
    song at d +- (tol + drift_bins), d = delta where warped == "a" and -delta where warped == "b" (fold_pairs_warps turned that
    side's sign); the jobs go to Table.match_songs_warps_extents in batches of at most batch_rows rows (one job at least).
    a_first .. a_last / b_first .. b_last: the frames of song a / b between which the aligned rows lie -- the warped song's
    are its OWN frames (extent.own_frames of warped_first .. warped_last, its warped frames), the other song's are the
    candidate's t_first .. t_last.  count: the aligned pairs in the range.  tempo_fit = extent.tempo_of(tempo_q16, slope of
    extent.line_fit): the warped song runs tempo_fit times as fast as the other -- what tempo_q16 / 65536 says, refined; NaN
    where line_fit gives None.  All of them are 0 (NaN) where count is 0.  The fit pays on a coarse tempo axis and on long
    tracks; scripts/catalog_fit_bench.py measured that on 10 s tracks under the default fine ladder the rung is nearer the
    truth than the fit.
    drift_bins=None: warp_drift_bins(the table's largest offset, pairs["tempo_q16"], tol), derived, not tuned.  The table's
    largest offset is an upper bound of every song's length, so the range is wide enough for every pair and wider than a
    short track needs (chance pairs inside the range pull the line): a catalogue mixing short and long tracks may want an
    explicit drift_bins.  Only the rungs the pairs were found at are known here: pairs found at ONE rung give no gap and
    drift_bins 0, pairs found at rungs that are not neighbours a gap larger than the ladder's.  find_duplicates, which has
    the ladder, derives the value from the ladder's rungs and hands it over."""
    return _pair_extents_warps(table, pairs, tol, drift_bins, batch_rows)[0]


def _find_duplicates_warps(table, sids, lad, topn, min_aligned, min_coverage, batch_rows, timings=False, fit=None):
    from .speed import MAX_WARPS
    t16, f16, row = lad
    min_aligned = MIN_ALIGNED_WARPED if min_aligned is None else min_aligned
    min_coverage = MIN_COVERAGE_WARPED if min_coverage is None else min_coverage
    row_off, _, _ = table.song_hashes(sids, counts_only=True)
    rows = np.diff(row_off.astype(np.int64))
    live = np.flatnonzero(rows > 0)
    per_call = max(1, min(len(t16), (MAX_WARPS // row) * row))      # warps of one library call
    parts = _batches(rows, live, max(int(batch_rows) // per_call, 1))   # a batch: at most batch_rows rows x warps
    res = [_match_songs_warps(table, sids[p], t16, f16, row, topn, timings=timings) for p in parts]
    if not res:
        out = fold_pairs_warps([], t16, f16, [], [], [], [], [], [], min_aligned, min_coverage)
    else:
        listed = np.concatenate([sids[p] for p in parts])
        cat = {f: np.concatenate([r[f] for r in res]) for f in ("sid", "delta", "aligned", "nres", "rows")}
        valid = np.arange(topn)[None, None, :] < cat["nres"][:, :, None].astype(np.int64)
        found = np.setdiff1d(np.unique(cat["sid"][valid]), listed)
        f_off, _, _ = table.song_hashes(found, counts_only=True)
        out = fold_pairs_warps(listed, t16, f16, cat["sid"], cat["delta"], cat["aligned"], cat["nres"],
                               np.concatenate([listed, found]), np.concatenate([cat["rows"], np.diff(f_off)]),
                               min_aligned, min_coverage)
    if timings:
        out["ms"] = tuple(np.sum([r["ms"] for r in res], axis=0).tolist()) if res else (0.0, 0.0, 0.0)
    if fit is not None:   # (tol, drift_bins): the extent stage on the found pairs
        tol, drift = fit
        if drift is None and len(out["pairs"]):   # the LADDER's rungs are known here: the pairs' rungs are a subset, their gaps no smaller
            from .shard import table_maxima
            drift = warp_drift_bins(table_maxima(table)[1], t16, tol)
        out["pairs"], ms = _pair_extents_warps(table, out["pairs"], tol, drift, batch_rows, timings)
        if timings:
            out["ms"] = out["ms"] + (float(sum(ms)),)
    return out


@takes_delta_tol(lambda *a, **k: (lambda x: x.ctx)(k["db_or_table"] if "db_or_table" in k else a[0]))
def find_duplicates(db_or_table, sids=None, topn: int = 5, min_aligned: int = None, min_coverage: float = None,
                    batch_rows: int = BATCH_ROWS, speeds=None, tempos=None, pitches=None, warps=None, timings: bool = False,
                    extents=False, drift_bins: int = None) -> dict:
    """Duplicate, contained and overlapping tracks among the listed songs (None: every song of the table) and the rest of
    the table.  The songs are walked in batches of at most batch_rows rows (one counts-only gather gives the row counts),
    each batch is one match_songs call, and fold_pairs makes one record per pair.  Returns its dict: "pairs" and
    "clusters" -- delete_songs(cluster[1:]) keeps the smallest id of every set of copies.  A pair is found when either
    song lists the other among its topn strongest; raise topn for catalogues with many copies of one recording.
    min_aligned / min_coverage = None: MIN_ALIGNED / MIN_COVERAGE.
    With a ladder (speeds= / tempos= + pitches= / warps=, as match_songs reads them) sped-up, slowed-down and pitch-shifted
    copies are found too: every batch -- at most batch_rows rows x warps -- is matched at every pair, fold_pairs_warps makes
    the records (WARP_PAIR_FIELDS: which song's rows were warped, by which factors, and the plain count), and the
    thresholds default to MIN_ALIGNED_WARPED / MIN_COVERAGE_WARPED.  Put 65536 on the ladder (speed_ladder does) to keep
    the exact copies in the same answer.  timings (ladder only): "ms" = (gather, warp, match) device times, summed.
    delta_tol= (keyword): the vote tolerance in offset bins while the call runs (Context.tolerance); None: the context's.
    A song filter is taken from the context: run the call inside `with ctx.songs(only=...)` / `ctx.songs(exclude=...)` to match
    within / without a set of songs (every variant, every listed song uses the one set).
    The key cap is taken from the context too: run the call inside `with ctx.key_cap(rows):` to leave out the keys that hold
    more than `rows` table rows (Context.key_cap).
    extents: "pairs" gains a_first, a_last, b_first, b_last (EXTENT_PAIR_FIELDS; pair_extents): where in a and where in b the
    aligned rows lie -- the position of an excerpt inside the longer track, the length of an overlap.  extents=True does not
    take a ladder.
    extents="fit" (ladder only; the spelling of scan()): the search as above, then pair_extents_warps on the found pairs with
    tol = the vote tolerance of the call -- "pairs" has WARP_EXTENT_PAIR_FIELDS: where in a and in b an altered copy and its
    original overlap (each in its song's own frames), how many rows align there, and tempo_fit, the tempo the copy really runs
    at between the rungs.  drift_bins: bins each side of a pair's delta the extent pass looks at, beside the tolerance; None:
    warp_drift_bins(the table's largest offset, the LADDER's tempo rungs, tol) -- the formula of pair_extents_warps with the
    rungs the search really had, whose gaps are no larger than those among the rungs the pairs were found at (on the note
    corpus of tests/test_gpu_find_duplicates_fit.py the two plants are found at the outer rungs of three: 15 bins from the
    ladder, 29 from the pairs alone, and at 29 six chance pairs move an excerpt's start by 12 frames).  "clusters" and every column of
    WARP_PAIR_FIELDS are what the call without extents gives; with timings "ms" gains a fourth entry, the device time of the
    extent stage (its gather, warp and extent passes together)."""
    table, _ = _table_of(db_or_table)
    lad = _ladder_of(speeds, tempos, pitches, warps)
    fit = isinstance(extents, str)
    if fit and extents != "fit":
        raise ValueError(f'extents is False, True or "fit"; got {extents!r}')
    if fit and lad is None:
        raise ValueError('extents="fit" takes a ladder (speeds= / tempos= / pitches= / warps=); without one use extents=True')
    if extents and not fit and lad is not None:
        raise ValueError('extents=True does not take a ladder (speeds= / tempos= / pitches= / warps=); with one use extents="fit"')
    if drift_bins is not None and not fit:
        raise ValueError('drift_bins belongs to extents="fit"')
    min_aligned = (MIN_ALIGNED if min_aligned is None else min_aligned) if lad is None else min_aligned
    min_coverage = (MIN_COVERAGE if min_coverage is None else min_coverage) if lad is None else min_coverage
    if sids is None:
        from .shard import table_maxima
        sids = np.arange(1, table_maxima(table)[0] + 1, dtype=np.uint32) if table.rows()[0] else np.zeros(0, np.uint32)
    sids = np.ascontiguousarray(sids, np.uint32).reshape(-1)
    if lad is not None:
        return _find_duplicates_warps(table, sids, lad, topn, min_aligned, min_coverage, batch_rows, timings,
                                      (table.ctx.vote_tolerance, drift_bins) if fit else None)
    row_off, _, _ = table.song_hashes(sids, counts_only=True)
    rows = np.diff(row_off.astype(np.int64))
    live = np.flatnonzero(rows > 0)                  # (songs without rows match nothing)
    parts, lo = [], 0
    cum = np.cumsum(rows[live])
    while lo < len(live):                            # the longest run of songs within the budget, one song at least
        base = cum[lo - 1] if lo else 0
        hi = max(lo + 1, int(np.searchsorted(cum, base + int(batch_rows), "right")))
        parts.append(live[lo:hi])
        lo = hi
    res = [table.match_songs(sids[p], topn=topn) for p in parts]
    if not res:
        out = fold_pairs([], [], [], [], [], [], [], min_aligned, min_coverage)
        if extents:
            out["pairs"] = pair_extents(table, out["pairs"])
        return out
    listed = np.concatenate([sids[p] for p in parts])
    cat = {f: np.concatenate([r[f] for r in res]) for f in ("sid", "delta", "aligned", "nres", "rows")}
    valid = np.arange(topn)[None, :] < cat["nres"][:, None].astype(np.int64)
    found = np.setdiff1d(np.unique(cat["sid"][valid]), listed)      # songs outside the list: their rows by one more count
    f_off, _, _ = table.song_hashes(found, counts_only=True)
    out = fold_pairs(listed, cat["sid"], cat["delta"], cat["aligned"], cat["nres"], np.concatenate([listed, found]),
                     np.concatenate([cat["rows"], np.diff(f_off)]), min_aligned, min_coverage)
    if extents:
        out["pairs"] = pair_extents(table, out["pairs"], tol=table.ctx.vote_tolerance, batch_rows=batch_rows)
    return out
