"""The catalogue's own question: "which of my tracks are the same recording?" (csrc/shz_catalog.hip).

Everything else here answers "which song is this audio?".  A catalogue of 10^5 to 10^6 tracks holds re-uploads, the album
and the single cut, tracks inside compilations and sets, radio edits inside full versions.  The reference has no answer
beyond deleting files by hand; INSERT IGNORE protects only against the same file_sha1.  The table already holds what is
needed: a song's rows are a ready-made query.  shz_table_song_hashes gathers the rows of listed songs on the device,
shz_match_songs matches them against the rest of the table in the same call, and find_duplicates() walks a catalogue in
batches and folds the answers of both directions into one record per pair of songs.

A pair (a, b), a < b, is reported with delta = off_b - off_a (b's frame under a's frame 0), the aligned count, both row
counts and both coverages aligned / rows.  "same": both songs are covered; "a_in_b" / "b_in_a": one is (an excerpt inside a
longer track); "overlap": neither, but enough rows align.  The clusters of "same" are what delete_songs() wants."""
from __future__ import annotations

import numpy as np

# Detection thresholds, set between the two distributions scripts/catalog_bench.py measured on the music-like synthetic
# corpus (10 s songs of about 3,180 rows): among 51,000 songs no unrelated pair aligned more than 59 rows or
# covered more than 0.027 of its smaller song; no planted copy or excerpt aligned fewer than 1,474 rows or covered less than
# 0.867 of its smaller song.  0.8 rather than the middle: "same" is what delete_songs() acts on, and an excerpt that lacks a
# fifth of the longer track should stay "a_in_b" / "b_in_a".  Not measured: re-encoded or noisy copies, tracks of minutes.
MIN_ALIGNED = 200
MIN_COVERAGE = 0.8
BATCH_ROWS = 1 << 22     # rows of the listed songs handed to one shz_match_songs call

PAIR_FIELDS = (("a", np.uint32), ("b", np.uint32), ("delta", np.int64), ("aligned", np.uint32), ("rows_a", np.uint64),
               ("rows_b", np.uint64), ("coverage_a", np.float64), ("coverage_b", np.float64), ("relation", "U7"))


def _table_of(db_or_table):
    """(table, db or None): a HipFingerprintDB is finalized first; a sharded one has no song gather."""
    db = db_or_table if hasattr(db_or_table, "table") else None
    table = db.table if db is not None else db_or_table
    if not hasattr(table, "h"):
        raise NotImplementedError("the catalogue calls take the unsharded table (shards=1)")
    if db is not None:
        db.finalize()
    return table, db


def match_songs(db_or_table, sids, topn: int = 5, full_sort: bool = False) -> dict:
    """Every listed song matched against the rest of the table in one library call (shz_match_songs): the arrays of
    Table.match with one query per listed song and the song itself left out (sid, delta, aligned, dedup [n, topn]; nres,
    nhash, npairs [n]), plus rows [n], the songs' row counts.  delta is the found song's frame under the listed song's
    frame 0."""
    table, _ = _table_of(db_or_table)
    return table.match_songs(sids, topn=topn, full_sort=full_sort)


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


def find_duplicates(db_or_table, sids=None, topn: int = 5, min_aligned: int = MIN_ALIGNED, min_coverage: float = MIN_COVERAGE,
                    batch_rows: int = BATCH_ROWS) -> dict:
    """Duplicate, contained and overlapping tracks among the listed songs (None: every song of the table) and the rest of
    the table.  The songs are walked in batches of at most batch_rows rows (one counts-only gather gives the row counts),
    each batch is one match_songs call, and fold_pairs makes one record per pair.  Returns its dict: "pairs" and
    "clusters" -- delete_songs(cluster[1:]) keeps the smallest id of every set of copies.  A pair is found when either
    song lists the other among its topn strongest; raise topn for catalogues with many copies of one recording."""
    table, _ = _table_of(db_or_table)
    if sids is None:
        from .shard import table_maxima
        sids = np.arange(1, table_maxima(table)[0] + 1, dtype=np.uint32) if table.rows()[0] else np.zeros(0, np.uint32)
    sids = np.ascontiguousarray(sids, np.uint32).reshape(-1)
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
        return fold_pairs([], [], [], [], [], [], [], min_aligned, min_coverage)
    listed = np.concatenate([sids[p] for p in parts])
    cat = {f: np.concatenate([r[f] for r in res]) for f in ("sid", "delta", "aligned", "nres", "rows")}
    valid = np.arange(topn)[None, :] < cat["nres"][:, None].astype(np.int64)
    found = np.setdiff1d(np.unique(cat["sid"][valid]), listed)      # songs outside the list: their rows by one more count
    f_off, _, _ = table.song_hashes(found, counts_only=True)
    return fold_pairs(listed, cat["sid"], cat["delta"], cat["aligned"], cat["nres"], np.concatenate([listed, found]),
                      np.concatenate([cat["rows"], np.diff(f_off)]), min_aligned, min_coverage)
