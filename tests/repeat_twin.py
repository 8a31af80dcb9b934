"""The definition of repeated content inside a recording in plain Python on lists: what shz_repeats_hashes /
shz_repeats_batch (pairs, cells), shz_repeats_fold (repeats) and shazam_amd.repeats.occurrences compute.  Brute force on
purpose -- nothing here shares a line of reasoning with the kernels or with the fold's neighbour search.

All quantities are integers, in frames."""
from collections import defaultdict


def cells(key32, t1, hash_off, rec_clip0, min_lag, max_lag, max_run, cell_shift, min_cell_pairs):
    """The device half.  key32 / t1: the hashes of all clips, hash_off their CSR over the clips, rec_clip0 the CSR of the
    recordings over the clips.  Returns a dict: cell_off (CSR of the returned cells over the recordings), lag, block, pairs,
    first, last (the cells with pairs >= min_cell_pairs, ordered by (rec, lag, block)), rec_hashes, rec_pairs,
    rec_skipped_keys, rec_skipped_rows."""
    n_recs = len(rec_clip0) - 1
    out = {k: [] for k in ("lag", "block", "pairs", "first", "last", "rec_hashes", "rec_pairs", "rec_skipped_keys", "rec_skipped_rows")}
    out["cell_off"] = [0]
    for r in range(n_recs):
        a, b = int(hash_off[int(rec_clip0[r])]), int(hash_off[int(rec_clip0[r + 1])])
        hashes = {(int(key32[i]), int(t1[i])) for i in range(a, b)}            # duplicates across or inside channels collapse
        times = defaultdict(list)
        for k, t in hashes:
            times[k].append(t)
        n_pairs = skipped_keys = skipped_rows = 0
        acc = {}                                                                # (lag, block) -> [pairs, first, last]
        for k, ts in times.items():
            ts.sort()
            if len(ts) > max_run:                                               # a stop hash
                skipped_keys += 1
                skipped_rows += len(ts)
                continue
            for i in range(len(ts)):
                for j in range(i + 1, len(ts)):
                    lag = ts[j] - ts[i]
                    if min_lag <= lag <= max_lag:
                        n_pairs += 1
                        c = acc.setdefault((lag, ts[i] >> cell_shift), [0, ts[i], ts[i]])
                        c[0] += 1
                        c[1] = min(c[1], ts[i])
                        c[2] = max(c[2], ts[i])
        for (lag, block) in sorted(acc):
            n, first, last = acc[(lag, block)]
            if n >= min_cell_pairs:
                out["lag"].append(lag)
                out["block"].append(block)
                out["pairs"].append(n)
                out["first"].append(first)
                out["last"].append(last)
        out["cell_off"].append(len(out["lag"]))
        out["rec_hashes"].append(len(hashes))
        out["rec_pairs"].append(n_pairs)
        out["rec_skipped_keys"].append(skipped_keys)
        out["rec_skipped_rows"].append(skipped_rows)
    return out


REPEAT_FIELDS = ("rec", "lag", "lag_lo", "lag_hi", "first", "last", "pairs", "cells")


def fold(cell_off, lag, block, pairs, first, last, lag_tol, max_gap, min_pairs):
    """The host half.  Two cells of one recording are linked iff |lag - lag'| <= lag_tol and |block - block'| <= max_gap + 1;
    a repeat is a connected component of that relation whose summed pairs reach min_pairs.  Returns a list of dicts with
    REPEAT_FIELDS, ordered by (rec, first, lag, smallest cell index of the component)."""
    reps = []
    for r in range(len(cell_off) - 1):
        idx = list(range(int(cell_off[r]), int(cell_off[r + 1])))
        comp = {i: i for i in idx}                                              # every cell's component label
        for x in idx:                                                           # every pair of cells: quadratic, and plain
            for y in range(x + 1, int(cell_off[r + 1])):
                if abs(int(lag[x]) - int(lag[y])) <= lag_tol and abs(int(block[x]) - int(block[y])) <= max_gap + 1 \
                        and comp[x] != comp[y]:
                    old, new = comp[y], comp[x]
                    for z in idx:
                        if comp[z] == old:
                            comp[z] = new
        groups = defaultdict(list)
        for i in idx:
            groups[comp[i]].append(i)
        for members in groups.values():
            total = sum(int(pairs[i]) for i in members)
            if total < min_pairs:
                continue
            per_lag = defaultdict(int)
            for i in members:
                per_lag[int(lag[i])] += int(pairs[i])
            best = min(per_lag, key=lambda v: (-per_lag[v], v))                  # most pairs, the smaller lag on a tie
            reps.append((r, min(int(first[i]) for i in members), best, min(members),
                         dict(rec=r, lag=best, lag_lo=min(per_lag), lag_hi=max(per_lag), first=min(int(first[i]) for i in members),
                              last=max(int(last[i]) for i in members), pairs=total, cells=len(members))))
    reps.sort(key=lambda x: x[:4])
    return [x[4] for x in reps]


def occurrences(repeats):
    """Airings: every repeat gives the intervals [first, last] and [first + lag, last + lag] of its recording; two intervals
    of one recording are the same airing when they overlap by at least half of the shorter one (in frames, both ends
    inclusive).  Returns a list of groups (recording, [(start, end), ...]): the connected intervals merged into their hull, a
    group = the airings joined by repeats, ordered by recording and first airing."""
    items = []                                                                  # (rec, start, end, repeat index)
    for n, p in enumerate(repeats):
        items.append((p["rec"], p["first"], p["last"], n))
        items.append((p["rec"], p["first"] + p["lag"], p["last"] + p["lag"], n))
    same = list(range(len(items)))                                              # interval -> airing label

    def relabel(lab, old, new):
        for k in range(len(lab)):
            if lab[k] == old:
                lab[k] = new
    for a in range(len(items)):
        for b in range(a + 1, len(items)):
            ra, sa, ea, _ = items[a]
            rb, sb, eb, _ = items[b]
            if ra != rb:
                continue
            over = min(ea, eb) - max(sa, sb) + 1
            if 2 * over >= min(ea - sa + 1, eb - sb + 1) and same[a] != same[b]:
                relabel(same, same[b], same[a])
    group = list(same)                                                          # airing label -> group label
    for n in range(len(repeats)):
        a, b = group[2 * n], group[2 * n + 1]
        if a != b:
            relabel(group, b, a)
    out = defaultdict(dict)
    for k, (rec, s, e, _) in enumerate(items):
        air = out[(rec, group[k])].setdefault(same[k], [s, e])
        air[0], air[1] = min(air[0], s), max(air[1], e)
    res = [(rec, sorted((s, e) for s, e in airs.values())) for (rec, _), airs in out.items()]
    res.sort(key=lambda g: (g[0], g[1][0]))
    return res
