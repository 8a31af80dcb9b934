"""The definition of content shared between recordings in plain Python on lists: what shz_shared_hashes /
shz_shared_batch (pairs, cells) and shazam_amd.shared.shared_occurrences compute.  Brute force on purpose -- nothing here
shares a line of reasoning with the kernels, with repeat_twin.py or with the union-find of the package.  The fold is
repeat_twin.fold on the biased lags, the jobs standing in for its recordings.

All quantities are integers, in frames; lags are signed here (the library returns them biased by 2^20)."""
from collections import defaultdict


def cells(key32, t1, hash_off, rec_clip0, jobs, lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs):
    """The device half.  key32 / t1: the hashes of all clips, hash_off their CSR over the clips, rec_clip0 the CSR of the
    recordings over the clips, jobs a list of (a, b).  Returns a dict: cell_off (CSR of the returned cells over the jobs), lag
    (signed), block, pairs, first, last (the cells with pairs >= min_cell_pairs, ordered by (job, lag, block)), rec_hashes,
    job_pairs, job_skipped_keys, job_skipped_rows."""
    n_recs = len(rec_clip0) - 1
    H = []                                                                      # per recording: key -> sorted distinct times
    for r in range(n_recs):
        a, b = int(hash_off[int(rec_clip0[r])]), int(hash_off[int(rec_clip0[r + 1])])
        times = defaultdict(set)
        for i in range(a, b):
            times[int(key32[i])].add(int(t1[i]))                                # duplicates across or inside channels collapse
        H.append({k: sorted(ts) for k, ts in times.items()})
    out = {k: [] for k in ("lag", "block", "pairs", "first", "last", "job_pairs", "job_skipped_keys", "job_skipped_rows")}
    out["cell_off"] = [0]
    out["rec_hashes"] = [sum(len(ts) for ts in h.values()) for h in H]
    for a, b in jobs:
        n_pairs = skipped_keys = skipped_rows = 0
        acc = {}                                                                # (lag, block) -> [pairs, first, last]
        for k, ta_all in H[a].items():
            tb_all = H[b].get(k)
            if tb_all is None:
                continue
            if len(ta_all) > max_run or len(tb_all) > max_run:                  # a stop hash
                skipped_keys += 1
                skipped_rows += len(ta_all) + len(tb_all)
                continue
            for ta in ta_all:
                for tb in tb_all:
                    lag = tb - ta
                    if lag_lo <= lag <= lag_hi:
                        n_pairs += 1
                        c = acc.setdefault((lag, ta >> cell_shift), [0, ta, ta])
                        c[0] += 1
                        c[1] = min(c[1], ta)
                        c[2] = max(c[2], ta)
        for (lag, block) in sorted(acc):
            n, first, last = acc[(lag, block)]
            if n >= min_cell_pairs:
                out["lag"].append(lag)
                out["block"].append(block)
                out["pairs"].append(n)
                out["first"].append(first)
                out["last"].append(last)
        out["cell_off"].append(len(out["lag"]))
        out["job_pairs"].append(n_pairs)
        out["job_skipped_keys"].append(skipped_keys)
        out["job_skipped_rows"].append(skipped_rows)
    return out


def occurrences(shared, repeats=()):
    """Airings across recordings.  Every shared stretch gives the intervals (rec_a, first, last) and (rec_b, first + lag,
    last + lag), every repeat (rec, first, last) and (rec, first + lag, last + lag); two intervals of ONE recording are the
    same airing when they overlap by at least half of the shorter one (in frames, both ends inclusive); airings joined by a
    stretch or a repeat form a group.  Returns a list of (airings, shared indices, repeat indices): airings = the sorted
    (recording, first, last) hulls, the list ordered by first airing."""
    items = []                                                                  # (rec, start, end, "s" / "r", index)
    for n, p in enumerate(shared):
        items.append((p["rec_a"], p["first"], p["last"], "s", n))
        items.append((p["rec_b"], p["first"] + p["lag"], p["last"] + p["lag"], "s", n))
    for n, p in enumerate(repeats):
        items.append((p["rec"], p["first"], p["last"], "r", n))
        items.append((p["rec"], p["first"] + p["lag"], p["last"] + p["lag"], "r", n))
    same = list(range(len(items)))                                              # interval -> airing label

    def relabel(lab, old, new):
        for k in range(len(lab)):
            if lab[k] == old:
                lab[k] = new
    for x in range(len(items)):
        for y in range(x + 1, len(items)):
            rx, sx, ex = items[x][:3]
            ry, sy, ey = items[y][:3]
            if rx != ry:
                continue
            over = min(ex, ey) - max(sx, sy) + 1
            if 2 * over >= min(ex - sx + 1, ey - sy + 1) and same[x] != same[y]:
                relabel(same, same[y], same[x])
    group = list(same)                                                          # interval -> group label
    for n in range(len(items) // 2):                                            # the two intervals of one stretch or repeat
        x, y = group[2 * n], group[2 * n + 1]
        if x != y:
            relabel(group, y, x)
    res = []
    for g in sorted(set(group)):
        members = [k for k in range(len(items)) if group[k] == g]
        airs = []
        for lab in sorted({same[k] for k in members}):
            ks = [k for k in members if same[k] == lab]
            airs.append((items[ks[0]][0], min(items[k][1] for k in ks), max(items[k][2] for k in ks)))
        res.append((sorted(airs), sorted({items[k][4] for k in members if items[k][3] == "s"}),
                    sorted({items[k][4] for k in members if items[k][3] == "r"})))
    res.sort(key=lambda x: x[0][0])
    return res
