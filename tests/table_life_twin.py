"""Test helper for the table's life cycle (not a conftest, not collected): the fingerprints table as the reference's
schema defines it -- a set of (hash, song_id, offset) under UNIQUE(song_id, offset, hash) with INSERT IGNORE and ON DELETE
CASCADE (mysql_database.py:54-68) -- a generator of operation sequences that reach every build path, and the checkpoint
that compares a real table with the model through every read path, exactly."""
import numpy as np

from vote_tol_twin import vote_tol

PROFILES = ("one_segment", "tiny_segments", "runs", "moving_limit", "widening")
NO_LIMIT = 1 << 31            # rows per segment of a table nobody called set_segment_rows on
KEY_MAX = (1 << 28) - 1       # largest key of every profile (2^20 buckets a segment: cheap to index, and to index again)
ABSENT_SID = 3000             # no profile ever inserts it
U_MAX = 30                    # the generator's bound on the segment count (SHZ_MAX_SEGS is 32)
_EMPTY = np.zeros(0, np.uint32)


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


def _triples(k, s, o):
    return list(zip(np.asarray(k).tolist(), np.asarray(s).tolist(), np.asarray(o).tolist()))


def clip_rows(key, t1, hash_off, sid0):
    """the rows insert_clips stages: hash i of clip c is (key[i], sid0 + c, t1[i])"""
    ho = np.asarray(hash_off, np.int64)
    sid = np.repeat(np.arange(len(ho) - 1, dtype=np.int64) + int(sid0), np.diff(ho))
    return _u32(key[ho[0]:ho[-1]]), _u32(sid), _u32(t1[ho[0]:ho[-1]])


class Model:
    """visible: the rows queries see.  pending: rows inserted and not yet finalized (a list: duplicates are still there)."""

    def __init__(self):
        self.visible, self.pending = set(), []

    def insert(self, k, s, o):
        self.pending += _triples(k, s, o)

    def insert_clips(self, key, t1, hash_off, sid0):
        self.insert(*clip_rows(key, t1, hash_off, sid0))

    def seal_run(self):
        pass    # whether sealed rows are visible before the next finalize is the table's choice: nobody looks in between

    def finalize(self):
        self.visible.update(self.pending)
        self.pending = []

    def delete_songs(self, ids):
        """(distinct visible rows removed, pending rows removed)"""
        ids = set(int(i) for i in np.asarray(ids).tolist())
        gone = {r for r in self.visible if r[1] in ids}
        self.visible -= gone
        kept = [r for r in self.pending if r[1] not in ids]
        n_pending = len(self.pending) - len(kept)
        self.pending = kept
        return len(gone), n_pending

    def clear(self):
        self.visible, self.pending = set(), []

    def set_segment_rows(self, rows):
        pass

    def set_run_rows(self, rows):
        pass

    def apply(self, op):
        return getattr(self, op[0])(*op[1:])


def u_cost(pending, limit):
    """what one seal or finalize of `pending` rows adds to the bound on the segment count"""
    return -(-int(pending) // int(limit)) + 2


# ------------------------------------------------------------------------------------------------ the generator
class _Gen:
    def __init__(self, seed, profile):
        assert profile in PROFILES
        self.profile = profile
        self.rng = r = np.random.default_rng([int(seed), PROFILES.index(profile)])
        keys = np.concatenate([[0, KEY_MAX], r.choice(KEY_MAX - 1, 58, replace=False) + 1])
        self.keys = _u32(np.sort(keys))
        self.key_p = np.full(60, 0.7 / 58)
        self.key_p[r.choice(60, 2, replace=False)] = 0.15          # two hot keys
        self.sids = np.arange(1, 41, dtype=np.uint32)
        self.off_hi = 600
        self.fresh = 41                                            # ids for songs that live in one scene only
        self.bmin, self.bmax = {"one_segment": (1, 3000), "runs": (100, 1500)}.get(profile, (100, 700))
        self.p_seal = 0.8 if profile == "runs" else 0.2
        self.k = 2 if profile == "runs" else 1                    # seal and finalize, or finalize alone: for the cost of a scene
        self.limit, self.U = NO_LIMIT, 0
        self.ops, self.model = [], Model()
        self.fin, self.staged = [], []     # batches (k, s, o) finalized since the last clear / staged since the last finalize
        self.fin_id = []                   # the finalize every batch of fin came with

    # -- bookkeeping -----------------------------------------------------------------------------
    def emit(self, *op):
        name = op[0]
        if name in ("seal_run", "finalize"):
            self.U += u_cost(len(self.model.pending), self.limit)
            assert self.U <= U_MAX, (self.profile, self.U)
        self.ops.append(op)
        self.model.apply(op)
        if name == "insert":
            self.staged.append(op[1:])
        elif name == "insert_clips":
            self.staged.append(clip_rows(*op[1:]))
        elif name == "finalize":
            self.fin += [b for b in self.staged if len(b[0])]
            self.fin_id += [len(self.ops)] * (len(self.fin) - len(self.fin_id))
            self.staged = []
        elif name == "clear":
            self.U, self.fin, self.fin_id, self.staged = 0, [], [], []
        elif name == "delete_songs":
            keep = lambda b: tuple(c[~np.isin(b[1], op[1])] for c in b)  # noqa: E731
            kept = [(b, i) for b, i in zip(map(keep, self.fin), self.fin_id) if len(b[0])]
            self.fin, self.fin_id = [b for b, _ in kept], [i for _, i in kept]
            self.staged = [keep(b) for b in self.staged]
        elif name == "set_segment_rows":
            self.limit = int(op[1])

    def cost(self, *pendings):
        return sum(u_cost(p, self.limit) for p in pendings)

    def prepare(self, batches, cost):
        """room for a scene that adds `cost` to U, on a table that holds the rows of `batches` finalize calls at least;
        clears (instead of inserting) where the scene could push U past the bound"""
        assert not self.model.pending
        missing = max(0, batches - len(set(self.fin_id)))
        if self.U + self.regrow_cost(missing) + cost > U_MAX:
            self.emit("clear")
            missing = max(batches, 1)
        for _ in range(missing):
            self.regrow()
        assert self.U + cost <= U_MAX, (self.profile, self.U, cost)

    # -- rows ------------------------------------------------------------------------------------
    def batch(self, n, sids=None, ordered=None):
        r = self.rng
        k = self.keys[r.choice(60, n, p=self.key_p)]
        s = _u32(r.choice(self.sids if sids is None else np.asarray(sids), n))
        o = _u32(r.integers(0, self.off_hi, n))
        return self.order(k, s, o, ordered)

    def order(self, k, s, o, ordered=None):
        """by (song id, offset) -- what an ingest of whole songs delivers, and seal_rows' cheaper sort plan -- or shuffled"""
        if ordered is None:
            ordered = bool(self.rng.integers(2))
        i = np.lexsort((o, s)) if ordered else self.rng.permutation(len(k))
        return _u32(k[i]), _u32(s[i]), _u32(o[i])

    def size(self):
        return int(self.rng.integers(self.bmin, self.bmax + 1))

    def sample(self, b, n):
        i = self.rng.choice(len(b[0]), min(n, len(b[0])), replace=False)
        return tuple(c[i] for c in b)

    # -- scenes: each starts and ends with nothing pending ------------------------------------------
    def regrow_cost(self, n=1):
        """what n calls of regrow add to U at most"""
        plain = self.cost(self.bmax) * (2 if self.profile == "runs" else 1)      # (runs: a seal and a finalize)
        first = self.cost(700, 1400, 1700, 1700) if self.profile == "widening" else plain
        return (first + (n - 1) * plain) if n else 0

    def regrow(self):
        """a plain batch into the table; the widening profile rebuilds its waiting runs"""
        if self.profile == "widening" and not self.fin:
            return self.widen()
        self.emit("insert", *self.batch(self.size()))
        self.maybe_seal()
        self.emit("finalize")

    def maybe_seal(self):
        """the runs profile seals after most inserts, wherever they happen"""
        if self.profile == "runs" and self.rng.random() < self.p_seal:
            self.emit("seal_run")

    def widen(self):
        """runs wait in the arena while the offsets, then the ids, outgrow their packing: run_repack_kernel in place"""
        self.sids, self.off_hi = np.append(np.arange(1, 41), 1023).astype(np.uint32), 1 << 9
        self.emit("insert", *self.batch(700))
        self.emit("seal_run")
        self.off_hi = 1 << 20
        k, s, o = self.batch(700)
        o[0] = (1 << 20) - 1
        self.emit("insert", k, s, o)
        self.emit("seal_run")
        self.sids = np.concatenate([self.sids, np.arange(1500, 1510), [2047]]).astype(np.uint32)
        k, s, o = self.batch(300)
        s[0] = 2047
        self.emit("insert", k, s, o)
        self.emit("seal_run")
        self.emit("finalize")

    def grow(self):
        n = self.size()
        seal = self.rng.random() < self.p_seal
        self.prepare(0, self.cost(n, n) if seal else self.cost(n))
        self.emit("insert", *self.batch(n))
        if seal:
            self.emit("seal_run")
        self.emit("finalize")

    def reinsert(self):
        """rows already visible come again (from the newest batch: the active segment; from the oldest: a frozen one where
        the profile has any), beside new rows and copies inside the batch"""
        n = min(self.size(), 600)
        self.prepare(2, self.k * self.cost(3 * n + 50))
        new = self.batch(n)
        parts = [new, self.sample(self.fin[-1], n), self.sample(self.fin[0], n), self.sample(new, 50)]
        k, s, o = (np.concatenate([p[i] for p in parts]) for i in range(3))
        self.emit("insert", *self.order(k, s, o))
        self.maybe_seal()
        self.emit("finalize")

    def overlap_runs(self):
        """two sealed runs with overlapping song-id ranges that share rows; in the runs profile from an empty table, with
        enough rows that the second seal cuts a full segment and the third meets rows of a frozen one"""
        if self.profile == "runs":
            self.emit("clear")
            a, b, c = self.batch(1500), self.batch(1200), self.batch(400)
            b = self.order(*(np.concatenate([b[i], a[i][::3]]) for i in range(3)))
            c = self.order(*(np.concatenate([c[i], a[i][::2], b[i][::5]]) for i in range(3)))
            steps = [a, b, c]
        else:
            self.prepare(1, self.cost(300, 600, 600))
            a, b = self.batch(300), self.batch(150)
            b = self.order(*(np.concatenate([b[i], a[i][::2]]) for i in range(3)))
            steps = [a, b]
        for x in steps:
            self.emit("insert", *x)
            self.emit("seal_run")
        self.emit("finalize")

    def delete_staged(self):
        """a song that is only staged leaves; half the time it is all there was to finalize"""
        alone = bool(self.rng.integers(2))
        self.prepare(1, 0 if alone else self.k * self.cost(500))
        sid, self.fresh = self.fresh, self.fresh + 1
        if not alone:
            self.emit("insert", *self.batch(300))
            self.maybe_seal()
        self.emit("insert", *self.batch(int(self.rng.integers(40, 200)), sids=[sid]))
        self.emit("delete_songs", _u32([sid]))
        if not alone:
            self.emit("finalize")

    def delete_sealed(self):
        """a song that sits only in sealed rows leaves: nothing is pending afterwards, and nothing of it is visible"""
        n = int(self.rng.integers(40, 200))
        self.prepare(1, self.cost(n))
        sid, self.fresh = self.fresh, self.fresh + 1
        self.emit("insert", *self.batch(n, sids=[sid]))
        self.emit("seal_run")
        self.emit("delete_songs", _u32([sid]))

    def delete_spread(self):
        """a song whose rows came with several finalize calls (several segments where the profile cuts any), beside an id
        that was never there; no finalize follows"""
        self.prepare(2, 0)
        both = np.intersect1d(self.fin[0][1], self.fin[-1][1])
        if len(both) == 0:          # (deletes took every shared song: two plain batches bring the whole pool back)
            self.prepare(0, self.regrow_cost(2))
            self.regrow()
            self.regrow()
            both = np.intersect1d(self.fin[-2][1], self.fin[-1][1])
        self.emit("delete_songs", _u32([self.rng.choice(both)]))

    def delete_absent(self):
        self.prepare(1, 0)
        self.emit("delete_songs", _u32([ABSENT_SID]))

    def delete_all(self):
        """every id present (and a few that are not): the table is empty mid-life, answers, and is used again"""
        self.prepare(1, self.regrow_cost())
        ids = sorted({r[1] for r in self.model.visible} | {0, ABSENT_SID})
        self.emit("delete_songs", _u32(ids))
        self.regrow()

    def clear_rebuild(self):
        self.prepare(1, 0)
        self.emit("clear")
        self.regrow()

    def small_batches(self):
        self.prepare(0, self.k * self.cost(1))
        self.emit("insert", _EMPTY, _EMPTY, _EMPTY)
        self.emit("insert", *self.batch(1))
        self.maybe_seal()
        self.emit("finalize")

    def clips(self):
        """the CSR form of fingerprint_batch: three clips, the middle one without hashes"""
        na, nb = int(self.rng.integers(20, 200)), int(self.rng.integers(20, 200))
        self.prepare(0, self.k * self.cost(na + nb))
        k, _, o = self.batch(na + nb)
        sid0 = int(self.rng.integers(1, 38))
        self.emit("insert_clips", k, o, np.array([0, na, na, na + nb], np.uint64), sid0)
        self.maybe_seal()
        self.emit("finalize")

    def limit_below_rows(self):
        """moving_limit: the limit drops below the rows the active segment holds, then a batch arrives"""
        self.emit("clear")
        self.emit("set_segment_rows", 1000)
        self.emit("insert", *self.batch(900))
        self.emit("finalize")
        self.emit("set_segment_rows", 200)
        self.emit("insert", *self.batch(500))
        self.emit("finalize")

    def run(self):
        p = self.profile
        if p in ("tiny_segments", "moving_limit"):
            self.emit("set_segment_rows", 256)
        if p == "runs":
            self.emit("set_run_rows", 500)
            self.emit("set_segment_rows", 2000)
        if p == "widening":
            self.emit("set_run_rows", 500)
        self.regrow()
        scenes = [self.grow, self.reinsert, self.overlap_runs, self.delete_staged, self.delete_sealed, self.delete_spread,
                  self.delete_absent, self.delete_all, self.clear_rebuild, self.small_batches, self.clips, self.reinsert]
        if p == "moving_limit":
            scenes.append(self.limit_below_rows)
        for i in self.rng.permutation(len(scenes)):
            if p == "moving_limit" and not self.model.pending:
                self.emit("set_segment_rows", int(self.rng.choice([200, 256, 400, 1000])))
            scenes[i]()
        if self.model.pending:
            self.emit("finalize")
        return self.ops


def sequence(seed, profile):
    """A deterministic list of operations (name, arrays...) for Model.apply and for drive()."""
    return _Gen(seed, profile).run()


# ------------------------------------------------------------------------------------------------ what a sequence reaches
def is_checkpoint(op, model):
    """after `op` was applied: a finalize, a clear, or a delete that left nothing pending"""
    return op[0] in ("finalize", "clear") or (op[0] == "delete_songs" and not model.pending)


def coverage(ops):
    """Replays a sequence on the model alone and reports what it reached: {name: bool}, plus "max_U" and "max_rows"."""
    names = ("reinsert_newest", "reinsert_older", "dup_in_batch", "dup_across_runs", "delete_staged_only", "delete_sealed_only",
             "delete_spread", "delete_absent", "delete_all_then_reuse", "clear_then_rebuild", "ordered_batch", "unordered_batch",
             "empty_batch", "one_row_batch", "insert_clips", "checkpoint_without_finalize", "limit_up", "limit_down",
             "limit_below_rows")
    cov = dict.fromkeys(names, False)
    m, age, n_fin = Model(), {}, 0            # age: row -> the finalize that made it visible
    sealed, unsealed = [], []                 # pending rows: sealed groups (sets), rows staged since the last seal
    limit, U, max_U, max_rows = NO_LIMIT, 0, 0, 0
    emptied = cleared = False
    fin_since_clear = []                      # pending counts of the finalize calls since the last clear
    for op in ops:
        name = op[0]
        if name in ("insert", "insert_clips"):
            k, s, o = op[1:] if name == "insert" else clip_rows(*op[1:])
            rows = _triples(k, s, o)
            cov["insert_clips"] |= name == "insert_clips"
            cov["empty_batch"] |= len(rows) == 0
            cov["one_row_batch"] |= len(rows) == 1
            cov["dup_in_batch"] |= len(set(rows)) < len(rows)
            seen = [age[r] for r in set(rows) if r in m.visible]
            cov["reinsert_newest"] |= any(a == n_fin for a in seen)
            cov["reinsert_older"] |= any(a < n_fin for a in seen)
            if len(rows) >= 64:
                so = np.asarray(s, np.int64) << 32 | np.asarray(o, np.int64)
                inorder = bool((np.diff(so) >= 0).all())
                cov["ordered_batch"] |= inorder
                cov["unordered_batch"] |= not inorder
            unsealed += rows
        elif name in ("seal_run", "finalize"):
            U += u_cost(len(m.pending), limit)
            if unsealed:
                group = set(unsealed)
                cov["dup_across_runs"] |= any(group & g for g in sealed)
                sealed.append(group)
                unsealed = []
            if name == "finalize":
                for r in m.pending:
                    if r not in m.visible:
                        age.setdefault(r, n_fin + 1)
                fin_since_clear.append(len(m.pending))
                n_fin += 1
                sealed = []
        elif name == "delete_songs":
            ids = set(np.asarray(op[1]).tolist())
            for i in ids:
                vis = {age[r] for r in m.visible if r[1] == i}
                in_sealed = any(r[1] == i for g in sealed for r in g)
                in_unsealed = any(r[1] == i for r in unsealed)
                cov["delete_staged_only"] |= in_unsealed and not in_sealed and not vis
                cov["delete_sealed_only"] |= in_sealed and not in_unsealed and not vis
                cov["delete_spread"] |= len(vis) >= 2
                cov["delete_absent"] |= not (vis or in_sealed or in_unsealed)
            sealed = [{r for r in g if r[1] not in ids} for g in sealed]
            unsealed = [r for r in unsealed if r[1] not in ids]
        elif name == "clear":
            sealed, unsealed, U, fin_since_clear = [], [], 0, []
        elif name == "set_segment_rows":
            r = int(op[1])
            cov["limit_up"] |= r > limit
            cov["limit_down"] |= r < limit
            # every visible row came with the one finalize since the clear and fitted the limit: one active segment
            cov["limit_below_rows"] |= len(fin_since_clear) == 1 and r < len(m.visible) <= min(limit, fin_since_clear[0])
            limit = r
        had = len(m.visible)
        m.apply(op)
        if name == "finalize" and m.visible:
            cov["delete_all_then_reuse"] |= emptied
            cov["clear_then_rebuild"] |= cleared
        if name == "delete_songs":
            for r in [r for r in age if r not in m.visible]:
                del age[r]
            emptied |= had > 0 and not m.visible and not m.pending
            cov["checkpoint_without_finalize"] |= is_checkpoint(op, m)
        if name == "clear":
            age, cleared = {}, cleared or had > 0
        max_U, max_rows = max(max_U, U), max(max_rows, len(m.visible))
    cov["max_U"], cov["max_rows"] = max_U, max_rows
    return cov


# ------------------------------------------------------------------------------------------------ the checkpoint
def index_rows(visible):
    """key -> [(sid, off)] ascending, and sid -> [(key, off)] ascending"""
    by_key, by_sid = {}, {}
    for k, s, o in sorted(visible):
        by_key.setdefault(k, []).append((s, o))
        by_sid.setdefault(s, []).append((k, o))
    return by_key, by_sid


def expected_query(by_key, hashes, tol, topn):
    """Table.match of one query (its hashes taken as a set, as return_matches does) against the indexed rows:
    ([(sid, delta, aligned, dedup)] ranked, npairs, nhash) -- vote_tol_twin.expected_match without its index per query."""
    hs = sorted(set((int(k), int(q)) for k, q in hashes))
    matches, dedup, seen = [], {}, set()
    for k, q in hs:
        for s, o in by_key.get(k, ()):
            matches.append((s, o - q))
            if k not in seen:
                dedup[s] = dedup.get(s, 0) + 1
        seen.add(k)
    return [(s, d, c, dedup[s]) for s, d, c in vote_tol(matches, tol, topn)], len(matches), len(hs)


def _queries(by_sid, deleted_rows, rng):
    """six queries as (key, q_off) lists: crops of two present songs at a shifted offset, a mix of two songs, the former
    rows of a deleted song, no hashes at all, keys no profile holds"""
    present = sorted(by_sid)
    out = []

    def crop(sid):
        rows = by_sid[sid]
        offs = sorted({o for _, o in rows})
        a = offs[int(rng.integers(len(offs)))] if len(offs) > 1 else offs[0]
        shift = int(rng.integers(0, 4))
        return [(k, o - a + shift) for k, o in rows if a <= o < a + 300][:150]

    picks = [present[int(i)] for i in rng.choice(len(present), 2, replace=len(present) < 2)] if present else []
    for sid in picks:
        out.append(crop(sid))
    while len(out) < 2:
        out.append([(int(KEY_MAX), 1), (0, 2)])
    out.append(out[0][::2] + out[1][1::2])
    gone = sorted(deleted_rows)[:150]
    out.append([(k, o) for k, _, o in gone if o < (1 << 20)] or [(0, 0)])
    out.append([])
    out.append([(int(KEY_MAX) + 1 + i, i) for i in range(40)])
    return [sorted(set(q)) for q in out]


def check_match(table, expected, queries, tol, topn, what):
    """expected: expected_query of every query at this tolerance and a topn no smaller (a ranking's head is the ranking
    of a smaller topn)"""
    qk = _u32([k for q in queries for k, _ in q])
    qo = _u32([o for q in queries for _, o in q])
    qoff = np.cumsum([0] + [len(q) for q in queries]).astype(np.uint64)
    res = table.match(qk, qo, qoff, topn, delta_tol=tol)
    for q, hashes in enumerate(queries):
        ranked, npairs, nhash = expected[q][0][:topn], expected[q][1], expected[q][2]
        assert int(res["npairs"][q]) == npairs and int(res["nhash"][q]) == nhash, (what, q, "counters")
        assert int(res["nres"][q]) == len(ranked), (what, q, "nres", int(res["nres"][q]), len(ranked))
        got = [(int(res["sid"][q, i]), int(res["delta"][q, i]), int(res["aligned"][q, i]), int(res["dedup"][q, i]))
               for i in range(len(ranked))]
        assert got == ranked, (what, q, got[:3], ranked[:3])
        for name in ("sid", "delta", "aligned", "dedup"):
            assert not res[name][q, len(ranked):].any(), (what, q, name, "rows behind the ranked ones")


def check(table, model, rng, ctx):
    """Every read path of `table` against model.visible, exactly.  ctx: {"what": str, "checkpoint": int, "U": bound on the
    segment count or None, "deleted": {rows deleted so far}, "gone_sid": a deleted id or None, "full": False for a
    ShardedTable (no segments(), no song_hashes), "hash_sid_max": song_hashes lists no id above it}.  Every part runs;
    the assertion names all that failed, so that one wrong table shows in each read path it reaches."""
    assert not model.pending
    what, visible, fails = ctx.get("what", ""), model.visible, []
    full = ctx.get("full", True)
    by_key, by_sid = index_rows(visible)
    present = sorted(by_sid)
    sids = [present[int(i)] for i in rng.choice(len(present), min(3, len(present)), replace=False)] if present else []
    if ctx.get("gone_sid") is not None and ctx["gone_sid"] not in by_sid:
        sids.append(int(ctx["gone_sid"]))
    sids = list(dict.fromkeys(sids + [ABSENT_SID]))

    def part(fn):
        try:
            fn()
        except AssertionError as e:
            fails.append((fn.__name__, e.args[0] if e.args else ""))

    def rows_and_segments():
        assert tuple(table.rows()) == (len(visible), 0), (table.rows(), len(visible))
        if full:
            n = table.segments()
            assert n == 0 if not visible else n >= 1, n
            assert ctx.get("U") is None or n <= ctx["U"], (n, ctx["U"])

    def export():
        k, s, o = table.export()
        assert len(k) == len(visible), (len(k), len(visible))       # no row sits in two segments
        assert set(_triples(k, s, o)) == visible

    def song_rows():
        for sid in sids:
            assert table.song_rows(sid) == len(by_sid.get(sid, ())), sid

    def song_hashes():
        ids = [s for s in sids if s <= ctx.get("hash_sid_max", 1 << 24)]
        want = [by_sid.get(s, []) for s in ids]
        off = np.cumsum([0] + [len(w) for w in want]).astype(np.uint64)
        ro, k, o = table.song_hashes(ids)
        assert np.array_equal(ro, off), (ro, off)
        assert list(zip(k.tolist(), o.tolist())) == [r for w in want for r in w]
        ro, k, o = table.song_hashes(ids, counts_only=True)
        assert np.array_equal(ro, off) and len(k) == 0 and len(o) == 0

    def lookup():
        held = np.array(sorted(by_key), np.int64)
        some = rng.choice(held, min(18, len(held)), replace=False).tolist() if len(held) else []
        absent = [int(x) for x in rng.integers(1, KEY_MAX, 20) if int(x) not in by_key] + [KEY_MAX + 7]
        keys = list(dict.fromkeys([0, int(ctx.get("key_max", KEY_MAX))] + some + absent))
        keys = [keys[int(i)] for i in rng.permutation(len(keys))]
        k, s, o = table.lookup(_u32(keys))
        want = [(key, s_, o_) for key in keys for s_, o_ in by_key.get(key, ())]
        assert len(k) == len(want), (len(k), len(want))
        assert k.tolist() == [w[0] for w in want]                       # grouped in key-list order
        assert sorted(_triples(k, s, o)) == sorted(want)

    def match():
        queries = _queries(by_sid, ctx.get("deleted", ()), rng)
        tols = [0, 2] if ctx.get("checkpoint", 0) % 3 == 0 else [0]
        for tol in tols:
            expected = [expected_query(by_key, q, tol, 5) for q in queries]
            for topn in (1, 5):
                check_match(table, expected, queries, tol, topn, (what, "tol", tol, "topn", topn))

    for fn in [rows_and_segments, export, song_rows] + ([song_hashes] if full else []) + [lookup, match]:
        part(fn)
    assert not fails, (what, "checkpoint", ctx.get("checkpoint"), [f[0] for f in fails], fails)


def _apply(table, op):
    if op[0] == "set_run_rows" and not hasattr(table, "set_run_rows"):      # a ShardedTable: every shard on this GPU
        return [t.set_run_rows(op[1]) for t in table.tables]
    return getattr(table, op[0])(*op[1:])


def drive(tables, ops, seed, what="", full=True):
    """Apply `ops` to every table of `tables` and to one model; check every table at every checkpoint.  The number a
    delete returns is checked too: the visible rows that left and, of the pending ones, every staged row -- a sealed row may
    have met its duplicate already, so those count between once and as often as they were inserted."""
    model = Model()
    fulls = list(full) if isinstance(full, (tuple, list)) else [full] * len(tables)
    limit, U, n_check, deleted, gone_sid, sealed = NO_LIMIT, 0, 0, set(), None, False
    for i, op in enumerate(ops):
        name = op[0]
        if name in ("seal_run", "finalize"):
            U += u_cost(len(model.pending), limit)
        sealed = (sealed or name == "seal_run") and name not in ("finalize", "clear")
        if name == "delete_songs":
            ids = set(np.asarray(op[1]).tolist())
            deleted |= {r for r in model.visible if r[1] in ids}
            gone_sid = int(op[1][0])
        got = [_apply(t, op) for t in tables]
        ret = model.apply(op)
        if name == "clear":
            U = 0
        if name == "set_segment_rows":
            limit = int(op[1])
        if name == "delete_songs":
            nv, npend = ret
            for g in got:
                assert (nv <= g <= nv + npend) if sealed else g == nv + npend, (what, i, "rows deleted", g, nv, npend)
        if is_checkpoint(op, model):
            deleted -= model.visible
            for j, t in enumerate(tables):
                check(t, model, np.random.default_rng([int(seed), i]),
                      {"what": (what, "op", i, name, "table", j), "checkpoint": n_check, "U": U, "deleted": deleted,
                       "gone_sid": gone_sid, "full": fulls[j]})
            n_check += 1
    return model
