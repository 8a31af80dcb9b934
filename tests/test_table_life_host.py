"""CPU: the generator and the model of table_life_twin.py, which tests/test_gpu_table_life.py trusts.

  * every sequence the GPU file drives reaches the cases it is there for: visible rows inserted again (newest
    finalize and older ones), duplicates inside a batch and across two sealed runs, every kind of delete, a clear with a
    rebuild, both batch orders of seal_rows, empty and one-row batches -- and its bound U on the segment count stays <= 30;
  * the model (sets) against a restatement of the schema on plain arrays (np.unique as UNIQUE + INSERT IGNORE);
  * sequence() is a function of its seed."""
import numpy as np
import pytest

import table_life_twin as T

SEEDS = range(12)
EVERY_PROFILE = ("reinsert_newest", "reinsert_older", "dup_in_batch", "dup_across_runs", "delete_staged_only",
                 "delete_sealed_only", "delete_spread", "delete_absent", "delete_all_then_reuse", "clear_then_rebuild",
                 "ordered_batch", "unordered_batch", "empty_batch", "one_row_batch", "insert_clips",
                 "checkpoint_without_finalize")


@pytest.mark.parametrize("profile", T.PROFILES)
def test_every_sequence_reaches_every_case(profile):
    for seed in SEEDS:
        ops = T.sequence(seed, profile)
        cov = T.coverage(ops)
        missed = [name for name in EVERY_PROFILE if not cov[name]]
        assert not missed, (profile, seed, missed)
        assert cov["max_U"] <= T.U_MAX, (profile, seed, cov["max_U"])
        assert cov["max_rows"] <= 12000, (profile, seed, cov["max_rows"])
        assert 25 <= len(ops) <= 70, (profile, seed, len(ops))
        assert ops[-1][0] in ("finalize", "clear", "delete_songs")      # the last state is looked at
        if profile == "moving_limit":
            assert cov["limit_up"] and cov["limit_down"] and cov["limit_below_rows"], (seed, cov)


def _setting(ops, name):
    return [int(op[1]) for op in ops if op[0] == name]


@pytest.mark.parametrize("seed", SEEDS)
def test_profiles_have_their_shapes(seed):
    seqs = {p: T.sequence(seed, p) for p in T.PROFILES}
    first_insert = {p: next(i for i, op in enumerate(ops) if op[0] == "insert") for p, ops in seqs.items()}
    assert not _setting(seqs["one_segment"], "set_segment_rows") and not _setting(seqs["one_segment"], "set_run_rows")
    ops = seqs["tiny_segments"]
    assert ops[0] == ("set_segment_rows", 256) and _setting(ops, "set_segment_rows") == [256] and first_insert["tiny_segments"] == 1
    ops = seqs["runs"]
    assert ops[:2] == [("set_run_rows", 500), ("set_segment_rows", 2000)] and first_insert["runs"] == 2
    names = [op[0] for op in ops]
    sealed = sum(1 for a, b in zip(names, names[1:]) if a == "insert" and b == "seal_run")
    assert 2 * sealed > names.count("insert")                            # a seal after most inserts
    assert len(set(_setting(seqs["moving_limit"], "set_segment_rows"))) >= 3
    # widening: narrow rows sealed, then offsets up to 2^20 and ids up to 2^11 while those runs wait
    ops = seqs["widening"]
    assert ops[0] == ("set_run_rows", 500)
    ins = [op for op in ops[:8] if op[0] == "insert"]
    assert [op[0] for op in ops[1:8]] == ["insert", "seal_run", "insert", "seal_run", "insert", "seal_run", "finalize"]
    assert ins[0][2].max() < (1 << 10) and ins[0][3].max() < (1 << 9) and ins[0][2].max() >= (1 << 9)
    assert ins[1][2].max() < (1 << 10) and ins[1][3].max() == (1 << 20) - 1
    assert ins[2][2].max() == (1 << 11) - 1 and ins[2][3].max() < (1 << 20)
    for ops in seqs.values():                                           # ids and offsets of every profile fit one packed row
        for op in ops:
            if op[0] == "insert" and len(op[1]):
                assert int(op[1].max()) <= T.KEY_MAX and int(op[2].max()) < T.ABSENT_SID and int(op[3].max()) < (1 << 20)


class ArrayTable:
    """the schema restated on arrays: rows of int64 [n, 3], UNIQUE + INSERT IGNORE as np.unique over the rows"""

    def __init__(self):
        self.rows, self.pend = np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)

    def step(self, op):
        name = op[0]
        if name in ("insert", "insert_clips"):
            k, s, o = op[1:] if name == "insert" else T.clip_rows(*op[1:])
            new = np.stack([np.asarray(c, np.int64) for c in (k, s, o)], axis=1).reshape(-1, 3)
            self.pend = np.concatenate([self.pend, new])
        elif name == "finalize":
            self.rows = np.unique(np.concatenate([self.rows, self.pend]), axis=0)
            self.pend = self.pend[:0]
        elif name == "delete_songs":
            ids = np.asarray(op[1], np.int64)
            a, b = np.isin(self.rows[:, 1], ids), np.isin(self.pend[:, 1], ids)
            self.rows, self.pend = self.rows[~a], self.pend[~b]
            return int(a.sum()), int(b.sum())
        elif name == "clear":
            self.rows, self.pend = self.rows[:0], self.pend[:0]
        return None


@pytest.mark.parametrize("seed,profile", [(0, "tiny_segments"), (1, "runs"), (2, "widening")])
def test_model_against_arrays(seed, profile):
    m, a = T.Model(), ArrayTable()
    for i, op in enumerate(T.sequence(seed, profile)):
        assert m.apply(op) == a.step(op), (i, op[0])
        assert sorted(m.visible) == [tuple(r) for r in a.rows.tolist()], (i, op[0])
        assert sorted(m.pending) == sorted(tuple(r) for r in a.pend.tolist()), (i, op[0])


def test_sequence_is_deterministic_in_its_seed():
    def same(x, y):
        return len(x) == len(y) and all(
            a[0] == b[0] and len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:])) for a, b in zip(x, y))
    for profile in T.PROFILES:
        assert same(T.sequence(5, profile), T.sequence(5, profile))
        assert not same(T.sequence(5, profile), T.sequence(6, profile))


def test_expected_query_is_vote_tol_twins_expected_match():
    """the checkpoint's per-query expectation (rows indexed once) against vote_tol_twin.expected_match (indexed per query)"""
    from vote_tol_twin import expected_match
    ops = T.sequence(3, "tiny_segments")
    m = T.Model()
    for op in ops[:12]:
        m.apply(op)
    m.finalize()
    rows = sorted(m.visible)
    tk, ts, to = (np.array([r[i] for r in rows], np.int64) for i in range(3))
    by_key, by_sid = T.index_rows(m.visible)
    sid = sorted(by_sid)[0]
    q = [(k, o + 2) for k, o in by_sid[sid][:200]] + [(T.KEY_MAX + 5, 1)]
    qk, qo = np.array([h[0] for h in q], np.int64), np.array([h[1] for h in q], np.int64)
    for tol in (0, 2):
        want = expected_match(tk, ts, to, qk, qo, [0, len(q)], tol, 5)[0]
        assert T.expected_query(by_key, q, tol, 5) == want
