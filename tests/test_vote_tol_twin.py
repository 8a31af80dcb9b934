"""CPU: the tolerant vote's plain-Python definition (tests/vote_tol_twin.py) at tolerance 0 is oracle.cpu_ref.vote, on the
golden match cases and on random matches; its window rules on small built cases; the new symbols are declared in
include/shz.h, exported, and refuse a NULL context without a GPU."""
import json
import os
import random

from vote_tol_twin import vote_tol


def test_tol0_is_the_oracle_vote_on_the_golden_cases(golden_dir):
    """the matches the golden file records (its crafted ties), against oracle.cpu_ref.vote and the recorded results"""
    from oracle import cpu_ref as O
    c = json.load(open(os.path.join(golden_dir, "match_cases.json")))["crafted"]
    matches = [tuple(m) for m in c["matches_sorted"]]
    assert len(matches) > 0
    for topn in (1, 2, 3, 10):
        got = vote_tol(matches, 0, topn)
        assert got == [tuple(x) for x in O.vote(matches, topn)]
        assert [(s, d) for s, d, _ in got] == [(r["song_id"], r["offset"]) for r in c[f"results_top{topn}"]]


def test_tol0_is_the_oracle_vote_on_random_matches():
    from oracle import cpu_ref as O
    rng = random.Random(5)
    for _ in range(200):
        n = rng.choice([0, 1, 7, 60, 400])
        matches = [(rng.randint(1, rng.choice([1, 3, 12])), rng.randint(-8, rng.choice([-8, 2, 40]))) for _ in range(n)]
        for topn in (1, 2, 5):
            assert vote_tol(matches, 0, topn) == [tuple(x) for x in O.vote(matches, topn)]


def _m(sid, bins):
    return [(sid, d) for d, c in bins.items() for _ in range(c)]


def test_window_rules():
    song = _m(1, {10: 3, 11: 4, 13: 5})
    assert vote_tol(song, 1, 1) == [(1, 11, 7)]
    assert vote_tol(song, 2, 1) == [(1, 13, 9)]
    assert vote_tol(song, 3, 1) == [(1, 13, 12)]
    assert vote_tol(song, 31, 1) == [(1, 13, 12)]
    assert vote_tol(_m(1, {5: 2, 6: 2, 20: 3, 21: 1}), 1, 1) == [(1, 5, 4)]      # equal sums: the smaller start; equal bins: the smaller delta
    assert vote_tol(_m(1, {-3: 1, -2: 2, 0: 2}), 2, 1) == [(1, -2, 4)]           # the window [-2, 0] beats [-3, -1]; its bins tie
    assert vote_tol(_m(2, {0: 2, 1: 1}) + _m(1, {7: 3}), 1, 2) == [(1, 7, 3), (2, 0, 3)]   # equal sums: the smaller id
    assert vote_tol([], 3, 2) == []


def test_symbols_declared_exported_and_null_safe():
    from shazam_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "shz.h")).read()
    for name in ("shz_set_vote_tolerance", "shz_get_vote_tolerance"):
        assert f"int32_t {name}(" in header and name in _ffi.SIGNATURES
    assert "#define SHZ_DEBUG_VOTE_TOLERANT_ROUTE 128u" in header and _ffi.DEBUG_VOTE_TOLERANT_ROUTE == 128
    L = _ffi.lib()
    import ctypes as C
    n = C.c_uint32(7)
    assert L.shz_set_vote_tolerance(None, 1) == _ffi.E_INVALID
    assert L.shz_set_vote_tolerance(None, 32) == _ffi.E_INVALID
    assert L.shz_get_vote_tolerance(None, C.byref(n)) == _ffi.E_INVALID and n.value == 7
