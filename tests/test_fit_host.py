"""Host: extent.line_fit, tempo_of and own_frames, and the plain-Python twin of the moments (tests/fit_twin.py), against brute
force on small integers.  No GPU."""
import random
from fractions import Fraction

import pytest

import fit_twin as F


@pytest.fixture(scope="module")
def X():
    from shazam_amd import extent
    return extent


def _sums(pairs, d_lo):
    """(count, sum_q, sum_u, sum_qq, sum_qu) of (q, d) pairs"""
    return (len(pairs), sum(q for q, _ in pairs), sum(d - d_lo for _, d in pairs), sum(q * q for q, _ in pairs),
            sum(q * (d - d_lo) for q, d in pairs))


def _brute_line(pairs):
    """least squares by the normal equations in Fractions, centred: no formula shared with line_fit"""
    n = len(pairs)
    mq, md = Fraction(sum(q for q, _ in pairs), n), Fraction(sum(d for _, d in pairs), n)
    sxx = sum((q - mq) ** 2 for q, _ in pairs)
    if sxx == 0:
        return None
    slope = sum((q - mq) * (d - md) for q, d in pairs) / sxx
    return slope, md - slope * mq


def test_line_fit_on_exact_lines(X):
    for slope, icpt, d_lo in ((Fraction(1, 8), 1000, 1000), (Fraction(-1, 4), 50, -10), (Fraction(0), -7, -7), (Fraction(3, 2), -100, -100)):
        pairs = [(q, icpt + slope * q) for q in range(0, 64, 8)]
        assert all(d.denominator == 1 for _, d in pairs)
        pairs = [(q, int(d)) for q, d in pairs]
        assert X.line_fit(*_sums(pairs, d_lo), d_lo) == (slope, icpt)
    assert X.tempo_of(65536, Fraction(1, 8)) == 1.125
    assert X.tempo_of(68157, Fraction(0)) == Fraction(68157, 65536)
    assert X.tempo_of(60000, Fraction(-1, 10)) == Fraction(60000, 65536) * Fraction(9, 10)


def test_line_fit_against_brute_force_and_where_there_is_no_line(X):
    rng = random.Random(5)
    for _ in range(300):
        n = rng.randint(2, 12)
        d_lo = rng.randint(-40, 40)
        pairs = [(rng.randint(0, 30), d_lo + rng.randint(0, 25)) for _ in range(n)]
        assert X.line_fit(*_sums(pairs, d_lo), d_lo) == _brute_line(pairs), pairs
    assert X.line_fit(0, 0, 0, 0, 0, 3) is None
    assert X.line_fit(*_sums([(5, 9)], 2), 2) is None                           # one pair
    assert X.line_fit(*_sums([(5, 9), (5, 11), (5, 30)], 2), 2) is None         # one q: the denominator is 0
    n = 1 << 24                                                                  # sum_qq may have wrapped: no fit
    assert X.line_fit(n, n, n, 3 * n, n, 0) is None
    assert X.line_fit(n - 1, n, n, 3 * n, n, 0) is not None


@pytest.mark.parametrize("t16", [32768, 60000, 65536, 70000, 131072])
def test_own_frames_is_the_inverse_of_the_map(X, t16):
    top = F.warp_map(299, t16)
    for first in range(top + 1):
        lo = X.own_frames(first, first, t16)[0]
        assert F.warp_map(lo, t16) >= first and (lo == 0 or F.warp_map(lo - 1, t16) < first), (t16, first)
    for t in range(300):
        last = F.warp_map(t, t16)
        hi = X.own_frames(0, last, t16)[1]
        assert F.warp_map(hi, t16) <= last < F.warp_map(hi + 1, t16) and hi >= t, (t16, t)
    for first, last in ((0, 0), (1, 1), (7, 40), (100, 100), (33, top)):        # and the twin's search gives the same
        assert X.own_frames(first, last, t16) == F.own_frames(first, last, t16, limit=700), (t16, first, last)


def test_twin_moments_against_a_loop_over_all_pairs():
    rng = random.Random(11)
    for _ in range(50):
        rows = [(rng.randint(0, 5), rng.randint(1, 3), rng.randint(0, 60)) for _ in range(40)]
        hashes = [(rng.randint(0, 5), rng.randint(0, 30)) for _ in range(15)]
        cands = [(rng.randint(1, 3), lo, lo + rng.randint(0, 40)) for lo in (rng.randint(-30, 30) for _ in range(4))]
        got = F.moments(rows, hashes, cands)
        for (sid, lo, hi), g in zip(cands, got):
            pairs = {(k, q, s, o) for k, q in hashes for kk, s, o in rows if kk == k and s == sid and lo <= o - q <= hi}
            assert g == {"sum_q": sum(p[1] for p in pairs), "sum_u": sum(p[3] - p[1] - lo for p in pairs),
                         "sum_qq": sum(p[1] ** 2 for p in pairs), "sum_qu": sum(p[1] * (p[3] - p[1] - lo) for p in pairs)}
    # modulo 2^64: 2^24 + 1 pairs at q = 2^20 - 1 would pass it; the rule is applied to the sum, shown on one huge q
    big = F.moments([(1, 1, (1 << 40) + 5)], [(1, 1 << 40)], [(1, 0, 10)])[0]
    assert big["sum_qq"] == (1 << 80) % (1 << 64) == 0 and big["sum_qu"] == (5 << 40)
