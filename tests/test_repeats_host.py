"""CPU: repeats.occurrences (shazam_amd/repeats.py) on built repeat lists against the plain-Python definition
in tests/repeat_twin.py, which shares no line of reasoning with the package's union-find.  Every case also states the
grouping it was built for, so that the twin is held to it as well."""
import repeat_twin
from shazam_amd import repeats


def _r(rec, first, last, lag):
    return dict(rec=rec, first=first, last=last, lag=lag)


def _occ(rp):
    got = repeats.occurrences(rp)
    assert [(g["recording"], g["intervals"]) for g in got] == repeat_twin.occurrences(rp)
    return got


# an ident of 100 frames airs at 100, 1100 and 2100: the three pairwise repeats, in the order find_repeats returns them
_IDENT = [(100, 199, 1000), (100, 199, 2000), (1100, 1199, 1000)]
_AIRS = [(100, 199), (1100, 1199), (2100, 2199)]


def test_no_repeats():
    assert _occ([]) == []


def test_three_airings_in_one_recording_are_one_group():
    got = _occ([_r(3, *p) for p in _IDENT])
    assert got == [{"recording": 3, "intervals": _AIRS, "repeats": [0, 1, 2]}]


def test_the_same_in_two_recordings_gives_two_groups():
    # the lists interleaved, the later recording first: the groups come back by recording, each with its own repeats
    rp = [_r(rec, *p) for p in _IDENT for rec in (5, 2)]
    got = _occ(rp)
    assert got == [{"recording": 2, "intervals": _AIRS, "repeats": [1, 3, 5]},
                   {"recording": 5, "intervals": _AIRS, "repeats": [0, 2, 4]}]


def test_overlap_of_exactly_half_the_shorter_interval_and_one_frame_less():
    # [0, 99] and [60, 139]: 40 of the shorter one's 80 frames overlap -- one airing, its hull [0, 139], and one group
    got = _occ([_r(0, 0, 99, 1000), _r(0, 60, 139, 3000)])
    assert got == [{"recording": 0, "intervals": [(0, 139), (1000, 1099), (3060, 3139)], "repeats": [0, 1]}]
    # [0, 99] and [61, 140]: 39 frames -- two airings, and nothing joins the two repeats
    got = _occ([_r(0, 0, 99, 1000), _r(0, 61, 140, 3000)])
    assert got == [{"recording": 0, "intervals": [(0, 99), (1000, 1099)], "repeats": [0]},
                   {"recording": 0, "intervals": [(61, 140), (3061, 3140)], "repeats": [1]}]
