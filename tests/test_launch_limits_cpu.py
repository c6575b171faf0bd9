"""tests/launch_limits.py against the sources under libxsmm-1_amd/csrc: every clamp, slab size and index-width switch the
table lists is still spelled the way the table says, with the value the table says, and `per_trip` follows from those values.
Who raises a clamp meets this test first and moves the table (and with it the sizes taken from it) along."""
import pytest

import launch_limits as ll


ENTRIES = dict(ll.LIMITS, **ll.THRESHOLDS)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_source_still_says_what_the_size_tests_assume(name):
    bad = ll.check(ENTRIES[name])
    assert not bad, "\n".join([name] + bad)


def test_a_changed_value_and_a_lost_expression_are_noticed():
    entry = dict(ll.LIMITS["pool"])
    path, pattern, value = entry["source"][0]
    assert ll.check(dict(entry, source=[(path, pattern, value + 1)] + entry["source"][1:]))
    assert ll.check(dict(entry, source=[(path, r"gy = items < 99999 \? items", None)]))
    assert ll.check(dict(entry, per_trip=entry["per_trip"] * 2))
    for name in ("quant_layout_pair", "quant_act_tiled", "matdiff_norms"):  # a clamp shared by several entries moves each of them
        entry = ll.LIMITS[name]
        path, pattern, value = entry["source"][0]
        assert "MAX_BLOCKS" in pattern and ll.check(dict(entry, source=[(path, pattern.replace("(\\d+)", "(\\d)"), 2)] + entry["source"][1:]))


def test_sizes_are_two_trips_and_an_odd_rest():
    for name in ll.LIMITS:
        n = ll.sized(name, 37)
        assert n > 2 * ll.per_trip(name) and (n - 2 * ll.per_trip(name)) % 2 == 1
    for rest in (0, 2, 64, 128):
        with pytest.raises(AssertionError):
            ll.sized("pool", rest)
    with pytest.raises(KeyError):
        ll.sized("quant_layout_wide", 37)
