"""PSALM.segment and PSALM.segment_many on one request, kernels in the host emulation: the same launch names in the same order, cold and warm, but
for the suffix entry's name and segment's query of the cache size; the same results bit for bit (tests/fronts_util.py)."""
import pytest

from fronts_util import fronts_case


@pytest.mark.parametrize("what", ["referring", "host_masks", "regions"])
def test_segment_and_segment_many_issue_the_same_launches(what):
    fronts_case("emu", what)
