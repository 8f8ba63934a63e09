"""The cases of tests/test_31_session_fronts_emu.py on the MI355X, through the real library (same helper, same bit-for-bit bars)."""
import pytest

from fronts_util import fronts_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("what", ["referring", "host_masks", "regions"])
def test_segment_and_segment_many_issue_the_same_launches_gpu(what):
    fronts_case("hip", what)
