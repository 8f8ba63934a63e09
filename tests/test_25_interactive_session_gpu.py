"""Region prompts given as geometry on the MI355X: the cases of tests/test_24_interactive_session_emu.py (same helpers, same bit-for-bit bars) on the
real library."""
import pytest

from interactive_util import equality_case, errors_case, ground_truth_case, pick_case, segment_many_case, unchanged_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch_decoder", [True, False])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_regions_equal_the_host_prepared_masks_gpu(precision, batch_decoder):
    equality_case("hip", precision, batch_decoder)


def test_ground_truth_is_passed_through_when_given_gpu():
    ground_truth_case("hip")


def test_picks_on_crafted_scores_gpu():
    pick_case("hip")


def test_segment_many_equals_the_loop_of_segment_calls_gpu():
    segment_many_case("hip", "f16x3")


def test_segment_without_regions_is_unchanged_gpu():
    unchanged_case("hip", "f16x3")


def test_errors_gpu():
    errors_case("hip")
