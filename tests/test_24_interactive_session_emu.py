"""Region prompts given as geometry (`regions=` of PSALM.segment / segment_many: click, box, scribble and mask prompts prepared on the device) on the
tiny region model, kernels in the host emulation.  The yardstick is the existing host path -- the prompt drawn in numpy, enhance_with_circles,
apply_segmentation, `instances.region_masks`, `region_points` -- on the same session under the same sampler: bit for bit (tests/interactive_util.py)."""
import pytest

from interactive_util import equality_case, errors_case, ground_truth_case, pick_case, segment_many_case, unchanged_case


@pytest.mark.parametrize("batch_decoder", [True, False])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_regions_equal_the_host_prepared_masks(precision, batch_decoder):
    """mask_pred, pred_masks and scores of segment(regions=...) == segment(seg_info=host masks); one launch of each of the four mask kernels; the
    picks are the first arg-max per region and that query's mask; no `gt` without ground truth"""
    equality_case("emu", precision, batch_decoder)


def test_ground_truth_is_passed_through_when_given():
    ground_truth_case("emu")


def test_picks_on_crafted_scores():
    pick_case("emu")


def test_segment_many_equals_the_loop_of_segment_calls():
    segment_many_case("emu", "fp32")


def test_segment_without_regions_is_unchanged():
    unchanged_case("emu", "fp32")


def test_errors():
    errors_case("emu")
