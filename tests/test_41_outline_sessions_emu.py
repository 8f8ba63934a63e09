"""Outlines and polygon prompts through the model's public calls -- PSALM.segment_everything(outlines=True), segment / segment_many(outlines=True),
{"polygon": ...} region prompts in segment, segment_many and VideoTracker.start, evalout.coco_instance_records(segmentation="polygon") -- on the
tiny region model, kernels in the host emulation.  The yardsticks are the sequential oracle of tests/outlines_util.py and, for polygon prompts,
the same call with {"mask": np_fill(polygon)}; every comparison is for equality.  The tiny random-weight model's masks are empty at any size, so
the case with real shapes feeds the device step the planted picks of tests/everything_clean_util.py."""
import pytest

from outlines_util import (coco_records_case, everything_outlines_case, polygon_errors_case, polygon_prompt_case, polygon_tracker_case,
                           public_call_case)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_everything_outlines_on_planted_picks(connectivity):
    everything_outlines_case("emu", connectivity)


def test_public_calls_gain_only_the_outline_keys():
    public_call_case("emu")


def test_polygon_prompts_equal_their_filled_masks():
    polygon_prompt_case("emu")


def test_polygon_prompts_start_a_track():
    polygon_tracker_case("emu")


def test_polygon_prompt_errors():
    polygon_errors_case("emu")


def test_coco_polygon_records_and_evalout_functions():
    coco_records_case("emu")
