"""Outlines and polygon prompts through the model's public calls on the MI355X: the cases of tests/test_41_outline_sessions_emu.py on the real
kernels (the oracle runs on this call's own masks)."""
import pytest
import torch

from outlines_util import (coco_records_case, everything_outlines_case, polygon_errors_case, polygon_prompt_case, polygon_tracker_case,
                           public_call_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("connectivity", [4, 8])
def test_everything_outlines_on_planted_picks(connectivity):
    everything_outlines_case("hip", connectivity)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_public_calls_gain_only_the_outline_keys(precision):
    public_call_case("hip", precision)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_polygon_prompts_equal_their_filled_masks(precision):
    polygon_prompt_case("hip", precision)


def test_polygon_prompts_start_a_track():
    polygon_tracker_case("hip")


def test_polygon_prompt_errors():
    polygon_errors_case("hip")


def test_coco_polygon_records_and_evalout_functions():
    coco_records_case("hip")
